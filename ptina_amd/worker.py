'''
The flat, procedural face of the renderer that the Blender add-on drives through its worker thread
(reference worker.py:11-87: same function names, same arguments, same effects).  Most entries hand their
arguments to one method of one singleton: those are generated from the table below; the few with
behaviour of their own are written out.
'''

from .things import *                 # noqa: F401,F403  (callers do `from ptina.worker import *` and expect the pools' names too)
from . import things as _things
from .engine.path import PathEngine as DefaultEngine
from .engine.preview import PreviewEngine
from .common import ctx

# worker function -> (singleton class, method, the worker function's own parameters: name or (name, default)).  Pure
# pass-throughs (reference worker.py:29-30,50-87).  The parameter names are the worker API's -- callers may pass them by keyword
# (round-5 ADVICE: `fast_export_image(pixels=...)`, `load_model(vertices=...)`) -- and the values go on positionally, so the
# method behind may name its own parameters as it likes.
_PASS_THROUGH = {
    'set_size': ('FilmTable', 'set_size', ('nx', 'ny')),
    'get_image': ('FilmTable', 'get_image', (('id', 0),)),
    'fast_export_image': ('FilmTable', 'fast_export_image', ('pixels', ('id', 0))),
    'clear_lights': ('LightPool', 'clear', ()),
    'set_world_light': ('WorldLight', 'set', ('fac', 'tex')),
    'add_light': ('LightPool', 'add', ('world', 'color', 'size', 'type')),
    'load_model': ('ModelPool', 'load', ('vertices', 'mtlids')),
    # (no reference counterparts: the meshes and the object table stay on the device, model.py)
    'load_meshes': ('ModelPool', 'load_meshes', ('primitives',)),
    'set_object_world': ('ModelPool', 'set_world', ('obj', 'world')),
    'set_object_morph_weights': ('ModelPool', 'set_morph_weights', ('obj', 'w')),
    'set_object_joints': ('ModelPool', 'set_joints', ('obj', 'mats')),
    'set_mesh_skeleton': ('ModelPool', 'add_skeleton', ('mesh', 'parents', 'rest_translation', 'rest_rotation', 'rest_scale', 'inverse_bind')),
    'add_mesh_clip': ('ModelPool', 'add_clip', ('mesh', 'tracks')),
    'set_object_animation': ('ModelPool', 'set_animation', ('obj', 'clip', ('offset', 0.0), ('speed', 1.0), ('loop', True))),
    'set_scene_time': ('ModelPool', 'set_time', ('t',)),
    'set_object_animation_blend': ('ModelPool', 'set_animation_blend', ('obj', 'clip', ('offset', 0.0), ('speed', 1.0), ('loop', True), ('weight', 1.0), ('fade', None))),
    'add_object_clip': ('ModelPool', 'add_object_clip', ('tracks',)),
    'set_object_motion': ('ModelPool', 'set_motion', ('obj', 'clip', ('offset', 0.0), ('speed', 1.0), ('loop', True), ('rest', None), ('base', None))),
    'set_object_parent': ('ModelPool', 'set_parent', ('obj', 'parent', ('joint', None))),
    'set_mesh_subdivision': ('ModelPool', 'add_subdivision', ('mesh', 'levels', ('creases', None), ('corners', None), ('scheme', 'loop'), ('polys', None))),
    'set_mesh_displacement': ('ModelPool', 'add_displacement', ('mesh', 'image', ('strength', 1.0), ('midlevel', 0.5), ('mode', 'normal'), ('channel', 'mean'))),
    'set_mesh_displacement_params': ('ModelPool', 'set_displacement', ('mesh', 'strength', ('midlevel', None))),
    'add_scatter': ('ModelPool', 'add_scatter', ('surface', 'mesh', 'count', ('seed', 0), ('mtlid', None), ('scale', (1, 1)), ('align', 'normal'), ('up', (0, 1, 0)),
                                                 ('random_yaw', True), ('density', None), ('channel', 'mean'), ('min_distance', 0.0), ('candidates', None))),
    'rescatter': ('ModelPool', 'rescatter', ('scatter', ('seed', None))),
    'load_images': ('ImagePool', 'load', ('images',)),
    'load_materials': ('MaterialPool', 'load', ('materials',)),
    'build_tree': ('BVHTree', 'build', ()),
    'set_camera': ('Camera', 'set_perspective', ('pers',)),
}


def _pass_through(name, owner, method, params):
    import inspect
    P = inspect.Parameter
    sig = inspect.Signature([P(p, P.POSITIONAL_OR_KEYWORD) if isinstance(p, str) else P(p[0], P.POSITIONAL_OR_KEYWORD, default=p[1])
                             for p in params])

    def call(*args, **kwargs):
        bound = sig.bind(*args, **kwargs)           # (TypeError for a missing / unknown / doubled argument, like a plain def)
        bound.apply_defaults()
        return getattr(getattr(_things, owner)(), method)(*bound.args)
    call.__name__ = call.__qualname__ = name
    call.__signature__ = sig
    call.__doc__ = '%s().%s%s' % (owner, method, sig)
    return call


for _name, (_owner, _method, _params) in _PASS_THROUGH.items():
    globals()[_name] = _pass_through(_name, _owner, _method, _params)


def init():
    '''every pool, then both engines (reference worker.py:11-14)'''
    init_things()
    for engine in (DefaultEngine, PreviewEngine):
        engine()


def synchronize():
    '''the reference forces a device sync by reading a field back (worker.py:17-18); here the C ABI has the call'''
    ctx().call('mpt_synchronize')


def compose_model():
    '''ModelPool().compose(): after set_object_world, rewrite the moved objects' faces on the device; build_tree() follows (no
    reference counterpart: its add-on runs compose_multiple_meshes + load_model over everything again)'''
    ModelPool().compose()


def refit_tree():
    '''BVHTree().refit(): after compose_model() (or load_model of as many faces), keep the built trees and fit their boxes to the
    moved model on the device; returns the growth of the tree's cost since it was built (no reference counterpart: its add-on
    builds again)'''
    return BVHTree().refit()


def update_tree(max_growth=None):
    '''BVHTree().update(max_growth): refit where that is allowed and the tree has not grown past max_growth (None: the default),
    build otherwise; returns 'refit' or 'build', whichever ran last'''
    return BVHTree().update() if max_growth is None else BVHTree().update(max_growth)


def keep_history():
    '''FilmTable().keep_history(): remember the rendered view on the device, before the scene or the camera is edited (no
    reference counterpart: its add-on clears the film at every change)'''
    FilmTable().keep_history()


def reproject(max_history=32, depth_tol=0.02):
    '''FilmTable().reproject(max_history, depth_tol): after the edit and update_tree(), carry the accumulated film over to the new
    view instead of clear(); returns the HistoryResult (how many pixels kept their history)'''
    return FilmTable().reproject(max_history, depth_tol)


def intersect(o, d, avoid=None):
    '''BVHTree().intersect(o, d, avoid): the closest hits of a batch of rays against the built tree -- a dict of arrays hit, depth,
    index, u, v, object (the reference asks its tree one ray at a time, inside a kernel: lbvh.py:314-347)'''
    return BVHTree().intersect(o, d, avoid)


def occluded(o, d, dis=float('inf'), avoid=None):
    '''BVHTree().occluded(o, d, dis, avoid): for each ray of a batch, is anything within dis along it?'''
    return BVHTree().occluded(o, d, dis, avoid)


def pick(x, y):
    '''BVHTree().pick(x, y): (object, face, depth) under clip point (x, y) of the camera, or None -- the object to hand to
    set_object_world'''
    return BVHTree().pick(x, y)


def render(aa=True):
    DefaultEngine().render()


def render_preview(aa=True):
    PreviewEngine().render()


def get_denoised(**kw):
    '''FilmTable().get_denoised(**kw), the keywords and defaults of _lib.denoise_params and variance=None: pass 0 filtered on the device, guided by the passes render_preview() fills and, with variance=sigma, by the film's own noise since the mark (no reference counterpart: its add-on leaves that to Blender)'''
    return FilmTable().get_denoised(**kw)


def get_display(**kw):
    '''FilmTable().get_display(id=0, denoised=False, op='aces', transfer='srgb', layout='film', dither=True, exposure=None, key=0.18,
    white=4.0, gamma=2.2, variance=None, **denoise_kw): the film tone-mapped and quantised to 8-bit RGBA on the device (no reference counterpart)'''
    return FilmTable().get_display(**kw)


def get_noise(threshold, **kw):
    '''FilmTable().get_noise(threshold, map=False, remark=False): the film's noise estimate against the mark FilmTable().mark() took,
    on the device (no reference counterpart)'''
    return FilmTable().get_noise(threshold, **kw)


def render_until(noise, max_spp, **kw):
    '''engine.render_until(DefaultEngine(), noise, max_spp, min_spp=16, fraction=0.0, keep_mark=False) -- DefaultEngine().render_until's
    loop: render on a doubling schedule until the noise estimate passes or max_spp frames are spent; expects a cleared film;
    keep_mark=True leaves the mark of the last check for get_denoised(variance=...) (no reference counterpart: its loop counts samples)'''
    from .engine import render_until as loop
    return loop(DefaultEngine(), noise, max_spp, **kw)


def render_adaptive(noise, max_spp, **kw):
    '''engine.render_adaptive(DefaultEngine(), noise, max_spp, min_spp=16, fraction=0.0, dilate=1, switch=None) -- DefaultEngine().render_adaptive's
    loop: render_until's schedule, sampling only the pixels whose estimate has not passed yet; expects a cleared film; leaves a mark
    for get_denoised(variance=...) (no reference counterpart: its loop counts samples)'''
    from .engine import render_adaptive as loop
    return loop(DefaultEngine(), noise, max_spp, **kw)


def get_size():
    film = FilmTable()
    return film.nx, film.ny


def clear(id=0):
    '''an engine that keeps state of its own between frames (the reference's MLT engine) is reset with the film'''
    reset = getattr(DefaultEngine(), 'reset', None)
    if callable(reset):
        reset()
    FilmTable().clear(id)


def set_mlt_param(lsp, sigma):
    '''Metropolis parameters: the MLT engine is outside this package's scope, so with PathEngine as the default
    engine they find nothing to set -- accepted and ignored, as in the reference (worker.py:45-49)'''
    engine = DefaultEngine()
    for attr, value in (('LSP', lsp), ('Sigma', sigma)):
        if attr in dir(engine):
            setattr(engine, attr, value)

'''
GPU tests (-m gpu) of the device composition (ModelPool.load_meshes / add_mesh / add_object / set_world / set_material / compose,
mpt_mesh_add ... mpt_compose; ptina_amd/csrc/compose.hip, scene_compose.cpp).

The kernel is held to the reference's own executed output (tests/golden/reference_compose.npz, made by
tests/golden/make_reference_compose_golden.py from the reference's compose_multiple_meshes) BIT FOR BIT: the fixture's values lie
more than compose_ref.MARGIN a-priori error bounds of an f64 evaluation away from every f32 rounding boundary
(tests/test_compose_cpu.py re-asserts it), so an f64 evaluation in any order rounds to the same f32 numbers.
'''

import os

import numpy as np
import pytest

import compose_ref

pytestmark = pytest.mark.gpu
u32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX = NY = 32
SPP = 4


@pytest.fixture(scope='module')
def gold():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_compose.npz'))
    prims = compose_ref.fixture_primitives(g)
    return prims, g['out_verts'].astype(np.float32), g['out_mtlids'].astype(np.int32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u32), b.view(u32))


def _pool():
    from ptina_amd.things import ModelPool
    return ModelPool()


def _ctx():
    from ptina_amd.common import ctx
    return ctx()


def _start(mode='fast', things_only=False):
    '''a fresh context with film, materials, camera and engine set up; the model is the test's'''
    from ptina_amd import scenes, _lib
    from ptina_amd.common import reset_all
    from ptina_amd.things import init_things, FilmTable, MaterialPool, Camera
    from ptina_amd.engine.path import PathEngine
    reset_all()
    init_things()
    if things_only:
        return None
    eng = PathEngine()
    _ctx().set_option('mode', _lib.MODE_STRICT if mode == 'strict' else _lib.MODE_FAST)
    FilmTable().set_size(NX, NY)
    MaterialPool().load(list(scenes.WALL_MATERIALS) + [scenes.material(basecolor=(0.8, 0.6, 0.2), roughness=0.3),
                                                       scenes.material(basecolor=(0.2, 0.3, 0.8), roughness=0.6, metallic=0.3),
                                                       scenes.material(basecolor=(0.7, 0.7, 0.7), roughness=0.4)])
    Camera().set_perspective(scenes.BENCH_CAMERA)
    return eng


def _build_render(eng):
    '''(raw film pass 0, the tree's arrays)'''
    from ptina_amd.things import FilmTable, BVHTree
    BVHTree().build()
    eng.render(SPP)
    raw = FilmTable().get_raw().copy()
    assert np.all(raw.reshape(-1, 4)[:, 3] == SPP)
    return raw, BVHTree().to_numpy()


def _same_tree(a, b):
    return a['depth'] == b['depth'] and all(_same(a[k], b[k]) for k in ('child', 'leaf', 'bmin', 'bmax', 'mc'))


def _sphere(info):
    return np.array([*info.scene_cen, info.scene_rad], np.float64).view(np.uint64).tolist()


def _edited(prims, obj, world=None, mtl='keep'):
    p, n, t, w, m = prims[obj]
    out = list(prims)
    out[obj] = (p, n, t, w if world is None else world, m if mtl == 'keep' else mtl)
    return out


def _move(w, k):
    '''another world matrix for the same object: a rotation about y and a shift in front of what there was'''
    th = 0.3 + 0.1 * k
    r = np.array([[np.cos(th), 0, np.sin(th), 0.25], [0, 1, 0, -0.125 * k], [-np.sin(th), 0, np.cos(th), 0.5], [0, 0, 0, 1]])
    return r @ w


# ---------------------------------------------------------------- 1, 2: the reference's output, and the bounding sphere
def test_load_meshes_gives_the_reference_output_bit_for_bit(fresh, gold):
    prims, want_v, want_m = gold
    _start(things_only=True)
    objs = _pool().load_meshes(prims)
    assert objs == list(range(9)) and _pool().nfaces == 621
    got_v, got_m = _pool().to_numpy()
    bad = np.flatnonzero((got_v.view(u32) != want_v.view(u32)).any(axis=1))
    print('compose: %d of %d vertex records differ from the reference' % (bad.size, want_v.shape[0]))
    assert got_v.dtype == np.float32 and got_v.shape == want_v.shape and bad.size == 0, (bad[:8], got_v[bad[:2]], want_v[bad[:2]])
    assert got_m.dtype == np.int32 and np.array_equal(got_m, want_m)
    info = _pool().compose_stats()
    assert (info.faces, info.recomposed, info.dirty_objects, info.host_fetches) == (621, 621, 9, 1)
    _pool().to_numpy()
    assert _pool().compose_stats().host_fetches == 1                           # fetched once


def test_bounding_sphere_equals_the_host_path(fresh, gold):
    prims, want_v, want_m = gold
    _start(things_only=True)
    _pool().load_meshes(prims)
    a = _sphere(_pool().compose_stats())
    _start(things_only=True)
    _pool().load(want_v, want_m)
    b = _sphere(_pool().compose_stats())
    assert a == b and _pool().compose_stats().scene_rad > 1.0


# ---------------------------------------------------------------- 3: end to end, through the lazy host copy (621 faces: the host SAH pass)
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_composed_model_builds_and_renders_like_the_loaded_one(fresh, gold, mode):
    prims, want_v, want_m = gold
    eng = _start(mode)
    _pool().load_meshes(prims)
    assert _pool().compose_stats().host_fetches == 0
    film_a, tree_a = _build_render(eng)
    assert _pool().compose_stats().host_fetches == 1                           # the host SAH pass read the model
    eng = _start(mode)
    _pool().load(want_v, want_m)
    film_b, tree_b = _build_render(eng)
    assert _pool().compose_stats().host_fetches == 0
    assert np.count_nonzero(film_b.reshape(-1, 4)[:, :3].sum(axis=1)) > NX * NY // 8, 'the film shows nothing'
    assert _same_tree(tree_a, tree_b)
    assert _same(film_a, film_b)


# ---------------------------------------------------------------- 4: partial recompose
@pytest.mark.parametrize('moved,painted', [(3, 6), (0, 8), (8, 0), (5, 5)])
def test_partial_recompose_equals_a_fresh_composition(fresh, gold, moved, painted):
    '''a mid-list pair, the first and the last object either way, and one object both moved and painted'''
    prims, _, _ = gold
    faces = [p[0].shape[0] for p in prims]
    _start(things_only=True)
    pool = _pool()
    pool.load_meshes(prims)
    before_v, before_m = pool.to_numpy()
    w = _move(prims[moved][3], moved)
    pool.set_world(moved, w)
    pool.set_material(painted, 7)
    pool.compose()
    info = pool.compose_stats()
    want_faces = faces[moved] + (faces[painted] if painted != moved else 0)
    assert (info.faces, info.recomposed, info.dirty_objects) == (621, want_faces, 1 if painted == moved else 2)
    got_v, got_m = pool.to_numpy()
    sphere = _sphere(info)
    edited = _edited(_edited(prims, moved, world=w), painted, mtl=7)
    pool.load_meshes(edited)
    assert pool.compose_stats().recomposed == 621
    want_v, want_m = pool.to_numpy()
    assert _same(got_v, want_v) and np.array_equal(got_m, want_m)
    assert sphere == _sphere(pool.compose_stats())                             # the untouched workgroups' partial boxes were kept
    first = np.concatenate([[0], np.cumsum(faces)])
    lo, hi = 3 * first[moved], 3 * first[moved + 1]
    changed = (got_v.view(u32) != before_v.view(u32)).any(axis=1)
    assert changed[lo:hi].all() and not changed[:lo].any() and not changed[hi:].any()
    assert np.array_equal(np.flatnonzero(got_m != before_m), np.arange(first[painted], first[painted + 1]))
    pool.compose()                                                             # nothing changed: nothing is written
    info = pool.compose_stats()
    assert (info.recomposed, info.dirty_objects) == (0, 0) and sphere == _sphere(info)


# ---------------------------------------------------------------- 5: above the host passes' limit
def test_grid_scene_edit_and_rebuild_stays_on_the_device(fresh):
    from ptina_amd.multimesh import compose_multiple_meshes
    prims, (obj, world) = compose_ref.grid_scene()
    edited = _edited(prims, obj, world=world)
    ref, ref_m = compose_multiple_meshes(prims)
    ref_e, _ = compose_multiple_meshes(edited)
    for which, (pr, out) in (('grid', (prims, ref)), ('edited grid', (edited, ref_e))):    # the precondition, on this test's own inputs
        worst, closest, count = compose_ref.margin(pr, out)
        print('%s: %d values, the closest %.3g error bounds (%.3g f32 ulp) from an f32 rounding boundary' % (which, count, worst, closest))
        assert worst > compose_ref.MARGIN, 'precondition: pick another compose_ref.GRID_SEED'
    assert ref_m.shape[0] == 18432
    eng = _start('fast')
    pool = _pool()
    objs = pool.load_meshes(prims)
    assert len(objs) == 9 and len(pool._mesh_faces) == 3 and pool.nfaces == 18432
    from ptina_amd.things import BVHTree
    BVHTree().build()
    pool.set_world(obj, world)
    pool.compose()
    info = pool.compose_stats()
    assert (info.faces, info.recomposed, info.dirty_objects) == (18432, 2048, 1)
    film_a, tree_a = _build_render(eng)
    assert _ctx().get_option('sah_fallback') == 0 and _ctx().get_option('sah_levels') > 0      # the device SAH pass ran
    assert pool.compose_stats().host_fetches == 0                              # two compositions, two builds, a render: nothing fetched
    got_e, got_em = pool.to_numpy()
    assert _same(got_e, ref_e.astype(np.float32)) and np.array_equal(got_em, ref_m)
    pool.set_world(obj, prims[obj][3])                                         # ... and back: the first composition
    pool.compose()
    got, got_m = pool.to_numpy()
    assert _same(got, ref.astype(np.float32)) and np.array_equal(got_m, ref_m)
    eng = _start('fast')
    _pool().load(ref_e.astype(np.float32), ref_m.astype(np.int32))
    film_b, tree_b = _build_render(eng)
    assert np.count_nonzero(film_b.reshape(-1, 4)[:, :3].sum(axis=1)) > NX * NY // 8, 'the film shows nothing'
    assert _same_tree(tree_a, tree_b)
    assert _same(film_a, film_b)


# ---------------------------------------------------------------- 6: mpt_load_model takes the model back
def test_load_after_compose_restores_the_host_model(fresh, gold):
    from ptina_amd import scenes
    prims, _, _ = gold
    v, m, _, _ = scenes.scene_s978()
    eng = _start('fast')
    _pool().load(v, m)
    film_a, tree_a = _build_render(eng)
    eng = _start('fast')
    _pool().load_meshes(prims)
    from ptina_amd.things import BVHTree
    BVHTree().build()
    _pool().load(v, m)
    film_b, tree_b = _build_render(eng)
    got_v, got_m = _pool().to_numpy()
    assert _same(got_v, v) and np.array_equal(got_m, m) and _pool().nfaces == 978
    assert _same_tree(tree_a, tree_b) and _same(film_a, film_b)
    fetched = _pool().compose_stats().host_fetches
    _pool().load_meshes(prims)                                                 # and composition takes it again: everything is written
    info = _pool().compose_stats()
    assert (info.faces, info.recomposed, info.host_fetches) == (621, 621, fetched)


def test_library_refusals(fresh, gold):
    '''worded like mpt_load_model's: capacity, material ids, unknown ids, a matrix that is not finite'''
    import ctypes as C
    from ptina_amd import _lib
    from ptina_amd.common import reset_all
    from ptina_amd.things import init_things
    reset_all()
    init_things(max_faces=100, max_materials=8)
    c = _ctx()
    rec = np.zeros((60 * 3, 8), np.float32)
    eye = np.eye(4)
    wp = lambda w: np.ascontiguousarray(w, np.float64).ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    mesh, obj = C.c_int(-1), C.c_int(-1)
    c.call('mpt_mesh_add', _lib.fptr(rec), 60, C.byref(mesh))
    with pytest.raises(RuntimeError, match='too many faces'):
        c.call('mpt_mesh_add', _lib.fptr(rec), 100, C.byref(mesh))
    for bad, what in ((8, 'material id 8 outside'), (-2, 'material id -2 outside')):
        with pytest.raises(RuntimeError, match=what):
            c.call('mpt_object_add', 0, wp(eye), bad, C.byref(obj))
    with pytest.raises(RuntimeError, match='unknown mesh 1'):
        c.call('mpt_object_add', 1, wp(eye), 0, C.byref(obj))
    nan = eye.copy()
    nan[2, 1] = np.inf
    with pytest.raises(RuntimeError, match='not finite'):
        c.call('mpt_object_add', 0, wp(nan), 0, C.byref(obj))
    c.call('mpt_object_add', 0, wp(eye), 7, C.byref(obj))
    assert obj.value == 0
    with pytest.raises(RuntimeError, match='unknown object 1'):
        c.call('mpt_object_set_world', 1, wp(eye))
    with pytest.raises(RuntimeError, match='unknown object -1'):
        c.call('mpt_object_set_material', -1, 0)
    with pytest.raises(RuntimeError, match='not finite'):
        c.call('mpt_object_set_world', 0, wp(nan))
    with pytest.raises(RuntimeError, match='material id 8 outside'):
        c.call('mpt_object_set_material', 0, 8)
    c.call('mpt_compose')
    c.call('mpt_object_add', 0, wp(eye), -1, C.byref(obj))                      # 120 faces
    with pytest.raises(RuntimeError, match='too many faces'):
        c.call('mpt_compose')
    n = C.c_int(-1)
    c.call('mpt_get_model', None, None, 0, C.byref(n))
    assert n.value == 60                                                       # the refused composition left the model alone
    c.call('mpt_scene_clear', 0)
    c.call('mpt_compose')
    c.call('mpt_get_model', None, None, 0, C.byref(n))
    assert n.value == 0

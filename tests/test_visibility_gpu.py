'''
Primary rays of every kernel, held to an exhaustive search in float64 (-m gpu).  An absorbing scene (every material
basecolor 0, transmission 1; no lights; a constant world light) makes a film a hit mask: after 8 frames a raw pixel is
bit for bit (0, 0, 0, 8) if all of its camera rays hit something and (8, 4, 2, 8) if none did -- tests/visibility_ref.py
says why, and which pixels it can decide without a tree or a sampler.  Every classified pixel of every film must agree:
no share of outliers, no other kernel as the witness.  The scenes, the caps on how much the reference classifies and the
checks are those of tests/test_visibility_ref_cpu.py, where the oracle's own walk passes them with zero wrong pixels.

1  PathEngine: the strict build and every production kernel (last_kernel asserted) at 2 .. 20000 triangles, over every tree
   builder, on a model moved far from the origin, one 1024 times the size, and a flat one
2  the plain SHADE instantiation (opaque materials, exactly one light; scene_feat and shade_inst asserted): the full-miss
   pixels (a false hit shows there whatever the material)
3  the spill path of the gather walk's stack (libmiptina_spilltest.so): against truth, and bit for bit the normal library
4  BruteEngine    5  the Metropolis path door    6  PreviewEngine: the NEAREST triangle's material, exactly
In the production build the last three walk the binary fnode records (the strict build walks snode, the reference's own
tree).  Up to 8192 triangles the default SAH pass is the host's; each of the three also runs with sah_build = 1, and then
n1025 and n5000 are sizes where the device pass's binned levels wrote those records.
7  the 64-level instantiations of every one-lane-per-item kernel -- the gather render kernels, BruteEngine, the Metropolis path
   door and chain kernel, the list pass, PreviewEngine -- on `deep`, whose tree needs more than 32 stack levels (asserted first)
'''

import os
import subprocess
import sys

import numpy as np
import pytest

from test_visibility_ref_cpu import WORLD, PREVIEW_CASES, case, assert_mask, preview_errors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 8

# selection: (build, render options, last_kernel on a scene that fits LDS, on one that does not; None: cannot serve / n/a)
SELECTIONS = {
    'strict': ('strict', {}, None, None),
    'default': ('fast', {}, 5, 2),
    'lds_binary': ('fast', {'lds_wide': 0}, 1, None),
    'gather_binary': ('fast', {'lds': 0, 'wide': 0}, 0, 0),
    'gather_wide_8bit': ('fast', {'lds': 0}, 2, 2),
    'gather_wide_exact': ('fast', {'lds': 0, 'wide_quant': 0}, 2, 2),
}
FITS_LDS = ('n2', 'n3', 'n33', 'n300', 'n1025', 'moved', 'x1024', 'flat')     # below 4095 triangles (lds_layout.h)
SIZES = ['n2', 'n3', 'n33', 'n300', 'n1025', 'n5000', 'n20000']
# (option sah_build is -1 by default: the host pass up to 8192 triangles, the device pass above.  'device_sah' asks for the device pass
# where the default would not take it: at n1025 its binned levels write the binary records)
SAH_PASSES = {'default_sah': None, 'device_sah': {'sah_build': 1}}      # for the engines that walk the binary records
TREES = {'lbvh': {'tree': 0}, 'host_sah': {'sah_build': 0}, 'device_sah': {'sah_build': 1}, 'host_collapse': {'wide_build': 0}}


def _setup(c, mode, tree=None, scene=None, lights=()):
    '''a context with the case's scene, camera and world light, no lights unless given; tree options are set before the
    build they steer'''
    from helpers import setup_engine
    from ptina_amd.common import ctx
    from ptina_amd.things import BVHTree
    eng = setup_engine(scene or c.scene, c.nx, c.ny, mode=mode, camera=c.camera, lights=list(lights), world=WORLD)
    if tree:
        for key, value in tree.items():
            ctx().set_option(key, value)
        BVHTree().build()
    return eng


def _path_film(c, selection, tree=None, scene=None):
    from ptina_amd.common import ctx
    from ptina_amd.things import FilmTable
    mode, opts, fit, nofit = SELECTIONS[selection]
    eng = _setup(c, mode, tree, scene)
    for key, value in opts.items():
        ctx().set_option(key, value)
    eng.render(FRAMES)
    raw = FilmTable().get_raw().copy()
    if mode != 'strict':
        want = fit if c.name in FITS_LDS else nofit
        assert ctx().get_option('last_kernel') == want, f'{c.name} {selection}: last_kernel {ctx().get_option("last_kernel")}, expected {want}'
    return raw


def _cases(names):
    return [(name, sel) for name in names for sel in SELECTIONS if sel != 'lds_binary' or name in FITS_LDS]


# ---------------------------------------------------------------- 1. PathEngine, every kernel
@pytest.mark.parametrize('name,selection', _cases(SIZES))
def test_path_engine_every_kernel_every_size(fresh, name, selection):
    '''n2 / n3: 4-wide nodes with unused slots; n1025: the first size with a binned SAH level; n5000 / n20000 do not fit LDS'''
    c = case(name)
    c.shares()
    assert_mask(c, _path_film(c, selection), FRAMES, f'{name} {selection}')


@pytest.mark.parametrize('tree', list(TREES))
@pytest.mark.parametrize('name,selection', _cases(['n300', 'n1025']))
def test_path_engine_over_every_tree_builder(fresh, name, selection, tree):
    c = case(name)
    c.shares()
    assert_mask(c, _path_film(c, selection, TREES[tree]), FRAMES, f'{name} {selection} {TREES[tree]}')


@pytest.mark.parametrize('selection', ['strict', 'default', 'lds_binary', 'gather_wide_8bit', 'gather_wide_exact'])
@pytest.mark.parametrize('name', ['moved', 'x1024', 'flat'])
def test_path_engine_moved_scaled_and_flat_models(fresh, name, selection):
    c = case(name)
    c.shares()
    assert_mask(c, _path_film(c, selection), FRAMES, f'{name} {selection}')


# ---------------------------------------------------------------- 2. the plain instantiation
def test_plain_shade_instantiation_has_no_false_hit(fresh):
    '''opaque wall materials (no clearcoat or transmission bit) and exactly ONE light (no light at all sets the many-lights
    bit): the scene's feature mask is empty and the LDS kernel runs its plain SHADE.  The light is a small sphere behind the
    camera, which no camera ray can meet, and a camera ray that misses ends its path before any light is sampled: a hit pixel
    holds bounced light, a full-miss pixel must still be exactly the world colour'''
    from ptina_amd.tools.matrix import translate
    from ptina_amd import scenes
    from ptina_amd.common import ctx
    from ptina_amd.things import FilmTable
    c = case('n300')
    _, miss = c.shares()
    v, m, _, im = c.scene
    light = (translate([0.0, 2.0, 20.0]), np.array([8.0, 8.0, 8.0]), 0.1, 'POINT')      # the eye is at z = 5.37 and looks down -z
    eng = _setup(c, 'fast', scene=(v, m, list(scenes.WALL_MATERIALS), im), lights=[light])
    assert ctx().get_option('scene_feat') == 0
    eng.render(FRAMES)
    raw = FilmTable().get_raw().reshape(c.nx, c.ny, 4)
    assert ctx().get_option('last_kernel') == 5 and np.all(raw[..., 3] == FRAMES)
    assert ctx().get_option('scene_feat') == 0 and ctx().get_option('shade_inst') == 0, 'the plain instantiation did not run'
    bad = np.argwhere(miss & (raw != np.array([8, 4, 2, 8], np.float32)).any(axis=-1))
    assert bad.shape[0] == 0, f'plain SHADE: {bad.shape[0]} full-miss pixels are not the world colour; first {tuple(bad[0])}: {raw[tuple(bad[0])].tolist()}'
    assert (raw[~miss][:, :3] != np.array([8, 4, 2], np.float32)).any()        # (the scene is not empty)


# ---------------------------------------------------------------- 3. the spill path
_SPILL_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from ptina_amd.common import reset_all
from test_visibility_ref_cpu import case
from test_visibility_gpu import _path_film
films = {}
for sel in ('gather_wide_8bit', 'gather_wide_exact'):
    reset_all()
    films[sel] = _path_film(case('n1025'), sel)
reset_all()
np.savez(sys.argv[2], **films)
for path in sorted({line.split()[-1] for line in open('/proc/self/maps') if 'libmiptina' in line}):
    print('LOADED', path)
print('DONE')
'''


def test_spilled_stacks_against_truth_and_the_normal_library(fresh, tmp_path):
    '''libmiptina_spilltest.so keeps 4 stack levels per lane and spills the rest to the global strips: push / pop beyond CAP
    and the divergent branch of stage_node4 near CAP run for every ray of the 1025-triangle scene.  Same tree, same visiting
    order, only where the stack lives differs: the film is the normal library's bit for bit, and both are the truth'''
    from ptina_amd.common import reset_all
    lib = os.path.join(ROOT, 'ptina_amd', 'libmiptina_spilltest.so')
    assert os.path.exists(lib), 'build it with make -C ptina_amd/csrc spilltest (__graft_entry__.build() does)'
    script, out = tmp_path / 'spill.py', tmp_path / 'spill.npz'
    script.write_text(_SPILL_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=dict(os.environ, MIPTINA_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'DONE' in r.stdout, r.stdout + r.stderr
    loaded = [line.split(' ', 1)[1] for line in r.stdout.splitlines() if line.startswith('LOADED ')]
    assert [os.path.realpath(x) for x in loaded] == [os.path.realpath(lib)], f'the child process mapped {loaded}, not only {lib}'
    spilled = np.load(out)
    c = case('n1025')
    for sel in ('gather_wide_8bit', 'gather_wide_exact'):
        assert_mask(c, spilled[sel], FRAMES, f'spilltest library, {sel}')
        reset_all()
        normal = _path_film(c, sel)
        assert_mask(c, normal, FRAMES, f'normal library, {sel}')
        diff = np.flatnonzero((spilled[sel].view(np.uint32) != normal.view(np.uint32)).any(axis=1))
        assert diff.size == 0, (f'{sel}: the spilltest film differs from the normal library\'s in {diff.size} pixels; first {divmod(int(diff[0]), c.ny)}: '
                                f'{spilled[sel][diff[0]].tolist()} against {normal[diff[0]].tolist()}')


# ---------------------------------------------------------------- 4. BruteEngine
@pytest.mark.parametrize('sah', list(SAH_PASSES))
@pytest.mark.parametrize('mode', ['strict', 'fast'])
@pytest.mark.parametrize('name', ['n300', 'n1025', 'n5000'])
def test_brute_engine(fresh, name, mode, sah):
    from ptina_amd.engine.brute import BruteEngine
    from ptina_amd.things import FilmTable
    c = case(name)
    c.shares()
    _setup(c, mode, SAH_PASSES[sah])
    BruteEngine().render(FRAMES)
    assert_mask(c, FilmTable().get_raw(), FRAMES, f'brute {mode} {name} {sah}')


# ---------------------------------------------------------------- 5. the Metropolis path door
def _door_points(c, hit, miss):
    '''nine screen points in each of up to 4096 classified pixels, as the door's 32-vectors -> (X, pi, pj)'''
    rng = np.random.default_rng(c.n)
    ij = np.argwhere(hit | miss)
    ij = ij[rng.permutation(ij.shape[0])[:4096]]
    u, v = [a.reshape(-1) for a in np.meshgrid([0.1, 0.5, 0.9], [0.1, 0.5, 0.9], indexing='ij')]
    pi, pj = np.repeat(ij[:, 0], 9), np.repeat(ij[:, 1], 9)
    X = rng.random((pi.shape[0], 32), dtype=np.float32)
    X[:, 0] = (pi + np.tile(u, ij.shape[0])) / c.nx
    X[:, 1] = (pj + np.tile(v, ij.shape[0])) / c.ny
    return X, pi, pj


@pytest.mark.parametrize('sah', list(SAH_PASSES))
@pytest.mark.parametrize('mode', ['strict', 'fast'])
@pytest.mark.parametrize('name', ['n1025', 'n5000'])
def test_metropolis_path_door(fresh, name, mode, sah):
    from ptina_amd.engine.mltpath import mlt_trace
    c = case(name)
    hit, miss = c.shares()
    X, pi, pj = _door_points(c, hit, miss)
    _setup(c, mode, SAH_PASSES[sah])
    rgb = mlt_trace(X)
    want = np.where(hit[pi, pj][:, None], np.zeros(3, np.float32), np.array([1, 0.5, 0.25], np.float32)).astype(np.float32)
    bad = np.flatnonzero((rgb.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert hit[pi, pj].any() and miss[pi, pj].any()
    assert bad.size == 0, (f'mlt_trace {mode} {name} {sah}: {bad.size} of {X.shape[0]} rays wrong; first: screen point {X[bad[0], :2].tolist()} of pixel '
                           f'({pi[bad[0]]}, {pj[bad[0]]}) gives {rgb[bad[0]].tolist()}, want {want[bad[0]].tolist()}')


# ---------------------------------------------------------------- 6. preview: the nearest triangle's material
@pytest.mark.parametrize('tree', ['device_sah', 'host_sah', 'lbvh'])
@pytest.mark.parametrize('mode', ['strict', 'fast'])
@pytest.mark.parametrize('name', PREVIEW_CASES)
def test_preview_names_the_nearest_material(fresh, name, mode, tree):
    '''63 grey materials (k + 1) / 64: three preview frames sum to exactly 3 (k + 1) / 64 where the nearest material is k.  The
    closest-hit check -- ordering, tbest culling, near / far choice -- of the binary walk over fnode'''
    from ptina_amd.engine.preview import PreviewEngine
    from ptina_amd.things import FilmTable
    c = case(name, preview=True)
    c.shares()
    c.materials()
    _setup(c, mode, {'device_sah': {'tree': 1, 'sah_build': 1}, 'host_sah': {'tree': 1, 'sah_build': 0}, 'lbvh': {'tree': 0}}[tree])
    for _ in range(3):
        PreviewEngine().render()
    bad = preview_errors(c, FilmTable().get_raw(1), 3, f'preview {mode} {name} {tree}')
    assert not bad, f'{len(bad)} wrong pixels; ' + '; '.join(bad[:4])


# ---------------------------------------------------------------- 7. the 64-level instantiations
def _deep(mode, scene=None):
    '''`deep` set up in the strict build or in the production build over the LBVH (option tree = 0: the same 37 levels), with the
    depth the launches are sized by asserted to need the 64-level instantiation -> (case, PathEngine)'''
    from ptina_amd.common import ctx
    c = case('deep')
    c.shares()
    eng = _setup(c, mode, None if mode == 'strict' else {'tree': 0}, scene)
    depth = ctx().get_option('tree_depth' if mode == 'strict' else 'fast_depth')
    assert depth + 2 > 32, f'deep {mode}: a tree of depth {depth} is served by the 32-level instantiation'
    return c, eng


def _deep_path_film(selection, count=0):
    from ptina_amd.common import ctx
    from ptina_amd.things import FilmTable
    mode, opts, _, _ = SELECTIONS[selection]
    c, eng = _deep(mode)
    for key, value in dict(opts, count=count).items():
        ctx().set_option(key, value)
    eng.render(FRAMES)
    raw = FilmTable().get_raw().copy()
    if mode != 'strict':
        assert ctx().get_option('last_kernel') == 0
    return c, raw


@pytest.mark.parametrize('count', [0, 1])
@pytest.mark.parametrize('selection', ['strict', 'gather_binary'])
def test_deep_path_engine(fresh, selection, count):
    '''the gather render kernel's table of (stack levels, counters) in both builds'''
    c, raw = _deep_path_film(selection, count)
    assert_mask(c, raw, FRAMES, f'deep {selection} count {count}')


@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_deep_brute_engine(fresh, mode):
    from ptina_amd.engine.brute import BruteEngine
    from ptina_amd.things import FilmTable
    c, _ = _deep(mode)
    BruteEngine().render(FRAMES)
    assert_mask(c, FilmTable().get_raw(), FRAMES, f'deep brute {mode}')


@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_deep_metropolis_path_door(fresh, mode):
    from ptina_amd.engine.mltpath import mlt_trace
    c = case('deep')
    hit, miss = c.shares()
    X, pi, pj = _door_points(c, hit, miss)
    _deep(mode)
    rgb = mlt_trace(X)
    want = np.where(hit[pi, pj][:, None], np.zeros(3, np.float32), np.array([1, 0.5, 0.25], np.float32)).astype(np.float32)
    bad = np.flatnonzero((rgb.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert hit[pi, pj].any() and miss[pi, pj].any()
    assert bad.size == 0, (f'deep mlt_trace {mode}: {bad.size} of {X.shape[0]} rays wrong; first: screen point {X[bad[0], :2].tolist()} of pixel '
                           f'({pi[bad[0]]}, {pj[bad[0]]}) gives {rgb[bad[0]].tolist()}, want {want[bad[0]].tolist()}')


@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_deep_metropolis_chains(fresh, mode):
    '''LSP = 1: every proposal is a fresh uniform vector, splatted where its first two draws point.  A splat into a full-hit pixel
    adds exactly 0 and one into a full-miss pixel exactly the world colour, whatever the chains accept'''
    from ptina_amd.engine.mltpath import MLTPathEngine
    from ptina_amd.things import FilmTable
    c, _ = _deep(mode)
    hit, miss = c.shares()
    FilmTable().clear()
    e = MLTPathEngine(nchains=4096, seed=7)
    e.LSP[None] = 1.0
    e.render(4)
    raw = FilmTable().get_raw().reshape(c.nx, c.ny, 4)
    assert raw[..., 3].sum() == 4096 * 4 and raw[hit][:, 3].sum() > 0 and raw[miss][:, 3].sum() > 0
    bad = np.argwhere(hit & (raw[..., :3] != 0).any(axis=-1))
    assert bad.shape[0] == 0, f'deep chains {mode}: {bad.shape[0]} full-hit pixels hold light; first {tuple(bad[0])}: {raw[tuple(bad[0])].tolist()}'
    r = raw[..., 0]
    bad = np.argwhere(miss & ((r != np.round(r)) | (raw[..., 1] != r / 2) | (raw[..., 2] != r / 4)))
    assert bad.shape[0] == 0, f'deep chains {mode}: {bad.shape[0]} full-miss pixels are not (r, r/2, r/4); first {tuple(bad[0])}: {raw[tuple(bad[0])].tolist()}'


@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_deep_list_pass(fresh, mode):
    '''every pixel listed: the list kernel renders the whole film; in the strict build it is the PathEngine's bit for bit'''
    from ptina_amd.common import reset_all
    from ptina_amd.things import FilmTable
    c, eng = _deep(mode)
    FilmTable().clear()
    FilmTable().set_selection(np.arange(c.nx * c.ny, dtype=np.int32))
    eng.render_selected(FRAMES)
    raw = FilmTable().get_raw().copy()
    assert_mask(c, raw, FRAMES, f'deep list pass {mode}')
    if mode == 'strict':
        reset_all()
        _, path = _deep_path_film('strict')
        diff = np.flatnonzero((raw.view(np.uint32) != path.view(np.uint32)).any(axis=1))
        assert diff.size == 0, (f'deep: the list pass differs from the strict PathEngine in {diff.size} pixels; first {divmod(int(diff[0]), c.ny)}: '
                                f'{raw[diff[0]].tolist()} against {path[diff[0]].tolist()}')


@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_deep_preview(fresh, mode):
    '''one material of basecolor 0.5 on every triangle: three preview frames sum to exactly 1.5 where every ray hits'''
    from ptina_amd import scenes
    from ptina_amd.engine.preview import PreviewEngine
    from ptina_amd.things import FilmTable
    c = case('deep')
    hit, miss = c.shares()
    v, m, _, im = c.scene
    _deep(mode, (v, m, [scenes.material(basecolor=(0.5, 0.5, 0.5))], im))
    for _ in range(3):
        PreviewEngine().render()
    raw = FilmTable().get_raw(1).reshape(c.nx, c.ny, 4)
    bad = np.argwhere(hit & (raw != np.array([1.5, 1.5, 1.5, 3], np.float32)).any(axis=-1))
    assert bad.shape[0] == 0, f'deep preview {mode}: {bad.shape[0]} full-hit pixels are not (1.5, 1.5, 1.5, 3); first {tuple(bad[0])}: {raw[tuple(bad[0])].tolist()}'
    bad = np.argwhere(miss & (raw != np.array([0, 0, 0, 3], np.float32)).any(axis=-1))
    assert bad.shape[0] == 0, f'deep preview {mode}: {bad.shape[0]} full-miss pixels are not (0, 0, 0, 3); first {tuple(bad[0])}: {raw[tuple(bad[0])].tolist()}'

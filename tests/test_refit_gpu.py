'''
BVHTree().refit() on the GPU (-m gpu): the trees of a build kept, their boxes and the triangle records fitted to a model whose
faces moved (csrc/refit.hip, csrc/tree_refit.cpp).

Two start models for a target model v: `jitter` -- every triangle translated by up to one edge length, seeded -- and
`shuffled` -- face f placed where face perm[f] is, so the built topology has nothing to do with the target: the boxes overlap
as badly as they can and the walks' stacks are exercised (wide_stack is a function of the ids alone, tree_checks S1, so it
still suffices).  Every test builds on the start model, loads the target (ModelPool().load, the same face count) and refits,
unless it says otherwise.

1  records: what comes back from the device equals tests/refit_ref.py byte for byte and passes every property of
   tests/tree_checks.py against the target; ids, hierarchy and the options the kernels size their stacks by are unchanged
2  round trip: start -> target -> start by refits gives the build's bytes, growth exactly 1.0 and the build's film bit for bit
3  visibility: every walk over a refitted tree, held to the exhaustive f64 search of tests/visibility_ref.py, no outliers
4  through the composition: set_world + compose + refit held to the oracle; no fetch of the model's host copy
5  state and refusals      6  refits between launches in flight
'''

import numpy as np
import pytest

import refit_ref
import tree_checks as tc
from test_refit_cpu import jitter, shuffled
from test_tree_invariants_gpu import BUILDERS, _positions, _random_model, _wide_records
from test_visibility_ref_cpu import WORLD, case, assert_mask, preview_errors
from test_visibility_gpu import SELECTIONS, FITS_LDS, FRAMES, _door_points

pytestmark = pytest.mark.gpu
F = np.float32
u32 = np.uint32


# ---------------------------------------------------------------- models and downloads
def _moved_model(v, m, kind, seed):
    '''the start model of kind `kind` for the target (v [3n][8], m [n]): positions moved, normals and texcoords kept'''
    v = np.array(v, F, copy=True).reshape(-1, 3, 8)
    if kind == 'jitter':
        v[:, :, :3] = jitter(v[:, :, :3], seed)
        return v.reshape(-1, 8), np.array(m, np.int32)
    perm = np.random.default_rng(seed).permutation(v.shape[0])
    assert np.array_equal(v[perm][:, :, :3], shuffled(v[:, :, :3], seed))
    return np.ascontiguousarray(v[perm]).reshape(-1, 8), np.array(m, np.int32)[perm]


def _ctx():
    from ptina_amd.common import ctx
    return ctx()


def _things():
    from ptina_amd.things import init_things
    init_things()
    return _ctx()


def _load(v, m):
    from ptina_amd.things import ModelPool
    ModelPool().load(v, m)


def _tree():
    from ptina_amd.things import BVHTree
    return BVHTree()


def _records(c):
    '''everything of the built trees that can be downloaded'''
    t = _tree().to_numpy()
    w, q = _wide_records(c)
    return dict(t, wnode=w, qnode=q, opts=tuple(c.get_option(k) for k in ('wide_nodes', 'wide_depth', 'wide_stack', 'tree_depth', 'fast_depth')))


def _same_records(a, b, what, keys=('child', 'leaf', 'mc', 'bmin', 'bmax', 'wnode', 'qnode')):
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(u32), y.view(u32)), f'{what}: {k} differs in {int((x.view(u32) != y.view(u32)).sum())} words'
    assert a['depth'] == b['depth'] and a['opts'] == b['opts'], f'{what}: depth / options {a["depth"]} {a["opts"]} != {b["depth"]} {b["opts"]}'


def _set_builder(c, tree, sah, wide):
    for key, value in (('tree', tree), ('sah_build', sah), ('wide_build', wide)):
        if value is not None:
            c.set_option(key, value)


def _refit_and_check(c, built, target_v, target_m, n, what, device_sah):
    '''load the target, refit, and hold what comes back to refit_ref and to the checker'''
    _load(target_v, target_m)
    growth = _tree().refit()
    assert np.isfinite(growth) and growth > 0, f'{what}: growth {growth}'
    got = _records(c)
    pos = _positions(target_v)
    bmin, bmax, w, q = refit_ref.refit_ref(built['child'], built['leaf'], built['wnode'], built['qnode'], n, pos)
    want = dict(built, bmin=bmin, bmax=bmax, wnode=w, qnode=q)
    _same_records(got, want, what)
    try:
        tc.check_lbvh(pos, got, n)
        t = tc.check_all(pos, got['leaf'], got['wnode'], got['qnode'], n)
    except AssertionError as e:
        raise AssertionError(f'{what}: {e}') from None
    assert np.array_equal(t.ids, tc.Tree(pos, built['leaf'], built['wnode'], built['qnode'], n).ids), f'{what}: an id row changed'
    if device_sah:
        assert c.get_option('sah_fallback') == 0, f'{what}: the device SAH pass fell back to the host pass'
    info = _tree().refit_stats()
    assert (info.faces, info.wide_nodes, info.host_fetches) == (n, t.nw, 0) and info.refits >= 1
    return growth


# ---------------------------------------------------------------- 1: records
@pytest.mark.parametrize('kind', ['jitter', 'shuffled'])
@pytest.mark.parametrize('n', [2, 3, 5, 33, 65, 300, 1025, 2049])
def test_records_over_every_builder(fresh, n, kind):
    '''2 to 5 triangles: nodes with unused slots, a root that is all leaves; 65, 300: more than one workgroup of nodes; 1025, 2049:
    the device SAH pass's binned levels wrote the binary records.  tree = 0: fnode is the LBVH itself, fitted by the same kernel'''
    v, m = _random_model(n)
    sv, sm = _moved_model(v, m, kind, n)
    c = _things()
    for tree, sah, wide in BUILDERS:
        what = f'n {n} {kind} tree {tree} sah_build {sah} wide_build {wide}'
        _load(sv, sm)
        _set_builder(c, tree, sah, wide)
        _tree().build()
        built = _records(c)
        _refit_and_check(c, built, v, m, n, what, sah == 1)


@pytest.mark.parametrize('kind', ['jitter', 'shuffled'])
def test_records_at_20000_triangles(fresh, kind):
    n = 20000
    v, m = _random_model(n)
    sv, sm = _moved_model(v, m, kind, n)
    c = _things()
    _load(sv, sm)
    _tree().build()
    g = _refit_and_check(c, _records(c), v, m, n, f'n {n} {kind} defaults', True)
    print(f'n {n} {kind}: growth {g:.3f}')


@pytest.mark.parametrize('kind', ['identical', 'on_a_line', 'huge', 'two_clusters'])
def test_records_of_degenerate_targets(fresh, kind):
    '''the models of test_tree_invariants_gpu.test_degenerate_models as TARGETS of a refit from the unit-size random model they
    are made of: `huge` multiplies every coordinate by 1e18, `identical` puts every triangle in one place'''
    n = 3000
    from ptina_amd import scenes
    sv, m, _, _ = scenes.scene_random_tris(n, seed=7, edge=0.05)
    v = np.array(sv, F, copy=True).reshape(n, 3, 8)
    if kind == 'identical':
        v[:] = v[0]
    elif kind == 'on_a_line':
        v[:, :, 1:3] = v[0, :, 1:3]
        v[:, :, 0] = v[0, :, 0] + np.arange(n, dtype=F)[:, None] * 1e-3
    elif kind == 'huge':
        v[:, :, :3] *= F(1e18)
    else:
        v[:] = v[0]
        v[n // 3:, :, :3] += F(5.0)
    v = v.reshape(n * 3, 8)
    c = _things()
    for wide in (1, 0):
        _load(sv, m)
        _set_builder(c, 1, 1, wide)
        _tree().build()
        _refit_and_check(c, _records(c), v, m, n, f'{kind} sah_build 1 wide_build {wide}', True)


# ---------------------------------------------------------------- 2: round trip
ROUND_TRIP = {'strict': ('strict', {}), 'default': ('fast', {}), 'gather_binary': ('fast', {'lds': 0, 'wide': 0})}


def _engine(mode, opts, nx=32, ny=32, scene_name='s978'):
    '''a context with film, materials, camera and engine; the model is the test's'''
    from ptina_amd import scenes, _lib
    from ptina_amd.things import init_things, FilmTable, MaterialPool, ImagePool, Camera
    from ptina_amd.engine.path import PathEngine
    init_things()
    eng = PathEngine()
    c = _ctx()
    c.set_option('mode', _lib.MODE_STRICT if mode == 'strict' else _lib.MODE_FAST)
    for k, val in opts.items():
        c.set_option(k, val)
    FilmTable().set_size(nx, ny)
    v, m, mats, imgs = scenes.get_scene(scene_name)
    MaterialPool().load(mats)
    ImagePool().load(imgs)
    Camera().set_perspective(scenes.BENCH_CAMERA)
    return eng, np.asarray(v, F), np.asarray(m, np.int32)


def _film(eng, spp=4):
    '''the raw film of spp frames from the sampler's start'''
    from ptina_amd.things import FilmTable
    from ptina_amd.sampling.sobol import SobolSampler
    SobolSampler().reset()
    FilmTable().clear()
    eng.render(spp)
    raw = FilmTable().get_raw().copy()
    assert np.all(raw.reshape(-1, 4)[:, 3] == spp)
    return raw


def _same_film(a, b, what):
    diff = np.flatnonzero((a.view(u32) != b.view(u32)).reshape(-1, 4).any(axis=1))
    assert diff.size == 0, f'{what}: {diff.size} pixels differ; first {int(diff[0])}: {a.reshape(-1, 4)[diff[0]].tolist()} against {b.reshape(-1, 4)[diff[0]].tolist()}'


@pytest.mark.parametrize('selection', list(ROUND_TRIP))
def test_round_trip_gives_the_builds_bytes_and_film(fresh, selection):
    '''s978 (32 x 32 x 4): built, refitted to the jittered scene, refitted back.  gather_binary walks fnode: its round trip shows
    here in the film and in the cost, which is the same integer again, and word for word in tests/test_records_gpu.py'''
    mode, opts = ROUND_TRIP[selection]
    eng, v, m = _engine(mode, opts)
    tv, tm = _moved_model(v, m, 'jitter', 978)
    c = _ctx()
    _load(v, m)
    _tree().build()
    built = _records(c)
    film = _film(eng)
    assert np.count_nonzero(film.reshape(-1, 4)[:, :3].sum(axis=1)) > 32 * 32 // 8, 'the film shows nothing'
    _load(tv, tm)
    g1 = _tree().refit()
    moved_film = _film(eng)
    assert (moved_film.view(u32) != film.view(u32)).any(), 'the moved scene renders the same film'
    _load(v, m)
    g2 = _tree().refit()
    assert g1 != 1.0 and g2 == 1.0, f'growth {g1} there, {g2} back'
    info = _tree().refit_stats()
    assert info.refits == 2 and info.cost_built == info.cost_now > 0 and info.host_fetches == 0
    _same_records(_records(c), built, f'{selection}: there and back')
    _same_film(_film(eng), film, f'{selection}: there and back')
    _tree().build()
    _same_records(_records(c), built, f'{selection}: built again after the refits')
    assert _tree().refit_stats().refits == 0
    _same_film(_film(eng), film, f'{selection}: built again after the refits')


# ---------------------------------------------------------------- 3: visibility, no outliers
TARGETS = ['n3', 'n33', 'n300', 'n1025', 'n5000', 'moved', 'flat']


def _refitted(c, mode, tree=None, selection='default'):
    '''the case's context with the tree built on a start model and refitted to the case's scene.  The start is the shuffled one,
    except for the strict build: its walk restates the reference's give-up after n node visits (lbvh.py:324,
    pt_device.h bvh_closest `ntimes < n`), which a tree whose boxes all overlap can exhaust by design -- there the start is jitter'''
    from test_visibility_gpu import _setup
    v, m, mats, imgs = c.scene
    sv, sm = _moved_model(v, m, 'jitter' if mode == 'strict' else 'shuffled', c.n)
    eng = _setup(c, mode, tree, scene=(sv, sm, mats, imgs))
    before = tuple(_ctx().get_option(k) for k in ('wide_nodes', 'wide_depth', 'wide_stack'))
    _load(v, m)
    _tree().refit()
    assert before == tuple(_ctx().get_option(k) for k in ('wide_nodes', 'wide_depth', 'wide_stack'))
    return eng


def _selections():
    out = [(name, sel, None) for name in TARGETS for sel in SELECTIONS if sel != 'lds_binary' or name in FITS_LDS]
    return out + [(name, 'default', 'device_sah') for name in TARGETS] + [(name, 'gather_binary', 'device_sah') for name in TARGETS]


@pytest.mark.parametrize('name,selection,tree', _selections())
def test_visibility_path_engine(fresh, name, selection, tree):
    from ptina_amd.things import FilmTable
    c = case(name)
    c.shares()
    mode, opts, fit, nofit = SELECTIONS[selection]
    eng = _refitted(c, mode, {'sah_build': 1} if tree else None)
    for key, value in opts.items():
        _ctx().set_option(key, value)
    eng.render(FRAMES)
    raw = FilmTable().get_raw().copy()
    if mode != 'strict':
        want = fit if name in FITS_LDS else nofit
        assert _ctx().get_option('last_kernel') == want, f'{name} {selection}: last_kernel {_ctx().get_option("last_kernel")}, expected {want}'
    assert_mask(c, raw, FRAMES, f'refitted {name} {selection} {tree}')


@pytest.mark.parametrize('mode', ['strict', 'fast'])
@pytest.mark.parametrize('name', ['n300', 'n1025', 'n5000'])
def test_visibility_brute_engine(fresh, name, mode):
    from ptina_amd.engine.brute import BruteEngine
    from ptina_amd.things import FilmTable
    c = case(name)
    c.shares()
    _refitted(c, mode)
    BruteEngine().render(FRAMES)
    assert_mask(c, FilmTable().get_raw(), FRAMES, f'refitted brute {mode} {name}')


@pytest.mark.parametrize('mode', ['strict', 'fast'])
@pytest.mark.parametrize('name', ['n1025', 'n5000'])
def test_visibility_metropolis_path_door(fresh, name, mode):
    from ptina_amd.engine.mltpath import mlt_trace
    c = case(name)
    hit, miss = c.shares()
    X, pi, pj = _door_points(c, hit, miss)
    _refitted(c, mode)
    rgb = mlt_trace(X)
    want = np.where(hit[pi, pj][:, None], np.zeros(3, F), np.array([1, 0.5, 0.25], F)).astype(F)
    bad = np.flatnonzero((rgb.view(u32) != want.view(u32)).any(axis=1))
    assert bad.size == 0, f'refitted mlt_trace {mode} {name}: {bad.size} of {X.shape[0]} rays wrong; first: pixel ({pi[bad[0]]}, {pj[bad[0]]}) gives {rgb[bad[0]].tolist()}'


@pytest.mark.parametrize('mode', ['strict', 'fast'])
@pytest.mark.parametrize('name', ['n300', 'n1025', 'n5000'])
def test_visibility_preview(fresh, name, mode):
    '''the nearest triangle's material, exactly: the refit carries the material ids with the faces (tshade)'''
    from ptina_amd.engine.preview import PreviewEngine
    from ptina_amd.things import FilmTable
    c = case(name, preview=True)
    c.shares()
    c.materials()
    _refitted(c, mode)
    for _ in range(3):
        PreviewEngine().render()
    bad = preview_errors(c, FilmTable().get_raw(1), 3, f'refitted preview {mode} {name}')
    assert not bad, f'{len(bad)} wrong pixels; ' + '; '.join(bad[:4])


# ---------------------------------------------------------------- 4: through the composition
def _placed(center, yaw_deg):
    th = np.radians(yaw_deg)
    return np.array([[np.cos(th), 0, np.sin(th), center[0]], [0, 1, 0, center[1]], [-np.sin(th), 0, np.cos(th), center[2]], [0, 0, 0, 1.0]])


def _s34_objects():
    '''the s34 scene as objects, as exams/animate_amd.py makes it -> (pool, the tall box's object id)'''
    from ptina_amd import scenes
    from ptina_amd.things import ModelPool
    wp, wn, wt, wm = scenes.cornell_walls()
    pool = ModelPool()
    for mtl in (0, 1, 2):
        pick = wm == mtl
        pool.add_object(pool.add_mesh(wp[pick], wn[pick], wt[pick]), np.eye(4), mtl)
    tall = pool.add_object(pool.add_mesh(*scenes.box((0, 0, 0), (0.6, 1.2, 0.6), 0.0, 3)[:3]), _placed((-0.7, 1.2, -0.6), 18.0), 3)
    pool.add_object(pool.add_mesh(*scenes.box((0, 0, 0), (0.6, 0.6, 0.6), 0.0, 4)[:3]), _placed((0.75, 0.6, 0.55), -17.0), 4)
    pool.compose()
    return pool, tall


# (the film sizes and sample counts at which tests/test_parity_gpu.py holds the s34 scene to the oracle in each build)
@pytest.mark.parametrize('mode,nx,ny,spp', [('strict', 64, 64, 8), ('fast', 96, 96, 32)])
def test_compose_then_refit_is_held_to_the_oracle(fresh, oracle_mod, mode, nx, ny, spp):
    from helpers import setup_oracle, assert_parity, bounds
    from ptina_amd import scenes
    from ptina_amd.things import FilmTable
    eng, _, _ = _engine(mode, {}, nx, ny, 's34')
    pool, tall = _s34_objects()
    _tree().build()
    fetched = pool.compose_stats().host_fetches            # (34 faces: the build's host SAH pass reads the model)
    pool.set_world(tall, _placed((-0.7, 1.2, -0.6), 63.0))
    pool.compose()
    assert pool.compose_stats().recomposed == 12
    _tree().refit()
    assert pool.compose_stats().host_fetches == fetched and _tree().refit_stats().host_fetches == 0
    eng.render()
    FilmTable().get_image()
    FilmTable().clear()
    for _ in range(spp):
        eng.render()
    img = FilmTable().get_image()
    assert pool.compose_stats().host_fetches == fetched
    v, m = pool.to_numpy()                                 # (fetches the model: after the counts above)
    _, _, mats, imgs = scenes.scene_s34()
    ref = setup_oracle(oracle_mod, (v, m, mats, imgs), nx, ny)
    ref.render(1)
    ref.clear()
    ref.render(spp)
    assert_parity(img, ref.get_image(), *bounds(mode), what=f'compose + refit {mode} {nx}x{ny}x{spp}')


def test_set_material_then_refit_repaints_that_object_alone(fresh):
    from ptina_amd.engine.preview import PreviewEngine
    from ptina_amd.things import FilmTable
    _engine('fast', {}, 64, 64, 's34')
    pool, tall = _s34_objects()
    _tree().build()

    def albedo():
        from ptina_amd.sampling.sobol import SobolSampler
        SobolSampler().reset()
        FilmTable().clear(1)
        PreviewEngine().render()
        return FilmTable().get_raw(1).copy().reshape(-1, 4)
    before = albedo()
    pool.set_material(tall, 4)
    pool.compose()
    assert _tree().refit() == 1.0                          # no face moved
    after = albedo()
    changed = (before.view(u32) != after.view(u32)).any(axis=1)
    pool.set_material(tall, 3)
    pool.compose()
    _tree().refit()
    assert np.array_equal(albedo().view(u32), before.view(u32))
    # the pixels that changed are those whose nearest face is the tall box's: found by hiding the box's albedo another way
    pool.set_material(tall, 0)
    pool.compose()
    _tree().refit()
    other = (before.view(u32) != albedo().view(u32)).any(axis=1)
    assert changed.any() and np.array_equal(changed, other), f'{int(changed.sum())} pixels changed, {int(other.sum())} show the tall box'
    assert pool.compose_stats().host_fetches <= 1 and _tree().refit_stats().host_fetches == 0


# ---------------------------------------------------------------- 5: state and refusals
def test_refusals_name_build_tree(fresh):
    c = _things()
    v, m = _random_model(33)
    _load(v, m)
    with pytest.raises(RuntimeError, match=r'no tree was ever built.*build_tree\(\)'):
        _tree().refit()
    assert not _tree().can_refit() and _tree().refit_stats().faces == -1
    _tree().build()
    assert _tree().can_refit()
    v2, m2 = _random_model(34)
    _load(v2, m2)
    with pytest.raises(RuntimeError, match=r'34 faces, the tree was built for 33.*build_tree\(\)'):
        _tree().refit()
    _load(v, m)
    assert _tree().refit() == 1.0
    c.set_option('tree', 0)
    with pytest.raises(RuntimeError, match=r'option.*build_tree\(\)'):
        _tree().refit()
    c.set_option('tree', 1)                                # set back: the topology is still not trusted
    assert not _tree().can_refit()
    c.set_option('gpu_build', 0)
    _tree().build()
    with pytest.raises(RuntimeError, match=r'gpu_build = 0.*build_tree\(\)'):
        _tree().refit()
    c.set_option('gpu_build', 1)
    _tree().build()
    c.set_option('lds', 0)                                 # an option that steers no build
    assert _tree().refit() == 1.0


@pytest.mark.parametrize('n', [0, 1])
def test_no_nodes(fresh, n):
    from ptina_amd import scenes
    _things()
    v, m, _, _ = scenes.scene_random_tris(2, seed=2, edge=0.05)
    _load(v[:3 * n], m[:n])
    _tree().build()
    _load(v[3:3 + 3 * n], m[:n])
    assert _tree().refit() == 1.0
    info = _tree().refit_stats()
    assert (info.faces, info.wide_nodes, info.refits, info.cost_now) == (n, 0, 1, 0.0)


def test_update_builds_or_refits(fresh):
    n = 300
    c = _things()
    v, m = _random_model(n)
    sv, sm = _moved_model(v, m, 'shuffled', n)
    near = np.array(v, F, copy=True)
    near[0:3, 0:3] += F(1e-3)                              # one triangle, a fiftieth of its edge
    _load(v, m)
    assert _tree().update() == 'build'
    fresh_build = _records(c)
    _load(near, m)
    assert _tree().update() == 'refit' and _tree().refit_stats().refits == 1
    _load(sv, sm)
    assert _tree().update() == 'build'                     # (every face somewhere else: the default bound says build)
    assert _tree().refit_stats().refits == 0
    _load(v, m)
    assert _tree().update(max_growth=float('inf')) == 'refit'
    assert _tree().refit_stats().growth > 1.0
    _load(sv, sm)
    _tree().build()
    _load(v, m)
    assert _tree().update(max_growth=1.0) == 'build'
    _same_records(_records(c), fresh_build, 'update(max_growth=1.0) on the shuffled start')
    _load(v[:3 * 299], m[:299])
    assert _tree().update() == 'build'                     # another face count: no refit is allowed


# ---------------------------------------------------------------- 6: in flight
def test_refits_between_launches_in_flight(fresh):
    '''twenty rounds of render(4) with no read-back, then the other of two models and a refit: the refit orders itself behind
    the launch that still reads the records, and every round's film is that model's film of round one'''
    eng, v, m = _engine('fast', {})
    models = [(v, m), _moved_model(v, m, 'jitter', 5)]
    _load(*models[0])
    _tree().build()
    first = [None, None]
    first[0] = _film(eng)
    for r in range(1, 21):
        eng.render(4)                                      # enqueued: the load below launches it, nothing waits for it
        k = r & 1
        _load(*models[k])
        _tree().refit()
        film = _film(eng)
        if first[k] is None:
            first[k] = film
            assert (first[0].view(u32) != first[1].view(u32)).any()
        else:
            _same_film(film, first[k], f'round {r}, model {k}')
    assert _tree().refit_stats().refits == 20 and _tree().refit_stats().host_fetches == 0

'''
Batch ray queries on the built tree (BVHTree.intersect / occluded / pick; csrc/query_kernel.hip) held to an exhaustive float64
search, ray by ray (-m gpu).  tests/query_ref.py says which rays it can decide without a tree; on those, hit, index and object
are exact in both builds, with no share of outliers.  depth, u and v are held to the f64 values within a tolerance that is
measured, not chosen: 4 x the largest deviation of the oracle's own f32 LinearBVH.intersect over the same decided rays of the
same scene (tests/test_query_cpu.py prints the figures; DESIGN.md section 3.15 records them).

1  closest hit: every tree shape (no inner node, one, SAH by the host and by the device, the 64-level instantiation), models far
   from the origin, 1024 times the size, flat       2  occlusion       3  avoid       4  launch edges: sizes about a workgroup,
   no rays, several chunks, single outputs, a broadcast origin       5  rays that are none       6  no side effects on a render
7  composed, edited and refitted scenes: object, the stale-tree error, pick       8  pick against the nearest material
'''

import numpy as np
import pytest

import query_ref as qr
import visibility_ref as vr
from test_query_cpu import reference
from test_visibility_ref_cpu import WORLD, case
from test_visibility_gpu import SAH_PASSES, _setup, _deep

pytestmark = pytest.mark.gpu
MODES = ['strict', 'fast']
INF = np.float32(1e6)          # the reference's inf (common.py:33): the depth of a miss

_tols = {}


def tolerance(oracle_mod, name):
    '''(depth, uv) a kernel may be off the f64 values on the decided hits of a case: 4 x what the oracle's f32 intersect is'''
    if name not in _tols:
        from helpers import setup_oracle
        c = case(name)
        o, d, ref = reference(name)
        orc = setup_oracle(oracle_mod, c.scene, c.nx, c.ny, camera=c.camera, lights=[], world=WORLD)
        got = qr.oracle_answers(orc, o, d)
        assert not qr.errors(ref, got, f'oracle {name}')
        dev_depth, dev_uv = qr.deviation(ref, got)
        print(f'{name}: oracle deviation depth {dev_depth:.3g}, uv {dev_uv:.3g}; the kernels get 4 x')
        assert dev_depth > 0 and dev_uv > 0
        _tols[name] = (4 * dev_depth, 4 * dev_uv)
    return _tols[name]


def tree():
    from ptina_amd.things import BVHTree
    return BVHTree()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8 if a.dtype == bool else np.uint32)


def same(a, b, what):
    '''two answers of intersect(), bit for bit'''
    for key in ('hit', 'depth', 'index', 'u', 'v', 'object'):
        diff = np.flatnonzero(bits(a[key]) != bits(b[key]))
        assert diff.size == 0, f'{what}: {key} differs in {diff.size} rays; first {int(diff[0])}: {a[key][diff[0]]!r} against {b[key][diff[0]]!r}'


def check(ref, got, what, **kw):
    bad = qr.errors(ref, got, what, **kw)
    assert not bad, f'{len(bad)}+ wrong rays; ' + '; '.join(bad[:4])
    miss = ~np.asarray(got['hit'])
    assert np.all(got['index'][miss] == -1) and np.all(got['depth'][miss] == INF) and np.all(got['u'][miss] == 0) and np.all(got['v'][miss] == 0), what


# ---------------------------------------------------------------- 1. closest
CLOSEST = ([(name, None) for name in ('n2', 'n3', 'n33', 'n300')] + [('n1025', sah) for sah in SAH_PASSES] +
           [(name, None) for name in ('n5000', 'moved', 'x1024', 'flat')])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name,sah', CLOSEST)
def test_closest_hit_on_every_decided_ray(fresh, oracle_mod, name, sah, mode):
    c = case(name)
    o, d, ref = reference(name)
    qr.caps(name, ref)
    tol_depth, tol_uv = tolerance(oracle_mod, name)
    _setup(c, mode, SAH_PASSES[sah] if sah else None)
    got = tree().intersect(o, d)
    assert got['hit'].dtype == bool and got['depth'].dtype == np.float32 and got['index'].dtype == np.int32 and got['hit'].shape == (qr.RAYS,)
    print(f'{name} {mode}: deviation depth, uv {qr.deviation(ref, got)} of {(tol_depth, tol_uv)} allowed')
    check(ref, got, f'closest {mode} {name} {sah}', tol_depth=tol_depth, tol_uv=tol_uv)
    assert np.all(got['object'] == -1)


@pytest.mark.parametrize('mode', MODES)
def test_closest_hit_through_the_64_level_instantiation(fresh, oracle_mod, mode):
    o, d, ref = reference('deep')
    qr.caps('deep', ref)
    tol_depth, tol_uv = tolerance(oracle_mod, 'deep')
    _deep(mode)                                              # (asserts tree_depth / fast_depth + 2 > 32)
    got = tree().intersect(o, d)
    print(f'deep {mode}: deviation depth, uv {qr.deviation(ref, got)} of {(tol_depth, tol_uv)} allowed')
    check(ref, got, f'closest {mode} deep', tol_depth=tol_depth, tol_uv=tol_uv)
    assert np.all(got['object'] == -1)


# ---------------------------------------------------------------- 2. occlusion
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['n300', 'n1025', 'deep'])
def test_occlusion(fresh, name, mode):
    o, d, ref = reference(name)
    qr.caps(name, ref)
    if name == 'deep':
        _deep(mode)
    else:
        _setup(case(name), mode)
    hits, misses = ref['decided'] & ref['hit'], ref['decided'] & ~ref['hit']
    tn = np.where(hits, ref['t'], 1.0)
    short = tree().occluded(o, d, (0.5 * tn).astype(np.float32))
    far = tree().occluded(o, d, (2.0 * tn).astype(np.float32))
    any_ = tree().occluded(o, d)
    assert short.dtype == bool and short.shape == (qr.RAYS,)
    for got, want, what in ((short, False, 'dis = tn / 2'), (far, True, 'dis = 2 tn'), (any_, True, 'dis = inf')):
        bad = np.flatnonzero(hits & (got != want))
        assert bad.size == 0, f'occluded {mode} {name}, {what}: {bad.size} decided hits are not {want}; first ray {int(bad[0])}, t {ref["t"][bad[0]]}'
    bad = np.flatnonzero(misses & any_)
    assert bad.size == 0, f'occluded {mode} {name}: {bad.size} decided misses are occluded; first ray {int(bad[0])}'
    same_inf = tree().occluded(o, d, np.inf, avoid=-1)
    assert np.array_equal(any_, same_inf)


# ---------------------------------------------------------------- 3. avoid
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['n300', 'n1025'])
def test_avoid_is_the_model_without_that_face(fresh, name, mode):
    c = case(name)
    o, d, ref = reference(name)
    sel = np.flatnonzero(ref['decided'] & ref['hit'])
    avoid = ref['index'][sel].astype(np.int32)
    without = qr.classify(c.pos, o[sel], d[sel], avoid=avoid)
    assert float(without['decided'].mean()) >= 0.5
    _setup(c, mode)
    got = tree().intersect(o[sel], d[sel], avoid=avoid)
    check(without, got, f'avoid {mode} {name}')
    assert (got['hit'] & without['decided']).any() and (~got['hit'] & without['decided']).any()
    occ = tree().occluded(o[sel], d[sel], avoid=avoid)
    bad = np.flatnonzero(without['decided'] & (occ != without['hit']))
    assert bad.size == 0, f'occluded with avoid {mode} {name}: {bad.size} rays wrong'
    plain = tree().intersect(o, d)
    same(plain, tree().intersect(o, d, avoid=-1), f'avoid = -1 {mode} {name}')
    same(plain, tree().intersect(o, d, avoid=np.full(qr.RAYS, -1, np.int32)), f'avoid = [-1] {mode} {name}')


# ---------------------------------------------------------------- 4. launch edges
def _closest_raw(n, o, d, only=None, chunk=0):
    '''mpt_query_closest itself; only: the one output that is asked for (the others NULL)'''
    from ptina_amd.common import ctx
    from ptina_amd._lib import fptr, iptr
    kinds = dict(hit=np.int32, depth=np.float32, index=np.int32, u=np.float32, v=np.float32, object=np.int32)
    out = {k: np.full(n, 77, t) for k, t in kinds.items() if only in (None, k)}
    ptr = lambda k: None if k not in out else (iptr(out[k]) if kinds[k] == np.int32 else fptr(out[k]))   # noqa: E731
    ctx().call('mpt_query_closest', n, fptr(o), fptr(d), None, ptr('hit'), ptr('depth'), ptr('index'), ptr('u'), ptr('v'), ptr('object'), chunk)
    return out


@pytest.mark.parametrize('mode', MODES)
def test_launch_edges(fresh, mode):
    c = case('n300')
    o, d, ref = reference('n300')
    _setup(c, mode)
    full = tree().intersect(o, d)
    check(ref, full, f'edges {mode}')
    for n in (1, 255, 256, 257):
        part = tree().intersect(o[:n], d[:n])
        assert part['hit'].shape == (n,)
        same(part, {k: a[:n] for k, a in full.items()}, f'{mode}: the first {n} rays alone')
    empty = tree().intersect(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert all(a.shape == (0,) for a in empty.values()) and empty['hit'].dtype == bool
    assert tree().occluded(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)).shape == (0,)
    for chunk in (512, 768, 100):
        same(tree().intersect(o, d, chunk=chunk), full, f'{mode}: chunks of {chunk}')
        assert np.array_equal(tree().occluded(o, d, chunk=chunk), tree().occluded(o, d))
    raw = _closest_raw(qr.RAYS, o, d)
    for key in raw:
        one = _closest_raw(qr.RAYS, o, d, only=key, chunk=768)
        assert list(one) == [key] and np.array_equal(bits(one[key]), bits(raw[key])), f'{mode}: {key} asked for alone'
        assert np.array_equal(raw[key] != 0, full[key]) if key == 'hit' else np.array_equal(bits(raw[key]), bits(full[key])), f'{mode}: {key} through the C call'
    # one origin, many directions
    aimed = (c.pos.mean(axis=1) - o[0].astype(np.float64)).astype(np.float32)
    same(tree().intersect(o[0], aimed), tree().intersect(np.tile(o[0], (aimed.shape[0], 1)), aimed), f'{mode}: a broadcast origin')
    assert tree().intersect(o[0], aimed)['hit'].any()
    from ptina_amd.common import ctx
    ms, launches = ctx().timer('mpt_query_kernel_time')
    assert launches > 0 and ms > 0
    assert ctx().timer('mpt_query_kernel_time') == (0.0, 0)


# ---------------------------------------------------------------- 5. rays that are none
@pytest.mark.parametrize('mode', MODES)
def test_bad_rays_are_misses_and_leave_the_others_alone(fresh, mode):
    c = case('n300')
    o, d, ref = reference('n300')
    _setup(c, mode)
    clean = tree().intersect(o, d)
    clean_occ = tree().occluded(o, d)
    rng = np.random.default_rng(5)
    at = rng.permutation(qr.RAYS)[:96]
    ob, db = o.copy(), d.copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for k, r in enumerate(at):
        axis = k % 3
        kind = (k // 3) % 6
        if kind == 0:
            db[r] = 0.0
        elif kind == 1:
            db[r] = (-0.0, 0.0, -0.0)
        elif kind == 2:
            ob[r, axis] = nan
        elif kind == 3:
            ob[r, axis] = inf if k % 2 else -inf
        elif kind == 4:
            db[r, axis] = nan
        else:
            db[r, axis] = inf
    got = tree().intersect(ob, db)
    occ = tree().occluded(ob, db)
    assert not got['hit'][at].any() and np.all(got['index'][at] == -1) and np.all(got['depth'][at] == INF) and np.all(got['object'][at] == -1)
    assert np.all(got['u'][at] == 0) and np.all(got['v'][at] == 0) and not occ[at].any()
    keep = np.ones(qr.RAYS, bool)
    keep[at] = False
    same({k: a[keep] for k, a in got.items()}, {k: a[keep] for k, a in clean.items()}, f'{mode}: the rays beside the bad ones')
    assert np.array_equal(occ[keep], clean_occ[keep])
    assert clean['hit'][at].any()                            # (some of the replaced rays were hits)


# ---------------------------------------------------------------- 6. no side effects
@pytest.mark.parametrize('mode', MODES)
def test_a_query_changes_nothing_a_render_reads_or_writes(fresh, mode):
    from helpers import setup_engine
    from ptina_amd import scenes
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import FilmTable
    from ptina_amd.sampling.sobol import SobolSampler
    scene = scenes.scene_s34()
    pos = vr.positions(scene[0])
    o, d = qr.rays(pos, 34, 512)
    ref = qr.classify(pos, o, d)
    assert (ref['decided'] & ref['hit']).any()

    def run(query, read_between):
        reset_all()
        eng = setup_engine(scene, 24, 24, mode=mode)
        ctx().set_option('count', 1)
        eng.render(4)
        if read_between:
            FilmTable().get_raw()                            # (the first launch has run: the query meets a settled context)
        answers = tree().intersect(o, d) if query else None  # (else: it meets the four frames still deferred, and flushes them)
        if query:
            tree().occluded(o, d)
        eng.render(4)
        raw = FilmTable().get_raw().copy()
        return raw, SobolSampler().state(), ctx().counters(), ctx().get_option('last_kernel'), answers

    for read_between in (True, False):
        raw0, sobol0, cnt0, k0, _ = run(False, read_between)
        raw1, sobol1, cnt1, k1, answers = run(True, read_between)
        what = f'{mode}, query {"after a read-back" if read_between else "on deferred frames"}'
        diff = np.flatnonzero((bits(raw0) != bits(raw1)).reshape(-1, 4).any(axis=1))
        assert diff.size == 0, f'{what}: {diff.size} film elements differ; first {int(diff[0])}: {raw0.reshape(-1, 4)[diff[0]]} against {raw1.reshape(-1, 4)[diff[0]]}'
        assert raw1.reshape(-1, 4)[:, 3].min() == 8
        assert sobol0[0] == sobol1[0] and np.array_equal(sobol0[1], sobol1[1]) and np.array_equal(bits(sobol0[2]), bits(sobol1[2])), what
        assert cnt0 == cnt1 and cnt0['samples'] > 0, (what, cnt0, cnt1)
        assert k0 == k1, what
        check(ref, answers, what)


# ---------------------------------------------------------------- 7. composed, edited, refitted scenes
def _placed(center, yaw_deg):
    th = np.radians(yaw_deg)
    return np.array([[np.cos(th), 0, np.sin(th), center[0]], [0, 1, 0, center[1]], [-np.sin(th), 0, np.cos(th), center[2]], [0, 0, 0, 1.0]])


def _objects():
    '''four objects of 80 faces each over two meshes, as exams/animate_amd.py makes objects -> (pool, object ids, first faces)'''
    from ptina_amd import scenes
    from ptina_amd.things import ModelPool
    pool = ModelPool()
    meshes = []
    for seed in (1, 2):
        v = np.asarray(scenes.scene_random_tris(80, seed=seed, edge=0.25)[0], np.float64).reshape(80, 3, 8)
        meshes.append(pool.add_mesh(v[:, :, 0:3] - [0.0, 2.0, 0.0], v[:, :, 3:6]))
    objs = [pool.add_object(meshes[0], _placed((0.0, 2.0, 0.0), 0.0), 0), pool.add_object(meshes[1], _placed((0.2, 2.1, 0.0), 30.0), 1),
            pool.add_object(meshes[0], _placed((-0.3, 1.9, 0.3), 120.0), 2), pool.add_object(meshes[1], _placed((0.0, 2.0, -0.4), 200.0), 0)]
    pool.compose()
    return pool, objs, np.arange(4) * 80


def _camera_ray(camera, x, y):
    inv = np.linalg.inv(np.asarray(camera, np.float64))
    a, b = inv @ [x, y, -1.0, 1.0], inv @ [x, y, 1.0, 1.0]
    o = a[:3] / a[3]
    return o.astype(np.float32), (b[:3] / b[3] - o).astype(np.float32)


@pytest.mark.parametrize('mode', MODES)
def test_composed_edited_and_refitted_scenes(fresh, mode):
    from ptina_amd import scenes
    c = case('n300')
    _setup(c, mode)
    pool, objs, first = _objects()
    tree().build()
    pos = vr.positions(pool.to_numpy()[0])
    assert pos.shape[0] == 320
    o, d = qr.rays(pos, 320)
    ref = qr.classify(pos, o, d)
    qr.caps('composed', ref)
    got = tree().intersect(o, d)
    check(ref, got, f'composed {mode}', first=first)
    assert len(set(got['object'][ref['decided'] & ref['hit']].tolist())) == 4

    moved = objs[2]
    pool.set_world(moved, _placed((0.6, 2.3, 0.8), 75.0))
    pool.compose()
    with pytest.raises(RuntimeError, match='BVH not built'):
        tree().intersect(o, d)
    with pytest.raises(RuntimeError, match='BVH not built'):
        tree().occluded(o, d)
    tree().refit()
    now = vr.positions(pool.to_numpy()[0])
    assert np.array_equal(now[:160], pos[:160]) and not np.array_equal(now[160:240], pos[160:240])
    o2, d2 = qr.rays(now, 321)
    ref2 = qr.classify(now, o2, d2)
    qr.caps('refitted', ref2)
    check(ref2, tree().intersect(o2, d2), f'refitted {mode}', first=first)
    stale = qr.errors(qr.classify(pos, o2, d2), tree().intersect(o2, d2), 'the model before the move')
    assert stale, 'the rays do not tell the moved model from the one before'

    # pick: a pixel whose camera ray is decided to hit the moved object
    pers = np.asarray(scenes.BENCH_CAMERA, np.float64)
    found = 0
    for f in range(160, 240):
        clip = pers @ np.append(now[f].mean(axis=0), 1.0)
        x, y = float(clip[0] / clip[3]), float(clip[1] / clip[3])
        if not (abs(x) < 1 and abs(y) < 1):
            continue
        ro, rd = _camera_ray(pers, x, y)
        one = qr.classify(now, ro[None], rd[None])
        if not (one['decided'][0] and one['hit'][0] and 160 <= one['index'][0] < 240):
            continue
        picked = tree().pick(x, y)
        assert picked is not None and picked[0] == moved and picked[1] == int(one['index'][0]), (mode, f, picked, int(one['index'][0]))
        assert abs(picked[2] - one['t'][0]) <= 1e-3 * one['t'][0]
        found += 1
    assert found >= 8, found


# ---------------------------------------------------------------- 8. pick
@pytest.mark.parametrize('mode', MODES)
def test_pick_names_a_face_of_the_nearest_material(fresh, mode):
    c = case('n300', preview=True)
    mat, _ = c.materials()
    _setup(c, mode)
    ij = np.argwhere(mat >= 0)
    ij = ij[np.random.default_rng(c.n).permutation(ij.shape[0])[:64]]
    assert ij.shape[0] == 64
    for i, j in ij:
        picked = tree().pick((i + 0.5) / c.nx * 2 - 1, (j + 0.5) / c.ny * 2 - 1)
        assert picked is not None, f'{mode}: pixel ({i}, {j}) of material {mat[i, j]} picks nothing'
        obj, face, depth = picked
        assert obj == -1 and c.mtlids[face] == mat[i, j] and 0 < depth < INF, f'{mode}: pixel ({i}, {j}): face {face} of material {c.mtlids[face]}, the nearest is {mat[i, j]}'
    miss = np.argwhere(c.shares()[1])
    if miss.shape[0]:
        i, j = miss[0]
        assert tree().pick((i + 0.5) / c.nx * 2 - 1, (j + 0.5) / c.ny * 2 - 1) is None

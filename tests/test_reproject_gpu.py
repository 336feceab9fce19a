'''
The film's reprojection on the GPU (FilmTable.keep_history / reproject / get_motion; csrc/history_kernel.hip, history.hip,
film_history.cpp), strict and production build (-m gpu).  Films of 1x1, 16x16, 20x12 (partial tiles) and 64x48.

1  the door: mpt_history_eval against the numpy restatement (tests/reproject_ref.py) on random inputs, accumulators and counts
   bit for bit       2  the G-buffer against the exhaustive f64 search (tests/visibility_ref.py)       3  nothing changed: keep +
   reproject(max_history = inf) is the identity, and a render that follows does not notice       4  the motion records against the
   f64 restatement: a yawed camera, a moved object, a posed skin       5  disocclusion       6  the film after resampling is the
   restatement's, from the context's own G-buffer and motion records (inside 3, 4, 5 and under stripes)       7  it helps
   8  refusals and side effects

Which pixels a test may judge: those where the exhaustive search knows the nearest face for EVERY ray of the pixel --
visibility_ref.nearest_material with every face a material of its own: a triangle covers the whole pixel (visibility_ref.covering)
and nothing else that reaches into the pixel can lie in front of it.  There the centre ray's face is that triangle, with no outlier.
'''

import numpy as np
import pytest

import reproject_ref as rr
import visibility_ref as vr
from test_visibility_ref_cpu import WORLD, case

pytestmark = pytest.mark.gpu
MODES = ['strict', 'fast']
FILMS = [(1, 1), (16, 16), (20, 12), (64, 48)]
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def film():
    from ptina_amd.things import FilmTable
    return FilmTable()


def tree():
    from ptina_amd.things import BVHTree
    return BVHTree()


def decided_faces(pers, pos, nx, ny):
    '''-> (face [nx, ny]: the nearest face of every ray of the pixel, -1 where the search does not know; full_miss [nx, ny])'''
    known, _ = vr.nearest_material(pers, pos, np.arange(pos.shape[0]), nx, ny)
    assert np.array_equal(known[known >= 0], vr.covering(pers, pos, nx, ny)[known >= 0])
    return known, vr.classify(pers, pos, nx, ny)[1]


def same_film(got, want, what):
    diff = np.flatnonzero((bits(got).reshape(-1, 4) != bits(want).reshape(-1, 4)).any(axis=1))
    assert diff.size == 0, f'{what}: {diff.size} film elements differ; first {int(diff[0])}: {got.reshape(-1, 4)[diff[0]]} against {want.reshape(-1, 4)[diff[0]]}'


def check_film(f_old, gbuf, result, nx, ny, what, own=None, **params):
    '''6: the film after reproject() is the restatement's resample step fed with the context's own G-buffer and motion records'''
    rec = film().get_motion_records()
    want, counts = rr.resample(f_old, *gbuf, rec.reshape(-1), nx, ny, own=own, **params)
    same_film(film().get_raw(), want, what)
    assert result.astuple() == tuple(counts[k] for k in rr.COUNTS), (what, result, counts)
    assert result.pixels == (nx * ny if own is None else int(np.sum(own)) * ny)
    return rec


# ---------------------------------------------------------------- 1. the door
def _door_inputs(nx, ny, seed):
    rng = np.random.default_rng(seed)
    n = nx * ny
    F = np.empty((n, 4), f32)
    F[:, 3] = rng.choice([0, 1, 4, 16, 16, 64], n).astype(f32)                      # w = 0 taps among them
    F[:, :3] = rng.random((n, 3), dtype=f32) * np.maximum(F[:, 3:], 1)
    F[rng.random(n) < 0.05, 0] = f32(-0.0)
    face = rng.integers(-1, 5, n).astype(np.int32)
    obj = np.where(face < 0, -1, rng.integers(0, 3, n)).astype(np.int32)          # ids that differ
    # depths around 5, a tap's just inside or just outside 2 % of the 5 (or nearly 5) the pixels expect
    rel = rng.choice([0.0, 0.0199, -0.0199, 0.0201, -0.0201, 0.5], n) + rng.choice([0.0, 1e-6, -1e-6], n)
    depth = (f32(5) * (1 + rel)).astype(f32)
    i, j = np.meshgrid(np.arange(nx, dtype=f32), np.arange(ny, dtype=f32), indexing='ij')
    i, j = i.reshape(-1), j.reshape(-1)
    kind = rng.integers(0, 10, n)
    off = lambda: rng.choice([-2, -1, 0, 0, 1, 2], n).astype(f32)                   # noqa: E731
    fx = np.where(kind < 3, i + off(), i + (rng.random(n, dtype=f32) * 4 - 2))      # exact integers | anywhere about the pixel
    fy = np.where(kind < 3, j + off(), j + (rng.random(n, dtype=f32) * 4 - 2))
    edge = kind == 3                                                                # in (-1, 0) and beyond the last column / row
    fx = np.where(edge, rng.choice([-0.75, -0.25, nx - 0.75, nx - 0.25, nx, nx + 3.5, -1.0], n), fx).astype(f32)
    fy = np.where(edge, rng.choice([-0.5, ny - 0.5, 0.25, ny, -1.0], n), fy).astype(f32)
    fx[kind == 4], fy[kind == 5] = np.nan, np.inf
    fx[kind == 6] = f32(1e30)
    d_exp = (f32(5) * (1 + rng.choice([0.0, 0.0, 1e-3], n))).astype(f32)
    cur = rng.integers(0, 3, n).astype(np.int32)
    flags = np.zeros(n, np.int32)
    static = kind == 7
    fx[static], fy[static], flags[static] = i[static], j[static], rr.STATIC
    miss = kind >= 8
    cur[miss] = -1
    flags[miss & (rng.random(n) < 0.6)] = rr.BACKGROUND
    return F, face, obj, depth, rr.records(nx, ny, cur.reshape(nx, ny), fx.reshape(nx, ny), fy.reshape(nx, ny), d_exp.reshape(nx, ny), flags.reshape(nx, ny))


@pytest.mark.parametrize('nx,ny', FILMS)
def test_door_against_the_restatement(fresh, nx, ny):
    from ptina_amd.common import ctx
    seen = dict.fromkeys(rr.COUNTS, 0)
    for seed in range(24 if nx * ny == 1 else 3):
        F, face, obj, depth, rec = _door_inputs(nx, ny, 100 * nx + seed)
        plain, _ = rr.resample(F, face, obj, depth, rec, nx, ny, max_history=np.inf)
        some_w = float(np.median(plain[plain[:, 3] > 0, 3])) if (plain[:, 3] > 0).any() else 16.0
        for max_history in (np.inf, 1000.0, 16.0, some_w, 4.0, 0.5):                # above, at and below R.w
            for depth_tol in (0.02, 0.25):
                want, counts = rr.resample(F, face, obj, depth, rec, nx, ny, max_history=max_history, depth_tol=depth_tol)
                got, res = ctx().history_eval(F, face, obj, depth, rec, nx, ny, max_history=max_history, depth_tol=depth_tol)
                same_film(got, want, f'door {nx}x{ny} seed {seed} max_history {max_history} depth_tol {depth_tol}')
                assert res.astuple() == tuple(counts[k] for k in rr.COUNTS) and res.pixels == nx * ny, (res, counts)
        for k in rr.COUNTS:
            seen[k] += counts[k]
    assert nx * ny < 200 or all(seen.values()), seen                                # every outcome was met (a few pixels may miss one)
    with pytest.raises(RuntimeError, match='mpt_history_eval: reproject: max_history'):
        ctx().history_eval(F, face, obj, depth, rec, nx, ny, max_history=0.0)
    with pytest.raises(RuntimeError, match='depth_tol'):
        ctx().history_eval(F, face, obj, depth, rec, nx, ny, depth_tol=np.inf)
    with pytest.raises(RuntimeError, match='max_filmsize'):
        ctx().history_eval(np.zeros((1, 4), f32)[:0], [], [], [], np.zeros(0, rr.MOTION_DTYPE), 0, 0)


# ---------------------------------------------------------------- 2. the G-buffer
def _setup(c, nx, ny, mode, scene=None, camera=None):
    from helpers import setup_engine
    return setup_engine(scene or c.scene, nx, ny, mode=mode, camera=c.camera if camera is None else camera, lights=[], world=WORLD)


def _device_rays(nx, ny):
    '''the centre rays as the context's build generates them (the camera_generate door): o, d f32 [nx * ny, 3]'''
    from ptina_amd.common import ctx
    i, j = np.meshgrid(np.arange(nx, dtype=f32), np.arange(ny, dtype=f32), indexing='ij')
    x = (i + f32(0.5)) / f32(nx) * f32(2) - f32(1)
    y = (j + f32(0.5)) / f32(ny) * f32(2) - f32(1)
    out = ctx().unit_eval('camera_generate', np.stack([x.reshape(-1), y.reshape(-1)], axis=1))
    return out[:, :3], out[:, 3:]


def _distance(pos, face, o, d):
    '''f64 Moller-Trumbore distance of ray r along its direction as given (normalised by the device) to triangle face[r]'''
    tri = pos[face]
    o, d = o.astype(np.float64), d.astype(np.float64)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    p = np.cross(d, e2)
    q = np.cross(o - tri[:, 0], e1)
    return (q * e2).sum(axis=1) / (p * e1).sum(axis=1) * np.linalg.norm(d, axis=1)


# (scene, film, the least number of pixels the search decides as one face): properties of the reference alone, asserted before any
# kernel output is looked at.  The small films of this file decide few hits on scenes of small triangles -- at 20x12 none, and the
# two triangles of n2 fill no pixel of any film: there the full misses, the ids and the launch's edges are what is held -- so n300
# and `moved` also run at the film their case is made for
GBUFFER = [('n2', 64, 64, 0), ('n2', 20, 12, 0), ('n300', 96, 80, 300), ('n300', 64, 48, 50), ('n300', 20, 12, 0), ('n1025', 64, 48, 30),
           ('n1025', 20, 12, 0), ('moved', 96, 80, 300), ('moved', 64, 48, 50)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name,nx,ny,least', GBUFFER)
def test_gbuffer_names_the_nearest_face(fresh, oracle_mod, name, nx, ny, least, mode):
    from test_query_gpu import tolerance
    c = case(name)
    known, miss = decided_faces(c.camera, c.pos, nx, ny)
    dec = known >= 0
    print(f'{name} {nx}x{ny} {mode}: {int(dec.sum())} pixels decided as one face, {int(miss.sum())} as a full miss')
    assert dec.sum() >= least and miss.sum() >= 10
    tol_depth, _ = tolerance(oracle_mod, name)
    _setup(c, nx, ny, mode)
    film().keep_history()
    face, obj, depth = film().get_gbuffer()
    bad = np.argwhere(dec & (face != known))
    assert bad.shape[0] == 0, f'{bad.shape[0]} decided pixels name another face; first {tuple(bad[0])}: {face[tuple(bad[0])]} against {known[tuple(bad[0])]}'
    assert np.all(face[miss] == -1) and np.all(obj[miss] == -1) and np.all(depth[miss] == f32(1e6))
    assert np.all(obj[face >= 0] == 0) and np.all(obj[face < 0] == -1)              # mpt_load_model brought the model
    if not dec.any():
        return
    o, d = _device_rays(nx, ny)
    at = np.flatnonzero(dec.reshape(-1))
    dev = np.abs(depth.reshape(-1)[at] - _distance(c.pos, known.reshape(-1)[at], o[at], d[at]))
    print(f'{name} {nx}x{ny} {mode}: depth deviates by {dev.max():.3g} of {tol_depth:.3g} allowed')
    assert dev.max() <= tol_depth


# ---------------------------------------------------------------- 3. nothing changed
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('nx,ny', [(20, 12), (64, 48)])
def test_keep_and_reproject_of_an_unchanged_view_is_the_identity(fresh, nx, ny, mode):
    from helpers import setup_engine
    from ptina_amd import scenes
    from ptina_amd.common import reset_all
    from ptina_amd.engine.preview import PreviewEngine
    from ptina_amd.sampling.sobol import SobolSampler

    def start():
        reset_all()
        eng = setup_engine(scenes.scene_s34(), nx, ny, mode=mode)
        PreviewEngine().render()
        eng.render(8)
        return eng

    eng = start()
    eng.render(4)
    plain = film().get_raw().copy()
    plain_sobol = SobolSampler().state()

    eng = start()
    before = film().get_raw().copy()
    assert np.all(before[:, 3] == 8) and film().get_raw(1)[:, 3].min() == 1
    film().mark()
    sobol = SobolSampler().state()
    film().keep_history()
    same_film(film().get_raw(), before, 'keep_history')
    gbuf = film().get_gbuffer()
    res = film().reproject(max_history=np.inf)
    same_film(film().get_raw(), before, f'reproject {mode}')
    vector, valid, static = film().get_motion()
    hit = gbuf[0] >= 0
    assert hit.any() and static[hit].all() and valid.all() and not vector.any()
    assert res.kept == res.static == int(hit.sum()) and res.kept + res.background_kept == nx * ny and res.pixels == nx * ny
    assert not film().get_raw(1).any() and not film().get_raw(2).any()
    with pytest.raises(RuntimeError, match='no mark'):
        film().get_noise(0.1)
    after = SobolSampler().state()
    assert sobol[0] == after[0] and np.array_equal(sobol[1], after[1]) and np.array_equal(bits(sobol[2]), bits(after[2]))
    check_film(before, [g.reshape(-1) for g in gbuf], res, nx, ny, f'identity {mode}', max_history=np.inf)
    with pytest.raises(RuntimeError, match='no history'):                           # the history is spent
        film().reproject()
    eng.render(4)
    same_film(film().get_raw(), plain, f'the render after the pair, {mode}')
    after = SobolSampler().state()
    assert plain_sobol[0] == after[0] and np.array_equal(plain_sobol[1], after[1])
    # the cap on a static film: the mean stays, the count comes down
    film().keep_history()
    film().reproject(max_history=6)
    raw = film().get_raw()
    assert np.allclose(raw[:, 3], 6, rtol=1e-6) and np.allclose(raw[:, :3] / raw[:, 3:], plain[:, :3] / plain[:, 3:], rtol=1e-5, atol=1e-7)
    keep_ms, reproject_ms, calls = film().history_kernel_time()
    assert calls == 4 and keep_ms > 0 and reproject_ms > 0 and film().history_kernel_time() == (0.0, 0.0, 0)
    film().drop_history()
    with pytest.raises(RuntimeError, match='no G-buffer'):
        film().get_gbuffer()


# ---------------------------------------------------------------- 4. motion
def _compare_motion(rec, ref, dec, tol_depth, what):
    '''the records against the f64 restatement in the decided pixels `dec` that it places in the kept view'''
    at = dec & ref['placed']
    assert at.sum() >= 40, (what, int(at.sum()))
    assert np.isfinite(rec['fx'][at]).all() and np.isfinite(rec['fy'][at]).all(), what
    dev_xy = max(np.abs(rec['fx'][at] - ref['fx'][at]).max(), np.abs(rec['fy'][at] - ref['fy'][at]).max())
    dev_d = np.abs(rec['d_exp'][at] - ref['d_exp'][at]).max()
    print(f'{what}: {int(at.sum())} pixels; fx, fy deviate by {dev_xy:.3g} px of {vr.MARGIN} allowed, d_exp by {dev_d:.3g} of {tol_depth:.3g}')
    assert dev_xy <= vr.MARGIN and dev_d <= tol_depth, what
    return dev_xy, dev_d


@pytest.mark.parametrize('mode', MODES)
def test_motion_of_a_yawed_camera(fresh, oracle_mod, mode):
    from test_query_gpu import tolerance
    from ptina_amd.things import Camera
    nx, ny = 64, 48
    c = case('n300')
    tol_depth, _ = tolerance(oracle_mod, 'n300')
    eng = _setup(c, nx, ny, mode)
    eng.render(8)
    before = film().get_raw().copy()
    film().keep_history()
    gbuf = [g.reshape(-1) for g in film().get_gbuffer()]
    new_cam = rr.yawed(c.camera, 2.0)
    Camera().set_perspective(new_cam)
    res = film().reproject()
    rec = check_film(before, gbuf, res, nx, ny, f'yaw {mode}')
    known, miss = decided_faces(new_cam, c.pos, nx, ny)
    ref = rr.motion(c.camera, new_cam, c.pos, c.pos, nx, ny)
    assert np.array_equal(ref['face'][known >= 0], known[known >= 0])
    _compare_motion(rec, ref, known >= 0, tol_depth, f'yaw 2 degrees {mode}')
    assert np.all(rec['cur_id'][known >= 0] == 0) and np.all(rec['cur_id'][miss] == -1)
    assert not (rec['flags'] != rr.NONE).any()                                      # another camera: nothing static, no background kept
    assert res.kept > 0 and res.static == 0 and res.background_kept == 0 and res.background_reset >= int(miss.sum())
    vector, valid, static = film().get_motion()
    assert valid[known >= 0].all() and not static.any() and not valid[miss].any()
    assert 1.0 < np.abs(np.median(vector[known >= 0, 0])) < 3.5


def _two_objects(skinned=False):
    '''two objects of 80 faces each, side by side in the camera's view, composed and built -> (pool, object ids).  skinned: the
    second one's mesh carries a skin of two joints, weighted by height'''
    from ptina_amd import scenes
    from ptina_amd.things import ModelPool
    from ptina_amd.tools.matrix import translate
    pool = ModelPool()
    objs = []
    for k, (seed, x) in enumerate(((1, -0.7), (2, 0.7))):
        v = np.asarray(scenes.scene_random_tris(80, seed=seed, edge=3.0)[0], np.float64).reshape(80, 3, 8)   # (triangles of some ten pixels)
        p = (v[:, :, 0:3] - [0.0, 2.0, 0.0]) * [0.3, 0.4, 0.3]
        mesh = pool.add_mesh(p, v[:, :, 3:6])
        if skinned and k == 1:
            w = np.clip(p[:, :, 1:2] / 1.6 + 0.5, 0, 1)
            weights = np.concatenate([w, 1 - w, np.zeros_like(w), np.zeros_like(w)], axis=2)
            joints = np.broadcast_to(np.array([0, 1, 0, 0]), (80, 3, 4))
            pool.add_skin(mesh, joints, weights, njoints=2)
        objs.append(pool.add_object(mesh, translate([x, 2.0, 0.0]), k))
    pool.compose()
    tree().build()
    return pool, objs


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('edit', ['set_world', 'set_joints'])
def test_motion_of_a_moved_and_of_a_posed_object(fresh, oracle_mod, edit, mode):
    from test_query_gpu import tolerance
    from ptina_amd.tools.matrix import translate
    nx, ny = 64, 48
    c = case('n300')
    tol_depth, _ = tolerance(oracle_mod, 'n300')
    eng = _setup(c, nx, ny, mode)
    pool, objs = _two_objects(skinned=edit == 'set_joints')
    first = np.array([0, 80])
    pos_kept = vr.positions(pool.to_numpy()[0])
    eng.render(8)
    before = film().get_raw().copy()
    film().keep_history()
    gbuf = [g.reshape(-1) for g in film().get_gbuffer()]
    assert set(np.unique(gbuf[1])) == {-1, 0, 1}
    if edit == 'set_world':
        th = np.radians(12.0)
        turn = np.array([[np.cos(th), -np.sin(th), 0, 0], [np.sin(th), np.cos(th), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
        pool.set_world(objs[1], translate([0.62, 2.05, 0.1]) @ turn)
    else:
        th = np.radians(15.0)
        bend = np.array([[np.cos(th), -np.sin(th), 0, 0.05], [np.sin(th), np.cos(th), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
        pool.set_joints(objs[1], np.stack([bend, np.eye(4)]))
    pool.compose()
    with pytest.raises(RuntimeError, match='BVH not built'):
        film().reproject()
    same_film(film().get_raw(), before, 'a refused reproject')
    assert tree().update() == 'refit'
    pos_new = vr.positions(pool.to_numpy()[0])
    assert np.array_equal(pos_new[:80], pos_kept[:80]) and not np.array_equal(pos_new[80:], pos_kept[80:])
    res = film().reproject()
    rec = check_film(before, gbuf, res, nx, ny, f'{edit} {mode}')
    known, miss = decided_faces(c.camera, pos_new, nx, ny)
    ref = rr.motion(c.camera, c.camera, pos_kept, pos_new, nx, ny)
    assert np.array_equal(ref['face'][known >= 0], known[known >= 0])
    moved = known >= 80
    still = (known >= 0) & ~moved
    _compare_motion(rec, ref, moved, tol_depth, f'{edit} {mode}')
    assert still.sum() >= 40 and np.all(rec['flags'][still] == rr.STATIC) and np.all(rec['cur_id'][still] == 0)
    i, j = np.meshgrid(np.arange(nx, dtype=f32), np.arange(ny, dtype=f32), indexing='ij')
    assert np.array_equal(rec['fx'][still], i[still]) and np.array_equal(rec['fy'][still], j[still])
    assert np.all(rec['cur_id'][moved] == 1) and np.all(rec['flags'][moved] == rr.NONE)
    assert np.all(rec['flags'][miss] == rr.BACKGROUND) and np.all(rec['cur_id'][miss] == -1)    # the camera stood still
    assert res.static > 0 and res.kept > res.static and res.background_kept > 0


# ---------------------------------------------------------------- 5. disocclusion
@pytest.mark.parametrize('mode', MODES)
def test_disocclusion_resets_and_the_rest_keeps(fresh, mode):
    from ptina_amd import scenes
    from ptina_amd.things import ModelPool
    from ptina_amd.tools.matrix import translate
    nx, ny = 64, 48
    c = case('n300')
    eng = _setup(c, nx, ny, mode, scene=(c.scene[0], c.scene[1], [scenes.material(basecolor=(0.7, 0.6, 0.5))] * 3, []))
    pool = ModelPool()
    nrm = np.broadcast_to([0.0, 0.0, 1.0], (2, 3, 3))
    wall = pool.add_mesh(np.array([[[-6, -3, 0], [6, -3, 0], [6, 7, 0]], [[-6, -3, 0], [6, 7, 0], [-6, 7, 0]]], np.float64), nrm)
    quad = pool.add_mesh(np.array([[[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0]], [[-0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]]], np.float64), nrm)
    objs = [pool.add_object(wall, translate([0.0, 0.0, -2.0]), 0), pool.add_object(quad, translate([-0.3, 2.0, 1.5]), 1)]
    pool.compose()
    tree().build()
    pos_kept = vr.positions(pool.to_numpy()[0])
    eng.render(8)
    before = film().get_raw().copy()
    assert np.all(before[:, 3] == 8)
    film().keep_history()
    gbuf = [g.reshape(-1) for g in film().get_gbuffer()]
    pool.set_world(objs[1], translate([0.43, 2.11, 1.5]))            # aside, by no whole number of pixels; 3.5 in front of the wall
    pool.compose()
    tree().update()
    pos_new = vr.positions(pool.to_numpy()[0])
    res = film().reproject(max_history=np.inf)
    check_film(before, gbuf, res, nx, ny, f'disocclusion {mode}', max_history=np.inf)
    raw = film().get_raw().reshape(nx, ny, 4)
    old, _ = decided_faces(c.camera, pos_kept, nx, ny)
    new, _ = decided_faces(c.camera, pos_new, nx, ny)
    was_quad, is_quad, was_wall, is_wall = old >= 2, new >= 2, (old >= 0) & (old < 2), (new >= 0) & (new < 2)
    uncovered = was_quad & is_wall
    assert uncovered.sum() >= 20 and np.all(raw[uncovered, 3] == 0) and not raw[uncovered].any()
    assert res.disoccluded >= int(uncovered.sum())
    stays = was_wall & is_wall
    assert stays.sum() >= 500
    same_film(raw[stays], before.reshape(nx, ny, 4)[stays], f'the wall before and after, {mode}')
    ref = rr.motion(c.camera, c.camera, pos_kept, pos_new, nx, ny)
    x0, y0 = np.floor(ref['fx']).astype(int), np.floor(ref['fy']).astype(int)
    inner = is_quad & ref['placed'] & (x0 >= 0) & (x0 + 1 < nx) & (y0 >= 0) & (y0 + 1 < ny)
    for a in (0, 1):
        for b in (0, 1):
            inner &= was_quad[np.clip(x0 + a, 0, nx - 1), np.clip(y0 + b, 0, ny - 1)]
    assert inner.sum() >= 20 and np.all(raw[inner, 3] > 0)
    assert np.allclose(raw[inner, 3], 8, rtol=1e-5)


# ---------------------------------------------------------------- 6. the share
@pytest.mark.parametrize('mode', MODES)
def test_stripes_resample_their_own_columns(fresh, mode):
    from ptina_amd.common import ctx
    from ptina_amd.things import Camera
    nx, ny = 64, 48
    c = case('n300')
    eng = _setup(c, nx, ny, mode)
    ctx().call('mpt_set_stripes', 16, 1, 2)                          # columns 16 .. 31 and 48 .. 63
    own = (np.arange(nx) // 16) % 2 == 1
    eng.render(8)
    before = film().get_raw().copy()
    assert np.all(before.reshape(nx, ny, 4)[own, :, 3] == 8) and not before.reshape(nx, ny, 4)[~own].any()
    film().keep_history()
    gbuf = [g.reshape(-1) for g in film().get_gbuffer()]
    for g, empty in zip(gbuf, (-1, -1, 0)):
        assert np.all(g.reshape(nx, ny)[~own] == empty)
    Camera().set_perspective(rr.yawed(c.camera, 2.0))
    res = film().reproject()
    rec = check_film(before, gbuf, res, nx, ny, f'stripes {mode}', own=own)
    assert np.all(rec.view(np.uint32).reshape(nx, ny, 5)[~own] == 0xffffffff)
    assert res.kept > 0 and not film().get_motion()[1][~own].any()
    assert not film().get_raw().reshape(nx, ny, 4)[~own].any()


# ---------------------------------------------------------------- 7. it helps
@pytest.mark.parametrize('mode', MODES)
def test_reprojected_history_beats_a_cleared_film(fresh, mode):
    '''Measured on an MI355X: see DESIGN.md section 3.18 for the ratios'''
    from helpers import setup_engine
    from ptina_amd import scenes
    from ptina_amd.things import Camera
    nx = ny = 64
    eng = setup_engine(scenes.scene_s978(), nx, ny, mode=mode)
    eng.render(64)
    film().keep_history()
    Camera().set_perspective(rr.yawed(scenes.BENCH_CAMERA, 2.0))
    res = film().reproject()
    kept = film().get_raw()[:, 3] > 0
    eng.render(4)
    A = film().get_raw().copy()
    film().clear()
    eng.render(4)
    B = film().get_raw().copy()
    film().clear()
    eng.render(1024)
    R = film().get_raw().copy()
    assert np.all(B[:, 3] == 4) and np.all(R[:, 3] == 1024) and np.allclose(A[kept, 3], 36, rtol=1e-5)

    def mse(F):
        rad = np.minimum(F[kept, :3].astype(np.float64) / F[kept, 3:], 4.0)
        return float(((rad - np.minimum(R[kept, :3].astype(np.float64) / R[kept, 3:], 4.0)) ** 2).mean())

    share = kept.mean()
    ratio = mse(A) / mse(B)
    print(f'{mode}: kept share {share:.4f} ({res}); mse with history {mse(A):.4g}, cleared {mse(B):.4g}, ratio {ratio:.4f} (ideal 0.06)')
    assert share > 0.5 and res.kept + res.background_kept == int(kept.sum())
    assert ratio < 0.5


# ---------------------------------------------------------------- 8. refusals and side effects
@pytest.mark.parametrize('mode', MODES)
def test_refusals_name_their_cause_and_leave_the_film(fresh, mode):
    from ptina_amd import scenes
    from ptina_amd.things import ModelPool
    nx, ny = 20, 12
    c = case('n300')
    eng = _setup(c, nx, ny, mode)
    eng.render(4)
    before = film().get_raw().copy()

    def refused(words, **kw):
        with pytest.raises(RuntimeError, match=words):
            film().reproject(**kw)
        same_film(film().get_raw(), before, words)

    refused('no history')
    with pytest.raises(RuntimeError, match='no motion records'):
        film().get_motion()
    film().keep_history()
    refused('max_history must be positive', max_history=0)
    refused('max_history must be positive', max_history=float('nan'))
    refused('depth_tol must be finite and positive', depth_tol=-1.0)
    film().set_size(16, 12)                                         # (smaller: the film's buffers stay)
    with pytest.raises(RuntimeError, match='the film is 16x12, the history was kept at 20x12'):
        film().reproject()
    with pytest.raises(RuntimeError, match='the G-buffer is of a film of 20x12'):
        film().get_gbuffer()
    film().set_size(nx, ny)
    same_film(film().get_raw(), before, 'set_size there and back')
    v, m = scenes.scene_random_tris(300, seed=7, edge=0.2)[:2]
    ModelPool().load(v, m)
    refused('BVH not built')                                         # as many faces, a stale tree
    ModelPool().load(v[:3 * 299], m[:299])
    refused('the model has 299 faces, the history was kept for 300')
    tree().build()
    refused('the model has 299 faces, the history was kept for 300')
    ModelPool().load(v, m)
    tree().build()
    res = film().reproject()                                         # as many faces, another model: callers are trusted, as for refit
    assert res.pixels == nx * ny
    with pytest.raises(RuntimeError, match='no history'):            # spent
        film().reproject()
    # a larger film makes the film's buffers again, the reprojection's with them
    film().keep_history()
    film().set_size(32, 32)
    with pytest.raises(RuntimeError, match='the film is 32x32, the history was kept at 20x12'):
        film().reproject()
    film().set_size(nx, ny)
    with pytest.raises(RuntimeError, match='no history: the film.s buffers were made again'):
        film().reproject()
    film().keep_history()
    assert film().reproject().pixels == nx * ny


@pytest.mark.parametrize('mode', MODES)
def test_the_pair_changes_nothing_a_render_reads_or_writes(fresh, mode):
    '''as test_query_gpu's no-side-effect test: counters, sampler, kernel choice and the film of the render that follows'''
    from helpers import setup_engine
    from ptina_amd import scenes
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.sampling.sobol import SobolSampler
    scene = scenes.scene_s34()

    def run(pair, read_between):
        reset_all()
        eng = setup_engine(scene, 24, 24, mode=mode)
        ctx().set_option('count', 1)
        eng.render(4)
        if read_between:
            film().get_raw()
        if pair:                                                    # (else: it meets the four frames still deferred, and flushes them)
            film().keep_history()
            film().reproject(max_history=np.inf)
        eng.render(4)
        raw = film().get_raw().copy()
        return raw, SobolSampler().state(), ctx().counters(), ctx().get_option('last_kernel')

    for read_between in (True, False):
        raw0, sobol0, cnt0, k0 = run(False, read_between)
        raw1, sobol1, cnt1, k1 = run(True, read_between)
        what = f'{mode}, the pair {"after a read-back" if read_between else "on deferred frames"}'
        same_film(raw1, raw0, what)
        assert raw1[:, 3].min() == 8
        assert sobol0[0] == sobol1[0] and np.array_equal(sobol0[1], sobol1[1]) and np.array_equal(bits(sobol0[2]), bits(sobol1[2])), what
        assert cnt0 == cnt1 and cnt0['samples'] > 0, (what, cnt0, cnt1)
        assert k0 == k1, what

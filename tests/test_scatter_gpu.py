'''
GPU tests (-m gpu) of scatters on the device (ModelPool.add_scatter / set_scatter / rescatter / scatter_to_numpy / scatter_of /
scatter_stats, mpt_scatter_add ... mpt_scatter_kernel_time; ptina_amd/csrc/scatter.hip, scene_scatter.cpp).

The kernels are held to tests/scatter_ref.py BIT FOR BIT -- sticky records, shares q and world matrices -- with no margin: both
sides evaluate the same expressions in f64 in the same order, every operation a correctly rounded IEEE + - * / sqrt floor.  The
surfaces are subdiv_ref's octahedron as it is (8 faces), its icosahedron at level 1 (80 faces) and -- because the icosahedron at
level 3 has 1280 = 5 x 256 faces, a multiple of the 256 a scan workgroup spans -- its 14-face bipyramid fan7 at level 3: 896 faces,
three workgroups and a half.  Surfaces stand under scatter_ref.BENT, a matrix that is not affine: w / wmax * 2^24 then lies near
an integer for no face but the largest itself (asserted here on every input, on the CPU), so the shares are compared exactly.
The density image is 2 x 2 with a zero texel and a texel above 1.
'''

import ctypes as C
import types

import numpy as np
import pytest

import compose_ref
import deform_ref
import displace_ref as dr
import scatter_ref as sc
import subdiv_ref as sr
import test_displace_gpu as dg
from test_subdiv_gpu import EYE, _ctx, _pose, _rig, _same, _set_pose, _start, _world

pytestmark = pytest.mark.gpu
u64 = np.uint64

DENSITY = np.float32([[[0, 0, 0, 0], [0.7, 0.2, 0.9, 0.4]], [[0.3, 0.6, 0.1, 0.8], [1.8, 1.2, 2.5, 1.1]]])   # 2 x 2: a zero texel, a texel above 1
IMAGES = [dg.IMAGES[0], dg.IMAGES[1], DENSITY]
TUFT = 'tetrahedron'                                                      # the instance mesh: 4 faces
# the four parameter sets every surface is scattered with: density off / on, align both ways, random yaw both ways
VARIANTS = (dict(scale=(0.05, 0.1)), dict(scale=(0.1, 0.1), align='up', up=(0.2, 1.0, -0.1), random_yaw=False, density=2, channel='r'),
            dict(scale=(0.02, 0.2), random_yaw=False, density=2, channel='mean'), dict(scale=(0.1, 0.3), align='up', up=(0, 0, -2.0)))


def _plain(pool, name):
    return pool.add_mesh(*deform_ref.split(sr.fixture(name)))


def _surface_mesh(pool, name, levels):
    return _plain(pool, name) if levels == 0 else dg._add(pool, name, levels, None)


def _surface_rec(name, levels):
    return sr.fixture(name) if levels == 0 else sr.fixture_subdivided(name, levels)


def _want(rec, world, seed, count, q=None, **kw):
    '''the restatement of a scatter with add_scatter's keywords over the surface records rec under `world`; asserts on the way that
    none of its shares but the largest's and the empty ones' lies near an integer'''
    image = None if kw.get('density') is None else IMAGES[kw['density']]
    channel = dg.CHANNELS.index(kw.get('channel', 'mean'))
    P = sc.world_corners(rec, world)
    w = sc.weights(P, None if image is None else sc.density(rec, image, channel))
    _, xs = sc.shares(w)
    flagged = sc.near_boundary(xs) & (w != w.max()) & (w != 0)
    assert flagged.mean() < 0.01 and not flagged.any(), 'precondition: a share of this input lies within 4 ulps of an integer'
    align = sc.UP if kw.get('align', 'normal') == 'up' else sc.NORMAL
    return sc.scatter(rec, world, seed, count, kw.get('scale', (1, 1)), align, kw.get('up', (0, 1, 0)), kw.get('random_yaw', True), image=image, channel=channel, q=q)


def _points_differ(got, want, what):
    for k in ('face', 'b1', 'b2', 'scale', 'cy', 'sy'):
        a, b = (got[k], want[k]) if k == 'face' else (got[k].view(u64), want[k].view(u64))
        bad = np.flatnonzero(a != b)
        assert got.shape == want.shape and bad.size == 0, (what, k, bad[:8], got[bad[:2]], want[bad[:2]])


def _worlds_differ(got, want, what):
    both_nan = np.isnan(got) & np.isnan(want)
    bad = np.flatnonzero(((got.view(u64) != want.view(u64)) & ~both_nan).any(axis=(1, 2)))
    print('%s (%d matrices): %d differ' % (what, want.shape[0], bad.size))
    assert got.shape == want.shape and bad.size == 0, (what, bad[:8], got[bad[:1]], want[bad[:1]])


def _check(pool, sid, rec, world, seed, count, what, **kw):
    '''records, shares and matrices of scatter sid against the restatement: the shares first, then the selection held to the
    device's shares (they are the restatement's), then the matrices'''
    points, worlds, q = pool.scatter_to_numpy(sid)
    want_p, want_w, want_q = _want(rec, world, seed, count, **kw)
    assert q.dtype == np.uint32 and np.array_equal(q, want_q), (what, np.flatnonzero(q != want_q)[:8])
    _points_differ(points, want_p, what)
    _worlds_differ(worlds, want_w, what)
    return points, worlds, q


def _sstats(pool):
    s = pool.scatter_stats()
    return (s.selected_scatters, s.placed_scatters, s.placed_instances), (s.weight_launches, s.scan_launches, s.select_launches, s.place_launches, s.host_fetches)


def _kernels():
    sel, plc, n = _ctx().timer('mpt_scatter_kernel_time', 2)
    assert sel >= 0 and plc >= 0
    return n


# ---------------------------------------------------------------- 1: records, shares and matrices
@pytest.mark.parametrize('count', [1, 64, 257])
@pytest.mark.parametrize('name,levels', [('octahedron', 0), ('icosahedron', 1), ('fan7', 3)])
def test_records_shares_and_matrices_equal_the_restatement_bit_for_bit(fresh, name, levels, count):
    pool = _start()
    dg._load_images(IMAGES)
    surf = pool.add_object(_surface_mesh(pool, name, levels), sc.BENT, 1)
    tuft = _plain(pool, TUFT)
    rec = _surface_rec(name, levels)
    F = rec.shape[0] // 3
    if (name, levels) == ('fan7', 3):
        assert F == 896 > sr.CHUNK and F % sr.CHUNK == 128                # more than a scan workgroup spans, and not a multiple of it
    ids = [pool.add_scatter(surf, tuft, count, seed=sc.SEED + 10 * v, mtlid=2, **kw) for v, kw in enumerate(VARIANTS)]
    assert [r for _, r in ids] == [range(1 + v * count, 1 + (v + 1) * count) for v in range(4)]
    pool.compose()
    assert _sstats(pool) == ((4, 4, 4 * count), (1, 3, 1, 1, 1)) and _kernels() == 7
    assert pool.nfaces == F + 4 * count * 4
    faces = set()
    for v, kw in enumerate(VARIANTS):
        points, worlds, q = _check(pool, ids[v][0], rec, sc.BENT, sc.SEED + 10 * v, count, '%s at level %d, %d instances, %s' % (name, levels, count, kw), **kw)
        assert (q[points['face']] > 0).all() and (worlds[:, 3] == [0, 0, 0, 1]).all()
        faces |= set(points['face'].tolist())
    if count == 257:
        assert len(faces) > min(F, 64) // 2                               # the instances spread over the surface
    pool.compose()                                                        # nothing changed: nothing launched
    assert _sstats(pool) == ((0, 0, 0), (0, 0, 0, 0, 0)) and _kernels() == 0 and pool.compose_stats().dirty_objects == 0


# ---------------------------------------------------------------- 2: the composed model
def test_composed_instances_equal_the_composition_of_the_fetched_matrices(fresh):
    from ptina_amd.multimesh import compose_multiple_meshes
    pool = _start()
    surf = pool.add_object(_surface_mesh(pool, 'icosahedron', 1), sc.BENT, 1)
    other = pool.add_object(_plain(pool, 'octahedron'), _world(3), 0)
    tuft = _plain(pool, TUFT)
    pool.compose()
    s = pool.scatter_stats()                                              # a scene without a scatter: no scatter launch
    assert (s.scatters, s.instances) == (0, 0) and _sstats(pool) == ((0, 0, 0), (0, 0, 0, 0, 0)) and _kernels() == 0
    before, before_m = pool.to_numpy()
    sid, objs = pool.add_scatter(surf, tuft, 64, seed=5, mtlid=2, scale=(0.05, 0.2))
    late = pool.add_object(_plain(pool, 'pair'), _world(4), 1)            # an object behind the instances
    pool.compose()
    got, got_m = pool.to_numpy()
    points, worlds, _ = _check(pool, sid, sr.fixture_subdivided('icosahedron', 1), sc.BENT, 5, 64, 'icosahedron', scale=(0.05, 0.2))
    prims = sc.instance_primitives(sr.fixture(TUFT), worlds, 2)
    ref, ref_m = compose_multiple_meshes(prims)
    worst, closest, n = compose_ref.margin(prims, ref)
    print('instances: %d values, the closest %.3g error bounds (%.3g f32 ulp) from an f32 rounding boundary' % (n, worst, closest))
    assert worst > compose_ref.MARGIN, 'precondition: pick another seed'
    a = before.shape[0]
    assert _same(got[a:a + 3 * 4 * 64], ref.astype(np.float32)) and np.array_equal(got_m[a // 3:a // 3 + 4 * 64], ref_m)
    assert _same(got[:a], before) and np.array_equal(got_m[:a // 3], before_m)   # the rest of the scene is untouched
    pair = compose_multiple_meshes([(*deform_ref.split(sr.fixture('pair')), _world(4), 1)])[0]
    assert np.allclose(got[a + 3 * 4 * 64:], pair, rtol=1e-6, atol=1e-7) and pool.nfaces == 80 + 8 + 256 + 2
    assert pool.scatter_of(objs[7]) == (sid, 7) and pool.scatter_of(surf) is None and pool.scatter_of(late) is None and pool.scatter_of(other) is None


# ---------------------------------------------------------------- 3: stickiness
STICKY_DISP = (1, dr.NORMAL, dr.A, 0.3, 0.45)


def _sticky_scene(pool, count, mode=None):
    '''a skinned, subdivided, displaced cylinder with `count` tufts on it, and an octahedron beside it'''
    rig = _rig('cylinder', 2)
    mesh = dg._add(pool, 'cylinder', 2, STICKY_DISP, rig)
    surf = pool.add_object(mesh, _world(21), 1)
    other = pool.add_object(_plain(pool, 'octahedron'), _world(22), 0)
    pose = _pose(42)
    _set_pose(pool, surf, pose)
    sid, objs = pool.add_scatter(surf, _plain(pool, TUFT), count, seed=9, mtlid=2, scale=(0.03, 0.08))
    return rig, mesh, surf, other, pose, sid, objs


def test_instances_stick_to_a_surface_that_is_posed_and_displaced_again(fresh):
    pool = _start()
    dg._load_images(IMAGES)
    count = 257
    rig, mesh, surf, other, pose, sid, objs = _sticky_scene(pool, count)
    pool.compose()
    rec = dg._expected('cylinder', 2, STICKY_DISP, rig, pose)
    dg._differ(pool.subdivided_to_numpy(surf), rec, 'the surface')
    points, worlds, q = _check(pool, sid, rec, _world(21), 9, count, 'posed cylinder', scale=(0.03, 0.08))
    assert _sstats(pool) == ((1, 1, count), (1, 3, 1, 1, 1))
    fetches = pool.compose_stats().host_fetches
    _kernels()
    # another pose and another strength: the records stay, the matrices follow the surface
    pose2 = _pose(43)
    _set_pose(pool, surf, pose2)
    pool.set_displacement(mesh, -0.2)
    pool.compose()
    c = pool.compose_stats()
    assert _sstats(pool) == ((0, 1, count), (0, 0, 0, 1, 0)) and _kernels() == 1
    assert (c.dirty_objects, c.recomposed) == (1 + count, 512 + 4 * count) and c.host_fetches == fetches
    rec2 = dg._expected('cylinder', 2, (1, dr.NORMAL, dr.A, -0.2, 0.45), rig, pose2)
    points2, worlds2, q2 = pool.scatter_to_numpy(sid)
    _points_differ(points2, points, 'the records after the edit')
    assert np.array_equal(q2, q)
    want = sc.place(sc.world_corners(rec2, _world(21)), points)
    _worlds_differ(worlds2, want, 'the matrices after the edit')
    assert not np.array_equal(worlds2, worlds)
    # the surface moved as a whole: placement alone again
    pool.set_world(surf, _world(23))
    pool.compose()
    assert _sstats(pool) == ((0, 1, count), (0, 0, 0, 1, 0))
    _worlds_differ(pool.scatter_to_numpy(sid)[1], sc.place(sc.world_corners(rec2, _world(23)), points), 'the matrices after set_world')
    # another object moved: the scatter sits the compose out
    pool.set_world(other, _world(24))
    pool.compose()
    assert _sstats(pool) == ((0, 0, 0), (0, 0, 0, 0, 0)) and pool.compose_stats().dirty_objects == 1
    # a material of an instance: allowed; its row goes up from the host, so its scatter places again, and the matrices stay
    pool.set_material(objs[3], 0)
    pool.compose()
    assert _sstats(pool) == ((0, 1, count), (0, 0, 0, 1, 0))
    _worlds_differ(pool.scatter_to_numpy(sid)[1], sc.place(sc.world_corners(rec2, _world(23)), points), 'the matrices after set_material')
    m = pool.to_numpy()[1]
    first = 512 + 8
    assert (m[first + 12:first + 16] == 0).all() and (m[first:first + 12] == 2).all() and (m[first + 16:] == 2).all()


# ---------------------------------------------------------------- 4: refit
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_an_edit_of_the_surface_then_update_refits(fresh, mode):
    import query_ref as qr
    import visibility_ref as vr
    from ptina_amd.things import BVHTree
    pool = _start(mode)
    dg._load_images(IMAGES)
    count = 64
    rig, mesh, surf, other, pose, sid, objs = _sticky_scene(pool, count, mode)
    pool.compose()
    tree = BVHTree()
    tree.build()
    _set_pose(pool, surf, _pose(43))
    pool.set_displacement(mesh, 0.1)
    pool.compose()
    assert _sstats(pool)[1] == (0, 0, 0, 1, 0) and pool.nfaces == 512 + 8 + 4 * count
    assert tree.update(max_growth=float('inf')) == 'refit' and tree.refit_stats().refits == 1 and tree.refit_stats().host_fetches == 0
    model, _ = pool.to_numpy()
    pos = vr.positions(model)
    first = np.array([0, 512] + [512 + 8 + 4 * i for i in range(count)])
    o, d = qr.rays(pos, 4, 256)
    ref = qr.classify(pos, o, d)
    dec = ref['decided']
    assert dec.mean() >= 0.9 and (dec & ref['hit']).any() and (dec & ~ref['hit']).any()
    refitted = tree.intersect(o, d)
    bad = qr.errors(ref, refitted, 'refitted %s' % mode, first=first)
    assert not bad, bad[:4]
    tree.build()                                                          # a tree freshly built on the same model
    built = tree.intersect(o, d)
    bad = qr.errors(ref, built, 'built %s' % mode, first=first)
    assert not bad, bad[:4]
    for k in ('hit', 'index', 'object'):
        assert np.array_equal(np.asarray(refitted[k])[dec], np.asarray(built[k])[dec]), k


# ---------------------------------------------------------------- 5: rescatter and set_scatter
def test_rescatter_and_set_scatter_select_again(fresh):
    pool = _start()
    dg._load_images(IMAGES)
    surf = pool.add_object(_surface_mesh(pool, 'fan7', 3), sc.BENT)
    rec = sr.fixture_subdivided('fan7', 3)
    sid, objs = pool.add_scatter(surf, _plain(pool, TUFT), 64, seed=1)
    pool.compose()
    p1, w1, q1 = _check(pool, sid, rec, sc.BENT, 1, 64, 'seed 1')
    pool.rescatter(sid, 2)
    with pytest.raises(RuntimeError, match='scatter %d has not been placed yet' % sid):
        pool.scatter_to_numpy(sid)
    pool.compose()
    assert _sstats(pool) == ((1, 1, 64), (1, 3, 1, 1, 1)) and pool.compose_stats().dirty_objects == 64
    p2, w2, q2 = _check(pool, sid, rec, sc.BENT, 2, 64, 'seed 2')
    assert not np.array_equal(p1['face'], p2['face']) and np.array_equal(q1, q2)
    pool.rescatter(sid, 1)
    pool.compose()
    p3, w3, _ = pool.scatter_to_numpy(sid)
    _points_differ(p3, p1, 'the old seed')
    _worlds_differ(w3, w1, 'the old seed')
    pool.rescatter(sid)                                                   # None: the seed after the last
    pool.compose()
    _points_differ(pool.scatter_to_numpy(sid)[0], p2, 'rescatter() without a seed')
    # new parameters: a density, another range of scales, another alignment
    kw = dict(scale=(0.5, 0.75), align='up', up=(1.0, 0, 0), density=2, channel='g')
    pool.set_scatter(sid, **kw)
    pool.compose()
    assert _sstats(pool)[1] == (1, 3, 1, 1, 1)
    _check(pool, sid, rec, sc.BENT, 2, 64, 'after set_scatter', random_yaw=True, **kw)
    with pytest.raises(ValueError, match='unknown scatter parameters: colour'):
        pool.set_scatter(sid, colour=1)


# ---------------------------------------------------------------- 6: a mixed scene
def test_mixed_scene_takes_one_launch_of_each_kind(fresh):
    import query_ref as qr
    import visibility_ref as vr
    from ptina_amd.things import BVHTree
    pool = _start('fast')
    dg._load_images(IMAGES)
    s0 = pool.add_object(_surface_mesh(pool, 'icosahedron', 1), sc.BENT, 0)
    hand = pool.add_object(_plain(pool, 'octahedron'), _world(5), 1)
    s1 = pool.add_object(_surface_mesh(pool, 'grid', 2), _world(6), 2)
    tuft = _plain(pool, TUFT)
    disp = (0, dr.VECTOR, dr.R, 0.2, 0.4)
    knob = dg._add(pool, 'tetrahedron', 1, disp)                          # a subdivided, displaced instance mesh: one shared copy
    a, objs_a = pool.add_scatter(s0, tuft, 300, seed=3, scale=(0.05, 0.1))
    hand2 = pool.add_object(tuft, _world(7), 1)
    b, objs_b = pool.add_scatter(s1, knob, 100, seed=4, scale=(0.1, 0.2), density=2, channel='b', random_yaw=False)
    pool.compose()
    assert _sstats(pool) == ((2, 2, 400), (1, 3, 1, 1, 1)) and _kernels() == 7
    assert pool.subdiv_stats().copies == 3 and pool.nfaces == 80 + 8 + 800 + 300 * 4 + 4 + 100 * 16
    _check(pool, a, sr.fixture_subdivided('icosahedron', 1), sc.BENT, 3, 300, 'the first scatter', scale=(0.05, 0.1))
    pb, wb, _ = _check(pool, b, sr.fixture_subdivided('grid', 2), _world(6), 4, 100, 'the second scatter', scale=(0.1, 0.2), density=2, channel='b', random_yaw=False)
    # the instances of the second scatter are the displaced copy under their matrices (the first instance, to f32 rounding)
    copy = pool.subdivided_to_numpy(objs_b[0])
    dg._differ(copy, dg._expected('tetrahedron', 1, disp), 'the shared copy of the instance mesh')
    model, _ = pool.to_numpy()
    at = 3 * (80 + 8 + 800 + 1200 + 4)
    ph = np.concatenate([copy[:, :3].astype(np.float64), np.ones((48, 1))], axis=1) @ wb[0].T
    assert np.allclose(model[at:at + 48, :3], ph[:, :3], rtol=1e-6, atol=1e-7)
    # one surface moves: its scatter alone places, in one launch
    pool.set_world(s1, _world(8))
    pool.compose()
    assert _sstats(pool) == ((0, 1, 100), (0, 0, 0, 1, 0)) and pool.compose_stats().dirty_objects == 101
    _worlds_differ(pool.scatter_to_numpy(b)[1], sc.place(sc.world_corners(sr.fixture_subdivided('grid', 2), _world(8)), pb), 'the second scatter, moved')
    # every object maps back
    for o in range(len(pool._obj_mesh)):
        want = (a, o - objs_a.start) if o in objs_a else (b, o - objs_b.start) if o in objs_b else None
        assert pool.scatter_of(o) == want
    tree = BVHTree()
    tree.build()
    pos = vr.positions(pool.to_numpy()[0])
    o, d = qr.rays(pos, 4, 256)
    res = tree.intersect(o, d)
    hit = np.asarray(res['hit']).astype(bool)
    seen = set(np.asarray(res['object'])[hit].tolist())
    assert seen & set(objs_a) and seen - set(objs_a) - set(objs_b)        # instances and hand-added objects are picked
    first = np.concatenate([[0], np.cumsum([pool._object_faces(m) for m in pool._obj_mesh])])
    for obj, face in zip(np.asarray(res['object'])[hit].tolist(), np.asarray(res['index'])[hit].tolist()):
        assert first[obj] <= face < first[obj + 1]
        assert (pool.scatter_of(obj) is not None) == (obj in objs_a or obj in objs_b)


# ---------------------------------------------------------------- 6b: the instances' own mesh is displaced again
def test_instances_keep_their_place_when_their_own_mesh_is_displaced_again(fresh):
    '''the instances of a subdivided, displaced mesh share its one copy: set_displacement of that mesh, and a reload of the images,
    mark every instance changed, and their rows would go up from the host's table with the placeholder matrix -- the scatter places
    again instead: the matrices stay bit for bit, and the composed instances are the new copy under them'''
    from ptina_amd.multimesh import compose_multiple_meshes
    pool = _start()
    dg._load_images(IMAGES)
    surf = pool.add_object(_surface_mesh(pool, 'icosahedron', 1), sc.BENT, 0)
    disp = (0, dr.VECTOR, dr.R, 0.2, 0.4)
    knob = dg._add(pool, 'tetrahedron', 1, disp)
    count = 40
    sid, objs = pool.add_scatter(surf, knob, count, seed=4, mtlid=1, scale=(0.1, 0.2))
    pool.compose()
    points, worlds, q = _check(pool, sid, sr.fixture_subdivided('icosahedron', 1), sc.BENT, 4, count, 'at first', scale=(0.1, 0.2))

    def composed(disp, images, what):
        copy = dg._expected('tetrahedron', 1, disp, images=images)
        dg._differ(pool.subdivided_to_numpy(objs[0]), copy, 'the shared copy ' + what)
        prims = sc.instance_primitives(copy, worlds, 1)
        ref, ref_m = compose_multiple_meshes(prims)
        worst, closest, n = compose_ref.margin(prims, ref)
        print('%s: %d values, the closest %.3g error bounds from an f32 rounding boundary' % (what, n, worst))
        assert worst > compose_ref.MARGIN, 'precondition: pick another seed'
        got, got_m = pool.to_numpy()
        assert got.shape[0] == 3 * (80 + 16 * count) and _same(got[240:], ref.astype(np.float32)) and np.array_equal(got_m[80:], ref_m), what
        return got
    first = composed(disp, IMAGES, 'at first')
    _kernels()

    def unmoved(what):
        c = pool.compose_stats()
        assert _sstats(pool) == ((0, 1, count), (0, 0, 0, 1, 0)) and _kernels() == 1 and (c.dirty_objects, c.recomposed) == (count, 16 * count), what
        p2, w2, q2 = pool.scatter_to_numpy(sid)
        _points_differ(p2, points, what)
        _worlds_differ(w2, worlds, what)
    disp2 = (0, dr.VECTOR, dr.R, -0.15, 0.4)
    pool.set_displacement(knob, -0.15)
    pool.compose()
    unmoved('after set_displacement of the instance mesh')
    second = composed(disp2, IMAGES, 'after set_displacement of the instance mesh')
    assert not _same(first, second)
    other = [dr.random_image(21, 4, 3), IMAGES[1], IMAGES[2]]
    dg._load_images(other)
    pool.compose()
    unmoved('after an image reload')
    third = composed(disp2, other, 'after an image reload')
    assert not _same(second, third)


# ---------------------------------------------------------------- 7: refusals
def test_refusals_say_what_is_wrong_and_leave_the_scene(fresh):
    from ptina_amd import _lib
    pool = _start()
    dg._load_images(IMAGES[:2])                                           # (the density image, id 2, is not loaded yet)
    c = _ctx()
    surf = pool.add_object(_surface_mesh(pool, 'icosahedron', 1), sc.BENT)
    tuft = _plain(pool, TUFT)
    soft = pool.add_mesh(*deform_ref.split(sr.fixture('cylinder')))
    rig = _rig('cylinder', 2)
    pool.add_skin(soft, rig['jt'], rig['wt'], rig['nj'])
    pool.compose()
    model = pool.to_numpy()[0]

    def add(surface=surf, mesh=tuft, count=8, **kw):
        sid, first = C.c_int(-1), C.c_int(-1)
        p = kw.pop('params', None) or _lib.scatter_params(**kw)
        c.call('mpt_scatter_add', surface, mesh, count, 1, -1, C.byref(p), C.byref(sid), C.byref(first))
    with pytest.raises(RuntimeError, match='unknown surface object 99'):
        add(surface=99)
    with pytest.raises(RuntimeError, match='unknown mesh 99'):
        add(mesh=99)
    with pytest.raises(RuntimeError, match='count 0 is below 1'):
        add(count=0)
    with pytest.raises(RuntimeError, match='too many faces: .* instances of mesh %d' % tuft):
        add(count=2 ** 19)
    with pytest.raises(RuntimeError, match='the scale range is empty: smin 2 above smax 1'):
        add(scale=(2.0, 1.0))
    for bad in ((float('nan'), 1.0), (0.0, float('inf'))):
        with pytest.raises(RuntimeError, match='the scale range is not finite'):
            add(scale=bad)
    with pytest.raises(RuntimeError, match=r'up \(0, 0, 0\) has no direction'):
        add(align='up', up=(0, 0, 0))
    with pytest.raises(RuntimeError, match='up is not finite'):
        add(up=(0, float('nan'), 1))
    with pytest.raises(RuntimeError, match='mesh %d carries morph targets or a skin' % soft):
        add(mesh=soft)
    for image in (64, -2):
        p = _lib.scatter_params()
        p.density_image = image
        with pytest.raises(RuntimeError, match=r'density image %d outside \[-1, 64\)' % image):
            add(params=p)
    p = _lib.scatter_params()
    p.align = 2
    with pytest.raises(RuntimeError, match=r'align 2 outside \[0, 1\]'):
        add(params=p)
    # ... and the Python side keeps the same books
    with pytest.raises(ValueError, match='unknown object'):
        pool.add_scatter(99, tuft, 8)
    with pytest.raises(ValueError, match='unknown mesh'):
        pool.add_scatter(surf, 99, 8)
    with pytest.raises(ValueError, match='below 1'):
        pool.add_scatter(surf, tuft, 0)
    with pytest.raises(ValueError, match='too many faces'):
        pool.add_scatter(surf, tuft, 2 ** 19)
    with pytest.raises(ValueError, match='unknown scatter'):
        pool.rescatter(0)
    s = pool.scatter_stats()
    assert (s.scatters, s.instances) == (0, 0) and len(pool._obj_mesh) == 1
    pool.compose()
    assert _same(pool.to_numpy()[0], model) and pool.nfaces == 80
    # a scatter whose density image is not loaded: compose refuses before anything changes, and succeeds once the image is there
    sid, objs = pool.add_scatter(surf, tuft, 8, seed=1, density=2, channel='a', scale=(0.1, 0.1))
    for _ in range(2):
        with pytest.raises(RuntimeError, match='the density of scatter %d reads image 2, and 2 images are loaded' % sid):
            pool.compose()
    assert _same(pool.to_numpy()[0], model) and _kernels() == 0
    # the surface may not be an instance; an instance may not be moved by hand
    with pytest.raises(RuntimeError, match='the surface, object %d, is itself an instance of scatter %d' % (objs[2], sid)):
        add(surface=objs[2])
    with pytest.raises(ValueError, match='itself an instance of scatter %d' % sid):
        pool.add_scatter(objs[2], tuft, 8)
    with pytest.raises(RuntimeError, match='object %d is an instance of scatter %d' % (objs[1], sid)):
        pool.set_world(objs[1], EYE)
    # an image without weight: refused when the weights are there, naming the surface; the composed model stays
    dg._load_images([IMAGES[0], IMAGES[1], np.zeros((2, 2, 4), np.float32)])
    for _ in range(2):
        with pytest.raises(RuntimeError, match='scatter %d: its surface, object %d, has no face with a weight above 0' % (sid, surf)):
            pool.compose()
    assert _same(pool.to_numpy()[0], model)
    with pytest.raises(RuntimeError, match='has not been placed yet'):
        pool.scatter_to_numpy(sid)
    dg._load_images(IMAGES)
    pool.compose()
    _check(pool, sid, sr.fixture_subdivided('icosahedron', 1), sc.BENT, 1, 8, 'after the refusals', density=2, channel='a', scale=(0.1, 0.1))
    assert _same(pool.to_numpy()[0][:240], model) and pool.nfaces == 80 + 32
    # a surface without faces
    pool.clear_objects()
    empty = pool.add_object(pool.add_mesh(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32)), EYE)
    pool.add_scatter(empty, tuft, 4)
    with pytest.raises(RuntimeError, match='scatter 0: its surface, object %d, has no faces' % empty):
        pool.compose()


def test_density_refuses_surface_uvs_the_displacement_would_refuse(fresh):
    '''with a density image the corner uvs of the surface's mesh are admitted as a displaced mesh's are: finite and at most 2^20 in
    magnitude, the corner named; without one they are not read'''
    pool = _start()
    dg._load_images(IMAGES)
    tuft = _plain(pool, TUFT)
    surfs = []
    for value, ok in ((np.nan, False), (np.inf, False), (2.0 ** 20 + 1, False), (-2.0 ** 20, True)):
        rec = np.array(sr.fixture('octahedron'))
        rec[3 * 2 + 1, 7] = value
        mesh = pool.add_mesh(*deform_ref.split(rec))
        surfs.append(pool.add_object(mesh, sc.BENT))
        nobj, nsc = len(pool._obj_mesh), pool.scatter_stats().scatters
        if ok:
            pool.add_scatter(surfs[-1], tuft, 4, density=2, channel='g')
            continue
        with pytest.raises(RuntimeError, match=r'mpt_scatter_add: the surface, object %d of mesh %d: .*the uv of corner 1 of face 2 is not finite or exceeds 2\^20' % (surfs[-1], mesh)):
            pool.add_scatter(surfs[-1], tuft, 4, density=2, channel='g')
        assert len(pool._obj_mesh) == nobj and pool.scatter_stats().scatters == nsc and pool.scatter_of(nobj) is None
    sid, objs = pool.add_scatter(surfs[2], tuft, 4, seed=3)              # no density: the uvs are not read
    with pytest.raises(RuntimeError, match=r'mpt_scatter_set_params: the surface, object %d of mesh .*exceeds 2\^20' % surfs[2]):
        pool.set_scatter(sid, density=2)
    pool.compose()
    assert _sstats(pool) == ((2, 2, 8), (1, 3, 1, 1, 1)) and pool.nfaces == 4 * 8 + 8 * 4
    rec = np.array(sr.fixture('octahedron'))
    rec[3 * 2 + 1, 7] = 2.0 ** 20 + 1
    _check(pool, sid, rec, sc.BENT, 3, 4, 'a surface whose uvs are not read')


# ---------------------------------------------------------------- 8: scene lifetime
def test_clear_and_mesh_add_while_scatters_exist(fresh):
    pool = _start()
    dg._load_images(IMAGES)
    disp = (1, dr.NORMAL, dr.MEAN, 0.2, 0.5)
    ms = dg._add(pool, 'grid', 2, disp)
    surf = pool.add_object(ms, _world(1))
    tuft = _plain(pool, TUFT)
    sid, objs = pool.add_scatter(surf, tuft, 64, seed=6, scale=(0.05, 0.1), density=2)
    pool.compose()
    rec = dg._expected('grid', 2, disp)
    p1, w1, q1 = _check(pool, sid, rec, _world(1), 6, 64, 'at first', scale=(0.05, 0.1), density=2)
    # a mesh joins the pool where the copies lay; an object of it joins the table: the records stay, everything is placed again
    extra = pool.add_object(_surface_mesh(pool, 'icosahedron', 1), _world(2))
    pool.compose()
    assert _sstats(pool) == ((0, 1, 64), (0, 0, 0, 1, 0))
    p2, w2, q2 = pool.scatter_to_numpy(sid)
    _points_differ(p2, p1, 'after a mesh and an object were added')
    _worlds_differ(w2, w1, 'after a mesh and an object were added')
    assert pool.nfaces == 800 + 256 + 80
    # clear_objects: the scatters go with the objects, the meshes stay
    pool.clear_objects()
    s = pool.scatter_stats()
    assert (s.scatters, s.instances) == (0, 0) and pool.scatter_of(1) is None
    with pytest.raises(ValueError, match='unknown scatter'):
        pool.scatter_to_numpy(sid)
    surf = pool.add_object(ms, _world(3))
    sid, objs = pool.add_scatter(surf, tuft, 65, seed=7)
    assert sid == 0 and objs == range(1, 66)
    pool.compose()
    _check(pool, sid, rec, _world(3), 7, 65, 'after clear_objects')
    assert pool.nfaces == 800 + 260
    # clear_meshes: everything goes
    pool.clear_meshes()
    assert pool.scatter_stats().scatters == 0
    surf = pool.add_object(_plain(pool, 'octahedron'), sc.BENT)
    sid, objs = pool.add_scatter(surf, _plain(pool, TUFT), 3, seed=8)
    pool.compose()
    _check(pool, sid, sr.fixture('octahedron'), sc.BENT, 8, 3, 'after clear_meshes')
    assert pool.nfaces == 8 + 12


# ---------------------------------------------------------------- 8b: the books of a scene built in pieces
def test_a_scene_built_in_pieces_equals_the_same_scene_built_at_once(fresh):
    '''a scene whose objects use every per-object fact the host keeps -- a mesh, a pose, a subdivided copy, a scatter -- built in an
    awkward order (a mesh joins behind an object, its rig and level come later, a plain object stands behind the instances), composed,
    cleared and added again in another order: everything read back equals, bit for bit, what a fresh context makes of the final
    scene added once.  Row bookkeeping is what can go wrong here; the arithmetic is the other tests' '''
    rig, pose = _rig('fan7', 5), _pose(44)
    kw = dict(seed=11, mtlid=2, scale=(0.05, 0.2))

    def meshes(pool, between=lambda mesh: None):
        plain = _plain(pool, 'octahedron')
        between(plain)
        soft = _plain(pool, 'fan7')                                       # behind the first object: the copies lose their room
        pool.add_morph_targets(soft, rig['dp'], rig['dn'])
        pool.add_skin(soft, rig['jt'], rig['wt'], rig['nj'])
        pool.add_subdivision(soft, 1)
        return plain, soft

    def rigged(pool, soft):
        obj = pool.add_object(soft, _world(31), 1)
        _set_pose(pool, obj, pose)
        return obj

    def read(pool, sid, soft_obj):
        model, mtlids = pool.to_numpy()
        points, worlds, q = pool.scatter_to_numpy(sid)
        return dict(model=model, mtlids=mtlids, points=points.view(np.uint8), worlds=worlds.view(u64), q=q,
                    subdivided=pool.subdivided_to_numpy(soft_obj), deformed=pool.deformed_to_numpy(soft_obj))

    # in pieces
    pool = _start()
    first = []
    plain, soft = meshes(pool, lambda mesh: first.append(pool.add_object(mesh, sc.BENT, 0)))
    soft_obj = rigged(pool, soft)
    knob = dg._add(pool, 'octahedron', 1, None)
    sid, objs = pool.add_scatter(first[0], knob, 3, **kw)
    ico = _plain(pool, 'icosahedron')
    late = pool.add_object(ico, _world(32), 1)                            # a plain object behind the instances
    assert (first[0], soft_obj, list(objs), late) == (0, 1, [2, 3, 4], 5)
    pool.compose()
    assert pool.nfaces == 8 + 56 + 3 * 32 + 20
    pool.clear_objects()
    late = pool.add_object(ico, _world(32), 1)                            # ... the plain object first this time
    surf = pool.add_object(plain, sc.BENT, 0)
    soft_obj = rigged(pool, soft)
    sid, objs = pool.add_scatter(surf, knob, 3, **kw)
    assert (late, surf, soft_obj, sid, list(objs)) == (0, 1, 2, 0, [3, 4, 5])
    pool.compose()
    got = read(pool, sid, soft_obj)
    assert pool.nfaces == 20 + 8 + 56 + 3 * 32 and pool.subdiv_stats().copies == 2 and pool.deform_stats().deformable_objects == 1

    # at once, in a fresh context
    pool = _start()
    plain, soft = meshes(pool)
    knob = dg._add(pool, 'octahedron', 1, None)
    ico = _plain(pool, 'icosahedron')
    late = pool.add_object(ico, _world(32), 1)
    surf = pool.add_object(plain, sc.BENT, 0)
    soft_obj = rigged(pool, soft)
    sid, objs = pool.add_scatter(surf, knob, 3, **kw)
    pool.compose()
    want = read(pool, sid, soft_obj)
    for k in want:
        assert _same(got[k], want[k]), k
    assert got['model'].shape[0] == 3 * 180 and got['subdivided'].shape[0] == 3 * 56 and got['deformed'].shape[0] == 3 * 14


# ---------------------------------------------------------------- 9: the worker facade
def test_worker_facade_through_the_thread_proxy(fresh):
    import threading
    from ptina_amd.common import reset_all
    from ptina_amd.tools.mtworker import DaemonModule, OnDemandProxy
    reset_all()
    seen = []

    def module():
        seen.append(threading.get_ident())
        from ptina_amd import worker
        ns = types.SimpleNamespace(**{k: getattr(worker, k) for k in dir(worker) if not k.startswith('_')})
        ns.add_mesh = lambda name: worker.ModelPool().add_mesh(*deform_ref.split(sr.fixture(name)))
        ns.add_object = lambda mesh: worker.ModelPool().add_object(mesh, sc.BENT)
        ns.fetch = lambda sid: worker.ModelPool().scatter_to_numpy(sid)
        return ns
    w = OnDemandProxy(lambda: DaemonModule(module))
    w.init()
    surf = w.add_object(w.add_mesh('octahedron'))
    sid, objs = w.add_scatter(surface=surf, mesh=w.add_mesh(TUFT), count=33, seed=12, scale=(0.1, 0.2))
    assert seen and seen[0] != threading.get_ident() and objs == range(1, 34)
    w.compose_model()
    want_p, want_w, want_q = _want(sr.fixture('octahedron'), sc.BENT, 12, 33, scale=(0.1, 0.2))
    points, worlds, q = w.fetch(sid)
    assert np.array_equal(q, want_q)
    _points_differ(points, want_p, 'through the worker')
    _worlds_differ(worlds, want_w, 'through the worker')
    w.rescatter(sid, 13)
    w.compose_model()
    _points_differ(w.fetch(sid)[0], _want(sr.fixture('octahedron'), sc.BENT, 13, 33, scale=(0.1, 0.2))[0], 'through the worker, scattered again')
    w.rescatter(scatter=sid)
    w.compose_model()
    _points_differ(w.fetch(sid)[0], _want(sr.fixture('octahedron'), sc.BENT, 14, 33, scale=(0.1, 0.2))[0], 'through the worker, the next seed')
    w.synchronize()

'''
GPU tests (-m gpu) of keyframe animation on the device (ModelPool.add_skeleton / add_clip / set_animation / set_time / pose_to_numpy /
anim_stats, mpt_mesh_set_skeleton ... mpt_anim_kernel_time; ptina_amd/csrc/anim.hip, scene_anim.cpp).

The kernel is held to tests/anim_ref.py: BIT FOR BIT for every object whose rotation tracks stay out of the slerp's theta branch, and
within anim_ref.error_bound -- with the device library's measured acos and sin error, ULP_TRIG_DEVICE -- for the others.  The deformed
copies are held to tests/deform_ref.py fed the palette FETCHED from the device, bit for bit: the deform kernel is exact given its
pose, so the feature's only tolerance sits in one place.  The cases are anim_ref.cases(): every one is a mesh of
tests/golden/reference_compose.npz (0, 1, 21, 22, 85, 86, 300 faces) with a random rig, its clip, and an object per binding, all in
ONE scene beside an unbound object posed by set_joints, so that one launch poses objects of different rigs and clips.
'''

import ctypes as C
import os
import types

import numpy as np
import pytest

import anim_ref as ar
import deform_ref

pytestmark = pytest.mark.gpu
u32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ar.cases()
NAMES = [c[0] for c in CASES]


@pytest.fixture(scope='module')
def gold():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_compose.npz'))
    meshes = [deform_ref.records(g['mesh%d_p' % i], g['mesh%d_n' % i], g['mesh%d_t' % i]) for i in range(int(g['nmeshes']))]
    worlds = [np.array(w, np.float64) for w in g['obj_world']]
    assert sorted(r.shape[0] // 3 for r in meshes) == [0, 1, 21, 22, 85, 86, 300]
    return sorted(meshes, key=lambda r: -r.shape[0]), worlds


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u32), b.view(u32))


def _ctx():
    from ptina_amd.common import ctx
    return ctx()


def _start(mode=None):
    from ptina_amd import _lib
    from ptina_amd.common import reset_all
    from ptina_amd.things import init_things, ModelPool
    reset_all()
    init_things()
    if mode is not None:
        from ptina_amd import scenes
        from ptina_amd.engine.path import PathEngine
        from ptina_amd.things import FilmTable, Camera
        PathEngine()
        _ctx().set_option('mode', _lib.MODE_STRICT if mode == 'strict' else _lib.MODE_FAST)
        FilmTable().set_size(32, 32)
        Camera().set_perspective(scenes.BENCH_CAMERA)
    return ModelPool()


def _rigged(pool, rec, case, seed):
    '''the mesh of a case: records rec with a random rig of the case's targets and joints, its skeleton and its clip.
    Returns (mesh, clip, rig)'''
    name, skel, T, tracks, binds, exact = case
    nj = len(skel[0]) if skel is not None else 0
    k = rec.shape[0] // 3
    dp, dn, jt, wt = deform_ref.random_rig(np.random.default_rng(seed), k, T, nj)
    mesh = pool.add_mesh(*deform_ref.split(rec))
    rig = dict(rec=rec, deltas=None, joints=None, weights=None)
    if T:
        pool.add_morph_targets(mesh, dp, dn)
        rig['deltas'] = np.ascontiguousarray(np.concatenate([dp.reshape(T, k * 3, 3), dn.reshape(T, k * 3, 3)], axis=2))
    if nj:
        pool.add_skin(mesh, jt, wt, nj)
        rig['joints'], rig['weights'] = jt.reshape(k * 3, 4), wt.reshape(k * 3, 4)
        parents, rest, ib = skel
        pool.add_skeleton(mesh, parents, rest[:, :3], rest[:, 3:7], rest[:, 7:], ib)
    return mesh, pool.add_clip(mesh, tracks), rig


def _mats4(pal):
    out = np.zeros((pal.shape[0], 4, 4))
    out[:, :3] = pal
    out[:, 3, 3] = 1.0
    return out


def _deformed(rig, w, pal):
    '''deform_ref's copy of the rig's mesh under the pose (w, pal)'''
    return deform_ref.deform(rig['rec'], rig['deltas'], w if rig['deltas'] is not None else None, rig['joints'], rig['weights'],
                             _mats4(pal) if rig['joints'] is not None else None)


def _fetch(pool, objs):
    return {o: (*pool.pose_to_numpy(o), pool.deformed_to_numpy(o)) for o in objs}


def _launches():
    return _ctx().timer('mpt_anim_kernel_time')[1], _ctx().timer('mpt_deform_kernel_time')[1]


# ---------------------------------------------------------------- the one scene of all cases, played once
@pytest.fixture(scope='module')
def played(gold):
    '''the scene built, composed at TIMES[0] and TIMES[1], composed again without a change, grown by an object, and one object
    unbound: what the device held each time, fetched.  The context is dropped at the end'''
    from ptina_amd.common import reset_all
    meshes, worlds = gold
    pool = _start()
    R = dict(rigs=[], clips=[], objs=[], bound=[])
    for i, case in enumerate(CASES):
        rec = meshes[i % len(meshes)]
        mesh, clip, rig = _rigged(pool, rec, case, 700 + i)
        R['rigs'].append(rig)
        R['clips'].append((mesh, clip))
        ids = []
        for b in case[4]:
            obj = pool.add_object(mesh, worlds[len(ids) % len(worlds)], i % 3)
            pool.set_animation(obj, clip, *b)
            ids.append(obj)
        R['objs'].append(ids)
        R['bound'] += ids
    five = NAMES.index('five joints, two roots')
    g = np.random.default_rng(77)
    mesh5 = R['clips'][five][0]
    hand = pool.add_object(mesh5, worlds[3], 1)                            # unbound, posed by hand, in the same compose
    R['hand_pose'] = (g.uniform(-1, 1.5, 3), deform_ref.random_joints(g, 5))
    pool.set_morph_weights(hand, R['hand_pose'][0])
    pool.set_joints(hand, R['hand_pose'][1])
    back = pool.add_object(mesh5, worlds[4], 2)                            # posed by hand, then bound: the clip's pose until it is unbound
    R['back_pose'] = (g.uniform(-1, 1.5, 3), deform_ref.random_joints(g, 5))
    pool.set_morph_weights(back, R['back_pose'][0])
    pool.set_joints(back, R['back_pose'][1])
    R['back_binding'] = (0.125, 0.75, False)
    pool.set_animation(back, R['clips'][five][1], *R['back_binding'])
    R['hand'], R['back'] = hand, back
    nbound = len(R['bound']) + 1
    _launches()
    R['frames'], R['counts'] = [], []
    for t in ar.TIMES:
        pool.set_time(t)
        pool.compose()
        R['counts'].append((*_launches(), pool.anim_stats().evaluated_objects, pool.deform_stats().deformed_objects, pool.anim_stats().bound_objects))
        R['frames'].append(_fetch(pool, R['bound'] + [hand, back]))
    R['nbound'] = nbound
    pool.set_time(ar.TIMES[1])                                             # the same time again: nothing to do
    pool.compose()
    R['idle'] = (*_launches(), pool.anim_stats().evaluated_objects, pool.deform_stats().deformed_objects)
    R['idle_frame'] = _fetch(pool, R['bound'][:3])
    # an object added behind the first composes: a relayout, the poses move and every bound object is evaluated again
    late = pool.add_object(R['clips'][0][0], worlds[5], 0)
    R['late'], R['late_binding'] = late, (0.3, 1.25, True)
    pool.set_animation(late, R['clips'][0][1], *R['late_binding'])
    pool.compose()
    R['grown'] = (*_launches(), pool.anim_stats().evaluated_objects, pool.deform_stats().deformed_objects)
    R['grown_frame'] = _fetch(pool, R['bound'] + [hand, back, late])
    # unbound again: the pose set by hand before the binding
    pool.set_animation(back, None)
    pool.compose()
    R['unbound'] = (*_launches(), pool.anim_stats().evaluated_objects, pool.deform_stats().deformed_objects, pool.anim_stats().bound_objects)
    R['unbound_frame'] = _fetch(pool, [back, hand])
    info = pool.anim_stats()
    R['info'] = (info.skeletons, info.clips, info.tracks)
    reset_all()
    return R


# ---------------------------------------------------------------- 1: the poses against the restatement
@pytest.mark.parametrize('name', NAMES)
def test_poses_equal_the_restatement(played, name):
    '''bit for bit off the theta branch, within the bound on it -- every binding of the case at both scene times'''
    i = NAMES.index(name)
    _, skel, T, tracks, binds, exact = CASES[i]
    thetas, worst = 0, 0.0
    for f, t in enumerate(ar.TIMES):
        for b, obj in zip(binds, played['objs'][i]):
            w, pal, _ = played['frames'][f][obj]
            theta, ratio = ar.check_pose((w, pal), skel, T, tracks, b, t, ar.ULP_TRIG_DEVICE, '%s %s t %g' % (name, b, t))
            assert not (exact and theta), 'a case that claims to be exact takes the theta branch'
            thetas += theta > 0
            worst = max(worst, ratio)
    print('%s: %d objects x %d times, %d on the theta branch, largest |device - restatement| / bound %.4f' % (name, len(binds), len(ar.TIMES), thetas, worst))
    assert exact or thetas >= len(binds), 'the theta case does not take the theta branch'
    if len(binds) > 1 and (tracks and skel is not None):
        a, b = (played['frames'][0][o][1] for o in played['objs'][i][:2])
        assert not ar.same_bits(a, b), 'two objects of one mesh on one clip at different offsets share a pose'


# ---------------------------------------------------------------- 2: the deformed copies given the fetched pose
def test_deformed_copies_follow_the_fetched_poses_bit_for_bit(played):
    n = 0
    for frame in played['frames'] + [played['grown_frame']]:
        for i, ids in enumerate(played['objs']):
            for obj in ids:
                w, pal, got = frame[obj]
                want = _deformed(played['rigs'][i], w, pal)
                bad = np.flatnonzero((got.view(u32) != want.view(u32)).any(axis=1))
                assert got.shape == want.shape and bad.size == 0, (NAMES[i], obj, bad[:8])
                n += want.shape[0] > 0
    assert n > 150


# ---------------------------------------------------------------- 3: launches, and the unbound object beside the bound ones
def test_one_launch_poses_every_bound_object_and_none_when_nothing_changed(played):
    nb = played['nbound']
    # at first everything is written: one anim launch for the bound objects, one deform launch for them and the two posed by hand
    assert played['counts'][0] == (1, 1, nb, nb + 1, nb)
    assert played['counts'][1] == (1, 1, nb, nb, nb), 'set_time marks the bound objects alone'
    assert played['idle'] == (0, 0, 0, 0), 'the same time again: nothing is launched'
    for obj, (w, pal, rec) in played['idle_frame'].items():
        assert ar.same_bits(pal, played['frames'][1][obj][1]) and _same(rec, played['frames'][1][obj][2])
    assert played['grown'] == (1, 1, nb + 1, nb + 2), 'a relayout evaluates every bound object again and deforms every deformable one'
    assert played['info'][:2] == (sum(c[1] is not None for c in CASES), len(CASES)) and played['info'][2] == sum(len(c[3]) for c in CASES)


def test_the_unbound_object_keeps_the_pose_set_by_hand(played):
    five = NAMES.index('five joints, two roots')
    rig = played['rigs'][five]
    hw, hm = played['hand_pose']
    for frame in played['frames'] + [played['grown_frame'], played['unbound_frame']]:
        w, pal, rec = frame[played['hand']]
        assert ar.same_bits(w, hw) and ar.same_bits(pal, hm[:, :3]) and _same(rec, _deformed(rig, hw, hm[:, :3]))


def test_relayout_evaluates_again_where_the_poses_moved(played):
    '''the poses lie elsewhere after the relayout and hold the same bits; the late object has its own'''
    for obj in played['bound']:
        assert ar.same_bits(played['grown_frame'][obj][1], played['frames'][1][obj][1]) and ar.same_bits(played['grown_frame'][obj][0], played['frames'][1][obj][0])
    _, skel, T, tracks, _, _ = CASES[0]
    w, pal, _ = played['grown_frame'][played['late']]
    ar.check_pose((w, pal), skel, T, tracks, played['late_binding'], ar.TIMES[1], ar.ULP_TRIG_DEVICE, 'the late object')


def test_unbinding_returns_the_pose_set_by_hand(played):
    five = NAMES.index('five joints, two roots')
    _, skel, T, tracks, _, _ = CASES[five]
    back = played['back']
    for f, t in enumerate(ar.TIMES):                                       # bound: the clip's pose, not the one set by hand before
        w, pal, rec = played['frames'][f][back]
        assert ar.check_pose((w, pal), skel, T, tracks, played['back_binding'], t, ar.ULP_TRIG_DEVICE, 'bound behind set_joints')[0] == 0
    bw, bm = played['back_pose']
    w, pal, rec = played['unbound_frame'][back]
    assert ar.same_bits(w, bw) and ar.same_bits(pal, bm[:, :3]) and _same(rec, _deformed(played['rigs'][five], bw, bm[:, :3]))
    assert played['unbound'] == (0, 1, 0, 1, played['nbound']), 'the unbound pose goes up as ever: no anim launch, one object deformed'


# ---------------------------------------------------------------- 4: the device's acos and sin
def test_device_trig_stays_within_its_measured_error(fresh):
    '''the device library's f64 acos and sin over the arguments the theta cases hand them (mpt_anim_trig), against np.longdouble:
    half of ULP_TRIG_DEVICE covers the largest error seen (the constant is twice that, rounded up)'''
    _start()

    def walk():
        for name, skel, T, tracks, binds, exact in CASES:
            if not exact:
                for b in binds:
                    for t in ar.TIMES:
                        ar.pose(skel, T, tracks, b, t)
    args = ar.record_trig(walk)
    assert args['acos'].size >= 20
    dp = C.POINTER(C.c_double)
    worst = {}
    for name in ('acos', 'sin'):
        x = np.ascontiguousarray(args[name])
        a, s = np.empty_like(x), np.empty_like(x)
        _ctx().call('mpt_anim_trig', x.ctypes.data_as(dp), int(x.size), a.ctypes.data_as(dp), s.ctypes.data_as(dp))
        worst[name] = float(ar.trig_ulps(x, a if name == 'acos' else s, name).max())
    print('device library over %d + %d arguments: acos within %.4f ulp, sin within %.4f ulp' % (args['acos'].size, args['sin'].size, worst['acos'], worst['sin']))
    assert 2 * max(worst.values()) <= ar.ULP_TRIG_DEVICE


# ---------------------------------------------------------------- 5: the stack behind the pose
def test_subdivision_and_sticky_scatter_follow_the_clip_as_they_follow_set_joints(fresh):
    '''a bound skinned, morphed surface with a subdivision level and a sticky scatter on it: after set_time + compose the model
    equals, word for word, the same scene posed through set_joints(fetched palette) + set_morph_weights(fetched weights)'''
    import subdiv_ref as sr
    case = CASES[NAMES.index('five joints, two roots')]
    surface, tuft = sr.fixture('cylinder'), sr.fixture('tetrahedron')
    world = np.eye(4)
    world[:3, 3] = [0.2, -0.1, 0.4]

    def scene(bound, first=None):
        pool = _start()
        name, skel, T, tracks, binds, exact = case
        nj = len(skel[0])
        k = surface.shape[0] // 3
        dp, dn, jt, wt = deform_ref.random_rig(np.random.default_rng(9), k, T, nj)
        mesh = pool.add_mesh(*deform_ref.split(surface))
        pool.add_morph_targets(mesh, 0.3 * dp, dn)
        pool.add_skin(mesh, jt, wt, nj)
        pool.add_skeleton(mesh, skel[0], skel[1][:, :3], skel[1][:, 3:7], skel[1][:, 7:], skel[2])
        clip = pool.add_clip(mesh, tracks)
        pool.add_subdivision(mesh, 1)
        surf = pool.add_object(mesh, world, 1)
        sid, objs = pool.add_scatter(surf, pool.add_mesh(*deform_ref.split(tuft)), 65, seed=4, mtlid=2, scale=(0.03, 0.08))
        if bound:
            pool.set_animation(surf, clip, 0.25, 1.5, True)
        else:                                                              # (the scatter chooses its faces on the surface as first composed)
            pool.set_morph_weights(surf, first[0])
            pool.set_joints(surf, _mats4(first[1]))
        pool.compose()
        return pool, surf
    pool, surf = scene(True)
    at_first = pool.to_numpy()[0]
    first = pool.pose_to_numpy(surf)
    poses, models = [], []
    for t in (0.4, 1.3):
        pool.set_time(t)
        pool.compose()
        assert pool.anim_stats().evaluated_objects == 1 and pool.subdiv_stats().refined_copies == 1 and pool.scatter_stats().placed_scatters == 1
        poses.append(pool.pose_to_numpy(surf))
        models.append(pool.to_numpy())
    assert not _same(models[0][0], at_first) and not _same(models[0][0], models[1][0])
    pool, surf = scene(False, first)
    assert _same(pool.to_numpy()[0], at_first)
    for (w, pal), (verts, mtl) in zip(poses, models):
        pool.set_morph_weights(surf, w)
        pool.set_joints(surf, _mats4(pal))
        pool.compose()
        assert pool.anim_stats().evaluated_objects == 0
        got, got_m = pool.to_numpy()
        assert _same(got, verts) and np.array_equal(got_m, mtl)


# ---------------------------------------------------------------- 6: build, set_time, compose, update
@pytest.fixture(scope='module')
def gold_scene():
    '''the fixture's nine objects as the deform tests lay them out: (meshes in file order, [(mesh, world, material)])'''
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_compose.npz'))
    meshes = [deform_ref.records(g['mesh%d_p' % i], g['mesh%d_n' % i], g['mesh%d_t' % i]) for i in range(int(g['nmeshes']))]
    objs = [(int(m), np.array(g['obj_world'][o], np.float64), None if g['obj_mtl_none'][o] else int(g['obj_mtl'][o])) for o, m in enumerate(g['obj_mesh'])]
    return meshes, objs


def _gentle_case():
    '''a chain of five joints that rests at the identity and a clip that moves it about as far as deform_ref.random_joints does, so
    that the scene stays the one the deform tests query'''
    from ptina_amd.tools.anim import quaternion
    g = np.random.default_rng(31)
    rest = np.tile([0, 0, 0, 0, 0, 0, 1, 1, 1, 1.0], (5, 1))
    skel = (np.arange(5) - 1, rest, np.tile(np.eye(4)[:3], (5, 1, 1)))
    times = [0.0, 0.5, 1.0, 2.0]
    tracks = []
    for j in range(5):
        tracks.append(ar.track(j, 'T', times, g.uniform(-0.03, 0.03, (4, 3))))
        tracks.append(ar.track(j, 'R', times, [quaternion(g.normal(size=3), g.uniform(-0.1, 0.1)) for _ in times]))
        tracks.append(ar.track(j, 'S', times, g.uniform(0.97, 1.03, (4, 3)), 'STEP' if j % 2 else 'LINEAR'))
    tracks.append(ar.track(None, 'W', times, g.uniform(-0.5, 1.0, (4, 3, 3)), 'CUBICSPLINE'))
    return ('gentle chain', skel, 3, tracks, None, True)


@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_set_time_then_refit(fresh, gold_scene, mode):
    import query_ref as qr
    import refit_ref
    import visibility_ref as vr
    from test_refit_gpu import _records, _same_records
    from ptina_amd.things import BVHTree
    meshes, objs = gold_scene
    pool = _start(mode)
    case = _gentle_case()
    rigged = [_rigged(pool, rec, case, 40 + i) for i, rec in enumerate(meshes)]
    ids = [pool.add_object(rigged[m][0], world, mtl) for m, world, mtl in objs]
    pool.compose()                                                         # every object at rest: identity joints, zero weights
    tree = BVHTree()
    tree.build()
    built = _records(_ctx())
    before = pool.to_numpy()[0]
    for o, b in ((2, (0.0, 1.0, True)), (5, (0.6, -0.5, True)), (8, (0.1, 2.0, False))):
        pool.set_animation(ids[o], rigged[objs[o][0]][1], *b)
    pool.set_time(0.35)
    pool.compose()
    assert pool.anim_stats().evaluated_objects == 3 and pool.deform_stats().deformed_objects == 3
    assert tree.update() == 'refit' and tree.refit_stats().host_fetches == 0
    got = _records(_ctx())
    model, _ = pool.to_numpy()
    assert not _same(model, before)
    pos = vr.positions(model)
    n = pos.shape[0]
    bmin, bmax, w, q = refit_ref.refit_ref(built['child'], built['leaf'], built['wnode'], built['qnode'], n, pos)
    _same_records(got, dict(built, bmin=bmin, bmax=bmax, wnode=w, qnode=q), 'refit after set_time (%s)' % mode)
    first = np.concatenate([[0], np.cumsum([meshes[m].shape[0] // 3 for m, _, _ in objs])])[:9]
    o, d = qr.rays(pos, 4, 512)
    ref = qr.classify(pos, o, d)
    dec = ref['decided']
    assert dec.mean() >= 0.9 and (dec & ref['hit']).any() and (dec & ~ref['hit']).any()
    bad = qr.errors(ref, tree.intersect(o, d), 'animated %s' % mode, first=first)
    assert not bad, bad[:4]


# ---------------------------------------------------------------- 7: refusals, clearing, a pool that is replaced
def test_refusals_name_their_argument(fresh, gold):
    meshes, worlds = gold
    pool = _start()
    tk = ar.track
    name, skel, T, tracks, binds, exact = CASES[NAMES.index('five joints, two roots')]
    parents, rest, ib = skel
    rec = meshes[3]
    k = rec.shape[0] // 3
    dp, dn, jt, wt = deform_ref.random_rig(np.random.default_rng(1), k, 3, 5)
    plain = pool.add_mesh(*deform_ref.split(rec))
    mesh = pool.add_mesh(*deform_ref.split(rec))
    morph = pool.add_mesh(*deform_ref.split(rec))
    pool.add_morph_targets(morph, dp, dn)
    sk = (rest[:, :3], rest[:, 3:7], rest[:, 7:], ib)
    with pytest.raises(RuntimeError, match='mesh %d has no skin' % mesh):
        pool.add_skeleton(mesh, parents, *sk)
    with pytest.raises(RuntimeError, match='neither morph targets nor a skin'):
        pool.add_clip(plain, [])
    pool.add_skin(mesh, jt, wt, 5)
    with pytest.raises(RuntimeError, match='a skin and no skeleton'):
        pool.add_clip(mesh, tracks[:1])
    with pytest.raises(RuntimeError, match='njoints 4, the skin of mesh %d has 5 joints' % mesh):
        pool.add_skeleton(mesh, parents[:4], rest[:4, :3], rest[:4, 3:7], rest[:4, 7:], ib[:4])
    with pytest.raises(RuntimeError, match=r'parents\[1\] is 1: parents come before their children'):
        pool.add_skeleton(mesh, [-1, 1, 0, 1, 2], *sk)
    bad = rest.copy()
    bad[2, 3:7] = 0
    with pytest.raises(RuntimeError, match=r'rest rotation rest\[2\]\[3..6\] is zero'):
        pool.add_skeleton(mesh, parents, bad[:, :3], bad[:, 3:7], bad[:, 7:], ib)
    with pytest.raises(ValueError, match='not affine'):
        pool.add_skeleton(mesh, parents, *sk[:3], np.ones((5, 4, 4)))
    pool.add_skeleton(mesh, parents, *sk)
    with pytest.raises(RuntimeError, match='already has a skeleton'):
        pool.add_skeleton(mesh, parents, *sk)
    for tr, words in (([tk(0, 'T', [0, np.inf], np.zeros((2, 3)))], r'times\[1\] of tracks\[0\] is not finite'),
                      ([tk(0, 'T', [1, 0.5], np.zeros((2, 3)))], r'times\[1\] of tracks\[0\] is not above the key before'),
                      ([tk(5, 'S', [0], np.ones((1, 3)))], r'tracks\[0\] names joint 5, beyond njoints 5'),
                      ([tk(None, 'W', [0], np.ones((1, 3)))], 'morph weights of a mesh without morph targets'),
                      ([tk(1, 'R', [0], [[0, 0, 0, 1]]), tk(1, 'R', [0, 1], [[0, 0, 0, 1], [1, 0, 0, 0]])], r'tracks\[0\] and tracks\[1\] animate the same target and path'),
                      ([tk(1, 'R', [0, 1], [[0, 0, 0, 1], [0, 0, 0, 0]])], r'rotation values of key 1 of tracks\[0\] are zero')):
        with pytest.raises(RuntimeError, match='mpt_mesh_add_clip: clip: .*' + words):
            pool.add_clip(mesh, tr)
    with pytest.raises(RuntimeError, match=r'tracks\[0\] names joint 0, beyond njoints 0'):
        pool.add_clip(morph, [tk(0, 'T', [0], np.zeros((1, 3)))])
    clip = pool.add_clip(mesh, [t for t in tracks if t.path != 3])
    wclip = pool.add_clip(morph, [t for t in tracks if t.path == 3])
    assert (clip, wclip) == (0, 1) and pool.anim_stats().clips == 2
    obj = pool.add_object(mesh, worlds[0], 0)
    mobj = pool.add_object(morph, worlds[1], 0)
    still = pool.add_object(plain, worlds[2], 0)
    with pytest.raises(ValueError, match='already has an object'):
        pool.add_clip(mesh, tracks[:1])
    with pytest.raises(ValueError, match='already has an object'):
        pool.add_skeleton(mesh, parents, *sk)
    dp_ = C.POINTER(C.c_double)
    with pytest.raises(RuntimeError, match='mpt_mesh_add_clip: mesh %d already has an object' % mesh):
        _ctx().call('mpt_mesh_add_clip', mesh, 0, None, None, 0, None, 0, C.byref(C.c_int(0)))
    with pytest.raises(RuntimeError, match='mpt_mesh_set_skeleton: mesh %d already has an object' % mesh):
        _ctx().call('mpt_mesh_set_skeleton', mesh, 5, None, None, None)
    with pytest.raises(RuntimeError, match='clip 1 is a clip of mesh %d, object %d an object of mesh %d' % (morph, obj, mesh)):
        pool.set_animation(obj, wclip)
    with pytest.raises(RuntimeError, match=r'unknown clip 2 \(2 clips\)'):
        pool.set_animation(obj, 2)
    with pytest.raises(RuntimeError, match='object %d has neither morph targets nor a skin' % still):
        pool.set_animation(still, clip)
    with pytest.raises(ValueError, match='unknown object'):
        pool.set_animation(99, clip)
    for kw, words in ((dict(offset=np.nan), 'offset is not finite'), (dict(speed=np.inf), 'speed is not finite')):
        with pytest.raises(RuntimeError, match=words):
            pool.set_animation(obj, clip, **kw)
    with pytest.raises(RuntimeError, match='t is not finite'):
        pool.set_time(np.nan)
    with pytest.raises(RuntimeError, match='no pose on the device yet'):
        pool.pose_to_numpy(obj)
    pool.set_animation(obj, clip)
    pool.set_animation(mobj, wclip, 0.5)
    with pytest.raises(RuntimeError, match='mpt_object_set_joints: object %d is bound to clip 0.*unbind it first' % obj):
        pool.set_joints(obj, np.tile(np.eye(4), (5, 1, 1)))
    with pytest.raises(RuntimeError, match='mpt_object_set_morph_weights: object %d is bound to clip 1.*unbind it first' % mobj):
        pool.set_morph_weights(mobj, [0, 0, 0])
    pool.set_time(0.8)
    pool.compose()
    s = pool.anim_stats()
    assert (s.skeletons, s.clips, s.bound_objects, s.evaluated_objects) == (1, 2, 2, 2)
    with pytest.raises(RuntimeError, match='neither morph targets nor a skin'):
        pool.pose_to_numpy(still)
    w, pal = pool.pose_to_numpy(mobj)                                      # a morph-only mesh: weights and an empty palette
    assert pal.shape == (0, 3, 4) and ar.same_bits(w, ar.pose(None, 3, [t for t in tracks if t.path == 3], (0.5, 1.0, True), 0.8)[0])
    # clear_objects drops the bindings and keeps the clips; clear_meshes drops both; a new pool starts empty and works
    pool.clear_objects()
    s = pool.anim_stats()
    assert (s.skeletons, s.clips, s.bound_objects) == (1, 2, 0)
    obj = pool.add_object(mesh, worlds[0], 0)
    pool.set_animation(obj, clip, 0.1)
    pool.compose()
    assert pool.anim_stats().evaluated_objects == 1
    kept = pool.pose_to_numpy(obj)
    ar.check_pose(kept, skel, 0, [t for t in tracks if t.path != 3], (0.1, 1.0, True), 0.8, ar.ULP_TRIG_DEVICE, 'after clear_objects')
    pool.clear_meshes()
    s = pool.anim_stats()
    assert (s.skeletons, s.clips, s.tracks, s.bound_objects) == (0, 0, 0, 0)
    pool = _start()
    assert pool.anim_stats().clips == 0
    mesh, clip, _ = _rigged(pool, rec, CASES[NAMES.index('five joints, two roots')], 1)
    obj = pool.add_object(mesh, worlds[0], 0)
    pool.set_animation(obj, clip, 0.1)
    pool.set_time(0.8)
    pool.compose()
    w, pal = pool.pose_to_numpy(obj)
    assert ar.same_bits(pal, kept[1]), 'a new pool evaluates the same skeleton and tracks to the same palette'


def test_worker_facade_through_the_thread_proxy(fresh, gold):
    import threading
    from ptina_amd.common import reset_all
    from ptina_amd.tools.mtworker import DaemonModule, OnDemandProxy
    meshes, worlds = gold
    case = CASES[NAMES.index('five joints, two roots')]
    name, skel, T, tracks, binds, exact = case
    pool = _start()
    mesh, clip, _ = _rigged(pool, meshes[2], case, 5)
    obj = pool.add_object(mesh, worlds[0], 0)
    pool.set_animation(obj, clip, 0.3, -1.25, True)
    pool.set_time(1.1)
    pool.compose()
    direct_v, direct_m = pool.to_numpy()
    direct_pose = pool.pose_to_numpy(obj)
    reset_all()
    seen = []

    def module():
        seen.append(threading.get_ident())
        from ptina_amd import worker
        ns = types.SimpleNamespace(**{k: getattr(worker, k) for k in dir(worker) if not k.startswith('_')})

        def rig():
            p = worker.ModelPool()
            k = meshes[2].shape[0] // 3
            dp, dn, jt, wt = deform_ref.random_rig(np.random.default_rng(5), k, T, 5)
            m = p.add_mesh(*deform_ref.split(meshes[2]))
            p.add_morph_targets(m, dp, dn)
            p.add_skin(m, jt, wt, 5)
            return m
        ns.rig = rig
        ns.add = lambda m: worker.ModelPool().add_object(m, worlds[0], 0)
        ns.fetch = lambda: worker.ModelPool().to_numpy()
        ns.pose = lambda o: worker.ModelPool().pose_to_numpy(o)
        return ns
    w = OnDemandProxy(lambda: DaemonModule(module))
    w.init()
    m = w.rig()
    w.set_mesh_skeleton(m, skel[0], skel[1][:, :3], skel[1][:, 3:7], rest_scale=skel[1][:, 7:], inverse_bind=skel[2])
    c = w.add_mesh_clip(mesh=m, tracks=tracks)
    o = w.add(m)
    w.set_object_animation(o, c, offset=0.3, speed=-1.25)
    w.set_scene_time(t=1.1)
    w.compose_model()
    assert seen and seen[0] != threading.get_ident()
    got_v, got_m = w.fetch()
    assert _same(got_v, direct_v) and np.array_equal(got_m, direct_m)
    gw, gp = w.pose(o)
    assert ar.same_bits(gw, direct_pose[0]) and ar.same_bits(gp, direct_pose[1])
    w.synchronize()

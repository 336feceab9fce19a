'''
GPU tests (-m gpu) of two blended clips and of objects moved by clips (ModelPool.set_animation_blend / add_object_clip / set_motion /
world_to_numpy / anim_blend_stats; anim.hip's blend path and motion_kernel, scene_anim.cpp).

The kernels are held to tests/anim_blend_ref.py: BIT FOR BIT for every object whose rotation tracks stay out of the slerp's theta
branch, within the first-order bound with the device library's measured error (anim_ref.ULP_TRIG_DEVICE) for the others.  Deformed
copies are held to tests/deform_ref.py fed the FETCHED palette, composed models to a twin scene fed the FETCHED matrices, word for
word, so that the feature's only tolerance stays in one place.  All cases are ONE scene of the meshes of
tests/golden/reference_compose.npz: an object per binding, blended and moved ones side by side, so that one anim launch and one
motion launch serve objects of different rigs and clips.
'''

import types

import numpy as np
import pytest

import anim_ref as ar
import anim_blend_ref as br
import deform_ref
from test_anim_gpu import _same, _ctx, _start, _rigged, _mats4, _deformed, _gentle_case, gold, gold_scene      # noqa: F401  (gold, gold_scene: fixtures)

pytestmark = pytest.mark.gpu
u32 = np.uint32
BCASES = br.blend_cases()
MCASES = br.motion_cases()
BNAMES = [c[0] for c in BCASES]
MNAMES = [c[0] for c in MCASES]
DEV = ar.ULP_TRIG_DEVICE


def _rigged2(pool, rec, case, seed):
    '''the mesh of a blend case with its rig, skeleton and both clips: (mesh, clip A, clip B, rig)'''
    name, skel, T, a, b = case[:5]
    mesh, clip_a, rig = _rigged(pool, rec, (name, skel, T, a, None, None), seed)
    return mesh, clip_a, pool.add_clip(mesh, b), rig


def _bind2(pool, obj, clip_a, clip_b, ba, bb, fade):
    pool.set_animation(obj, clip_a, *ba)
    pool.set_animation_blend(obj, clip_b, *bb, weight=fade[:2], fade=fade[2:])


def _launches():
    return _ctx().timer('mpt_anim_kernel_time')[1], _ctx().timer('mpt_motion_kernel_time')[1]


def _counts(pool):
    s = pool.anim_blend_stats()
    return (*_launches(), pool.anim_stats().evaluated_objects, s.evaluated_blended, s.evaluated_moved)


# ---------------------------------------------------------------- the one scene of all cases, played once
@pytest.fixture(scope='module')
def played(gold):      # noqa: F811
    from ptina_amd.common import reset_all
    meshes, worlds = gold
    pool = _start()
    R = dict(rigs=[], bobjs=[], mobjs=[], blended=[], moved=[], set_world={})
    clips = []
    for i, case in enumerate(BCASES):
        mesh, ca, cb, rig = _rigged2(pool, meshes[i % len(meshes)], case, 900 + i)
        R['rigs'].append(rig)
        clips.append((mesh, ca, cb))
    plain = [pool.add_mesh(*deform_ref.split(meshes[k])) for k in (2, 3, 5)]       # rigid meshes of 85, 22 and 1 faces
    oclips = [pool.add_object_clip(c[1]) for c in MCASES]
    for i, case in enumerate(BCASES):
        ids = []
        for ba, bb, fade in case[5]:
            obj = pool.add_object(clips[i][0], worlds[len(ids) % len(worlds)], i % 3)
            _bind2(pool, obj, clips[i][1], clips[i][2], ba, bb, fade)
            ids.append(obj)
        R['bobjs'].append(ids)
        R['blended'] += ids
    for i, case in enumerate(MCASES):
        ids = []
        for b in case[4]:
            obj = pool.add_object(plain[len(ids) % 3], worlds[(i + len(ids)) % len(worlds)], (i + 1) % 3)
            pool.set_motion(obj, oclips[i], *b, rest=case[2], base=case[3])
            R['set_world'][obj] = worlds[(i + len(ids)) % len(worlds)]
            ids.append(obj)
        R['mobjs'].append(ids)
        R['moved'] += ids
    # a finished fade beside the same mesh bound to B alone with B's binding; an object posed by hand, then bound twice, then unbound
    three = BNAMES.index('three joints, disjoint')
    mesh3, ca3, cb3 = clips[three]
    R['bb'] = (0.25, 1.5, True)
    R['faded'] = pool.add_object(mesh3, worlds[1], 0)
    _bind2(pool, R['faded'], ca3, cb3, (0.0, 1.0, True), R['bb'], (0.3, 1.0, -3.0, 1.0))
    R['b_alone'] = pool.add_object(mesh3, worlds[1], 0)
    pool.set_animation(R['b_alone'], cb3, *R['bb'])
    g = np.random.default_rng(78)
    R['hand_pose'] = (g.uniform(-1, 1.5, 3), deform_ref.random_joints(g, 3))
    R['back'] = pool.add_object(mesh3, worlds[2], 1)
    pool.set_morph_weights(R['back'], R['hand_pose'][0])
    pool.set_joints(R['back'], R['hand_pose'][1])
    R['back_bind'] = ((0.125, 0.75, False), (0.5, -1.5, True), (0.25, 0.75, 0.5, 2.0))
    _bind2(pool, R['back'], ca3, cb3, *R['back_bind'])
    # a deformable, blended object that also moves; a rigid object that stays where set_world put it
    R['both'] = pool.add_object(mesh3, worlds[3], 2)
    _bind2(pool, R['both'], ca3, cb3, (0.0, 1.0, True), R['bb'], (0.5, 0.5, 0.0, 0.0))
    R['both_motion'] = (MNAMES.index('T R S, CUBICSPLINE and STEP'), (0.5, -1.5, True))
    pool.set_motion(R['both'], oclips[R['both_motion'][0]], *R['both_motion'][1], rest=MCASES[R['both_motion'][0]][2], base=MCASES[R['both_motion'][0]][3])
    R['still'] = pool.add_object(plain[1], worlds[4], 0)
    R['set_world'][R['still']] = worlds[4]
    posed = R['blended'] + [R['faded'], R['b_alone'], R['back'], R['both']]
    placed = R['moved'] + [R['both'], R['still']]
    R['nblended'], R['nmoved'], R['nposed'] = len(R['blended']) + 3, len(R['moved']) + 1, len(posed)

    def fetch():
        return dict(pose={o: pool.pose_to_numpy(o) for o in posed}, copy={o: pool.deformed_to_numpy(o) for o in posed},
                    world={o: pool.world_to_numpy(o) for o in placed})
    _launches()
    R['frames'], R['counts'] = [], []
    for t in br.TIMES:
        pool.set_time(t)
        pool.compose()
        R['counts'].append(_counts(pool))
        R['frames'].append(fetch())
    s = pool.anim_blend_stats()
    R['info'] = (s.object_clips, s.blended_objects, s.moved_objects, pool.anim_stats().clips)
    pool.set_time(br.TIMES[1])                                             # the same time again: nothing to do
    pool.compose()
    R['idle'] = _counts(pool)
    R['idle_frame'] = fetch()
    # a material: the row goes up with the host's matrix, and the object is evaluated again
    R['painted'] = R['mobjs'][1][0]
    pool.set_material(R['painted'], 2)
    pool.compose()
    R['paint'] = _counts(pool)
    R['paint_world'] = pool.world_to_numpy(R['painted'])
    # an object added behind the first composes: a relayout, the whole table goes up and every moved object is evaluated again
    R['late'], R['late_bind'] = pool.add_object(plain[2], worlds[5], 0), (0.3, 1.25, True)
    pool.set_motion(R['late'], oclips[1], *R['late_bind'], rest=MCASES[1][2], base=MCASES[1][3])
    pool.compose()
    R['grown'] = _counts(pool)
    R['grown_frame'] = fetch()
    R['late_world'] = pool.world_to_numpy(R['late'])
    # unbound: the second binding alone (A's pose), both (the hand-set pose), the motion (set_world's matrix); set_world works again
    pool.set_animation_blend(R['both'], None)
    pool.set_animation(R['back'], None)
    R['freed'] = R['mobjs'][0][0]
    pool.set_motion(R['freed'], None)
    pool.compose()
    R['unbound'] = _counts(pool)
    R['unbound_frame'] = dict(both=pool.pose_to_numpy(R['both']), back=pool.pose_to_numpy(R['back']), back_copy=pool.deformed_to_numpy(R['back']),
                              freed=pool.world_to_numpy(R['freed']))
    s = pool.anim_blend_stats()
    R['unbound_info'] = (s.blended_objects, s.moved_objects)
    R['elsewhere'] = np.array(worlds[6], np.float64)
    pool.set_world(R['freed'], R['elsewhere'])
    pool.compose()
    R['moved_by_hand'] = pool.world_to_numpy(R['freed'])
    reset_all()
    return R


# ---------------------------------------------------------------- 1: poses and matrices against the restatement
@pytest.mark.parametrize('name', BNAMES)
def test_blended_poses_equal_the_restatement(played, name):
    i = BNAMES.index(name)
    _, skel, T, a, b, objs, exact = BCASES[i]
    thetas, worst = 0, 0.0
    br.undecided[0] = 0
    for f, t in enumerate(br.TIMES):
        for (ba, bb, fade), obj in zip(objs, played['bobjs'][i]):
            theta, ratio = br.check_blend(played['frames'][f]['pose'][obj], skel, T, a, ba, b, bb, fade, t, DEV, '%s %s %s %s t %g' % (name, ba, bb, fade, t))
            assert not (exact and theta), 'a case that claims to be exact takes the theta branch'
            thetas += theta > 0
            worst = max(worst, ratio)
    print('%s: %d objects x %d times, %d on the theta branch, largest |device - restatement| / bound %.4f' % (name, len(objs), len(br.TIMES), thetas, worst))
    assert br.undecided[0] == 0
    assert exact or thetas >= len(objs), 'the theta case does not take the theta branch'


@pytest.mark.parametrize('name', MNAMES)
def test_moved_worlds_equal_the_restatement(played, name):
    i = MNAMES.index(name)
    _, tracks, rest, base, binds, exact = MCASES[i]
    thetas, worst = 0, 0.0
    for f, t in enumerate(br.TIMES):
        for b, obj in zip(binds, played['mobjs'][i]):
            theta, ratio = br.check_world(played['frames'][f]['world'][obj], tracks, b, rest, base, t, DEV, '%s %s t %g' % (name, b, t))
            assert not (exact and theta)
            thetas += theta > 0
            worst = max(worst, ratio)
    print('%s: %d objects x %d times, %d on the theta branch, largest |device - restatement| / bound %.4f' % (name, len(binds), len(br.TIMES), thetas, worst))
    assert exact or thetas >= len(binds) // 2


def test_an_object_may_be_blended_and_moved_and_a_rigid_one_left_alone(played):
    three = BNAMES.index('three joints, disjoint')
    _, skel, T, a, b = BCASES[three][:5]
    k, bind = played['both_motion']
    for f, t in enumerate(br.TIMES):
        fr = played['frames'][f]
        assert br.check_blend(fr['pose'][played['both']], skel, T, a, (0.0, 1.0, True), b, played['bb'], (0.5, 0.5, 0.0, 0.0), t, DEV, 'blended and moved')[0] == 0
        assert br.check_world(fr['world'][played['both']], MCASES[k][1], bind, MCASES[k][2], MCASES[k][3], t, DEV, 'blended and moved')[0] == 0
        assert br.same_bits(fr['world'][played['still']], played['set_world'][played['still']])


def test_deformed_copies_follow_the_fetched_poses_bit_for_bit(played):
    n = 0
    three = BNAMES.index('three joints, disjoint')
    for frame in played['frames'] + [played['grown_frame']]:
        for i, ids in enumerate(played['bobjs']):
            for obj in ids + ([played['faded'], played['b_alone'], played['back'], played['both']] if i == three else []):
                w, pal = frame['pose'][obj]
                got, want = frame['copy'][obj], _deformed(played['rigs'][i], w, pal)
                bad = np.flatnonzero((got.view(u32) != want.view(u32)).any(axis=1))
                assert got.shape == want.shape and bad.size == 0, (BNAMES[i], obj, bad[:8])
                n += want.shape[0] > 0
    assert n > 100


def test_a_finished_fade_is_clip_b_alone_word_for_word(played):
    for frame in played['frames']:
        for k in range(2):
            assert br.same_bits(frame['pose'][played['faded']][k], frame['pose'][played['b_alone']][k])
        assert _same(frame['copy'][played['faded']], frame['copy'][played['b_alone']])
    assert not br.same_bits(played['frames'][0]['pose'][played['faded']][1], played['frames'][1]['pose'][played['faded']][1])


# ---------------------------------------------------------------- 2: launches, marking, relayout, unbinding
def test_one_anim_launch_and_one_motion_launch_per_compose_and_none_when_nothing_changed(played):
    nb, nm, nposed = played['nblended'], played['nmoved'], played['nposed']
    bound = nposed                                                        # every deformable object of the scene is bound
    assert played['counts'][0] == (1, 1, bound, nb, nm)
    assert played['counts'][1] == (1, 1, bound, nb, nm), 'set_time marks the bound and the moved objects'
    assert played['idle'] == (0, 0, 0, 0, 0), 'the same time again: nothing is launched'
    for o, w in played['idle_frame']['world'].items():
        assert br.same_bits(w, played['frames'][1]['world'][o])
    assert played['info'] == (len(MCASES), nb, nm, 2 * len(BCASES) + len(MCASES))


def test_a_row_that_goes_up_for_another_reason_is_evaluated_again(played):
    assert played['paint'] == (0, 1, 0, 0, 1), 'set_material uploads the row with the host\'s matrix: the object alone is moved again'
    assert br.same_bits(played['paint_world'], played['frames'][1]['world'][played['painted']])
    assert not br.same_bits(played['paint_world'], played['set_world'][played['painted']])


def test_relayout_evaluates_every_moved_object_again(played):
    nb, nm, nposed = played['nblended'], played['nmoved'], played['nposed']
    assert played['grown'] == (1, 1, nposed, nb, nm + 1)
    for o, w in played['grown_frame']['world'].items():
        assert br.same_bits(w, played['frames'][1]['world'][o])
    for o, p in played['grown_frame']['pose'].items():
        assert br.same_bits(p[0], played['frames'][1]['pose'][o][0]) and br.same_bits(p[1], played['frames'][1]['pose'][o][1])
    br.check_world(played['late_world'], MCASES[1][1], played['late_bind'], MCASES[1][2], MCASES[1][3], br.TIMES[1], DEV, 'the late object')


def test_unbinding_returns_what_was_set_by_hand(played):
    three = BNAMES.index('three joints, disjoint')
    _, skel, T, a, b = BCASES[three][:5]
    ba, bb, fade = played['back_bind']
    for f, t in enumerate(br.TIMES):                                       # bound twice: the blend, not the pose set by hand before
        br.check_blend(played['frames'][f]['pose'][played['back']], skel, T, a, ba, b, bb, fade, t, DEV, 'bound behind set_joints')
    u = played['unbound_frame']
    hw, hm = played['hand_pose']
    assert br.same_bits(u['back'][0], hw) and br.same_bits(u['back'][1], hm[:, :3]) and _same(u['back_copy'], _deformed(played['rigs'][three], hw, hm[:, :3]))
    w, pal, theta = ar.pose(skel, T, a, (0.0, 1.0, True), br.TIMES[1])     # the second binding removed: clip A alone
    assert theta == 0 and br.same_bits(u['both'][0], w) and br.same_bits(u['both'][1], pal)
    assert br.same_bits(u['freed'], played['set_world'][played['freed']]), 'unbound: the matrix add_object gave'
    # one object posed again, by clip A alone; its row goes up for that, and as it is moved too, its matrix is evaluated again
    assert played['unbound'] == (1, 1, 1, 0, 1)
    assert played['unbound_info'] == (played['nblended'] - 2, played['nmoved'] + 1 - 1)      # (the late object came, the freed one went)
    assert br.same_bits(played['moved_by_hand'], played['elsewhere'])


# ---------------------------------------------------------------- 3: 1, 64, 65 and 257 moved objects in one launch
def test_motion_launches_across_a_wave_and_a_workgroup(fresh, gold):      # noqa: F811
    meshes, worlds = gold
    pool = _start()
    one = pool.add_mesh(*deform_ref.split(meshes[5]))
    assert meshes[5].shape[0] == 3
    clips = [(pool.add_object_clip(c[1]), c) for c in MCASES]
    objs = [pool.add_object(one, worlds[i % len(worlds)], 0) for i in range(257)]
    binds = ar.bindings(MCASES[0][1])
    pool.compose()
    assert pool.anim_blend_stats().evaluated_moved == 0 and _launches()[1] == 0
    done = 0
    for n, t in ((1, 0.4), (64, 0.9), (65, 1.3), (257, 1.71)):
        for i in range(done, n):
            clip, c = clips[i % len(clips)]
            pool.set_motion(objs[i], clip, *binds[i % len(binds)], rest=c[2], base=c[3])
        done = n
        pool.set_time(t)
        pool.compose()
        assert pool.anim_blend_stats().evaluated_moved == n and _launches() == (0, 1)
        for i in range(257):
            got = pool.world_to_numpy(objs[i])
            if i < n:
                c = clips[i % len(clips)][1]
                br.check_world(got, c[1], binds[i % len(binds)], c[2], c[3], t, DEV, 'object %d of %d' % (i, n))
            else:
                assert br.same_bits(got, worlds[i % len(worlds)])


# ---------------------------------------------------------------- 4: the composed model against a twin given the fetched matrices
def _motions():
    g = np.random.default_rng(55)
    from ptina_amd.tools.anim import quaternion
    times = [0.0, 0.7, 2.0]
    return [[ar.track(0, 'T', times, g.uniform(-0.05, 0.05, (3, 3))), ar.track(0, 'R', times, [quaternion(g.normal(size=3), g.uniform(-0.2, 0.2)) for _ in times])],
            [ar.track(0, 'S', times, g.uniform(0.9, 1.1, (3, 3)), 'STEP'), ar.track(0, 'T', times, g.uniform(-0.05, 0.05, (3, 3, 3)), 'CUBICSPLINE')],
            [ar.track(0, 'R', [0.0, 2.0], [[0, 0, 0, 1], quaternion([0, 0, 1], 2.5)])]]


def test_composed_model_equals_a_twin_given_the_fetched_matrices(fresh, gold_scene):      # noqa: F811
    meshes, objs = gold_scene
    motions = _motions()
    moved = {1: (0, (0.0, 1.0, True)), 4: (1, (0.5, -0.5, True)), 6: (2, (0.25, 1.0, False)), 7: (0, (3.0, 1.0, False))}

    def scene():
        pool = _start()
        ids_m = [pool.add_mesh(*deform_ref.split(rec)) for rec in meshes]
        return pool, [pool.add_object(ids_m[m], world, mtl) for m, world, mtl in objs]
    pool, ids = scene()
    clips = [pool.add_object_clip(m) for m in motions]
    pool.compose()
    at_rest = pool.to_numpy()[0]
    for o, (k, b) in moved.items():
        pool.set_motion(ids[o], clips[k], *b, base=objs[o][1])              # about where the object stood
    frames = []
    for t in (0.6, 1.4):
        pool.set_time(t)
        pool.compose()
        assert pool.anim_blend_stats().evaluated_moved == len(moved) and pool.compose_stats().dirty_objects == len(moved)
        frames.append(([pool.world_to_numpy(o) for o in ids], pool.to_numpy()))
    assert not _same(frames[0][1][0], at_rest) and not _same(frames[0][1][0], frames[1][1][0])
    for o in range(len(ids)):
        if o not in moved:
            assert br.same_bits(frames[1][0][o], objs[o][1])
    pool, ids = scene()
    pool.compose()
    for worlds, (verts, mtl) in frames:
        for o in moved:
            pool.set_world(ids[o], worlds[o])
        pool.compose()
        got, got_m = pool.to_numpy()
        assert _same(got, verts) and np.array_equal(got_m, mtl)


def test_a_moved_blended_subdivided_surface_carries_its_sticky_scatter(fresh):
    '''a skinned, morphed surface with a subdivision level and a sticky scatter on it, blended between two clips and moved by an object
    clip: after set_time + compose the model equals, word for word, the same scene posed through set_joints / set_morph_weights and
    placed through set_world with what was fetched'''
    import subdiv_ref as sr
    case = BCASES[BNAMES.index('three joints, disjoint')]
    name, skel, T, a, b = case[:5]
    surface, tuft = sr.fixture('cylinder'), sr.fixture('tetrahedron')
    world = np.eye(4)
    world[:3, 3] = [0.2, -0.1, 0.4]
    motion = _motions()[0]

    def scene(bound, first=None):
        pool = _start()
        nj = len(skel[0])
        k = surface.shape[0] // 3
        dp, dn, jt, wt = deform_ref.random_rig(np.random.default_rng(9), k, T, nj)
        mesh = pool.add_mesh(*deform_ref.split(surface))
        pool.add_morph_targets(mesh, 0.3 * dp, dn)
        pool.add_skin(mesh, jt, wt, nj)
        pool.add_skeleton(mesh, skel[0], skel[1][:, :3], skel[1][:, 3:7], skel[1][:, 7:], skel[2])
        ca, cb = pool.add_clip(mesh, a), pool.add_clip(mesh, b)
        pool.add_subdivision(mesh, 1)
        surf = pool.add_object(mesh, world, 1)
        sid, objs = pool.add_scatter(surf, pool.add_mesh(*deform_ref.split(tuft)), 65, seed=4, mtlid=2, scale=(0.03, 0.08))
        if bound:
            _bind2(pool, surf, ca, cb, (0.25, 1.5, True), (0.0, -0.5, True), (0.0, 1.0, 0.0, 2.0))
            pool.set_motion(surf, pool.add_object_clip(motion), 0.1, 1.0, True, base=world)
            with pytest.raises(RuntimeError, match='object %d is an instance of scatter %d' % (objs[0], sid)):
                pool.set_motion(objs[0], 2)
        else:                                                              # (the scatter chooses its faces on the surface as first composed)
            pool.set_morph_weights(surf, first[0])
            pool.set_joints(surf, _mats4(first[1]))
            pool.set_world(surf, first[2])
        pool.compose()
        return pool, surf
    pool, surf = scene(True)
    at_first = pool.to_numpy()[0]
    first = (*pool.pose_to_numpy(surf), pool.world_to_numpy(surf))
    seen, models = [], []
    for t in (0.4, 1.3):
        pool.set_time(t)
        pool.compose()
        s = pool.anim_blend_stats()
        assert (s.evaluated_blended, s.evaluated_moved) == (1, 1) and pool.subdiv_stats().refined_copies == 1 and pool.scatter_stats().placed_scatters == 1
        seen.append((*pool.pose_to_numpy(surf), pool.world_to_numpy(surf)))
        models.append(pool.to_numpy())
    assert not _same(models[0][0], at_first) and not _same(models[0][0], models[1][0])
    pool, surf = scene(False, first)
    assert _same(pool.to_numpy()[0], at_first)
    for (w, pal, wm), (verts, mtl) in zip(seen, models):
        pool.set_morph_weights(surf, w)
        pool.set_joints(surf, _mats4(pal))
        pool.set_world(surf, wm)
        pool.compose()
        got, got_m = pool.to_numpy()
        assert _same(got, verts) and np.array_equal(got_m, mtl)


# ---------------------------------------------------------------- 5: build, set_time, compose, update
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_set_time_then_refit(fresh, gold_scene, mode):      # noqa: F811
    import query_ref as qr
    import refit_ref
    import visibility_ref as vr
    from test_refit_gpu import _records, _same_records
    from ptina_amd.things import BVHTree
    meshes, objs = gold_scene
    pool = _start(mode)
    case = _gentle_case()
    g = np.random.default_rng(32)
    other = [ar.track(j, 'T', [0.0, 1.0, 3.0], g.uniform(-0.03, 0.03, (3, 3))) for j in range(5)] + [ar.track(None, 'W', [0.0, 3.0], g.uniform(-0.5, 1.0, (2, 3)))]
    rigged = [_rigged(pool, rec, case, 40 + i) for i, rec in enumerate(meshes)]
    second = [pool.add_clip(r[0], other) for r in rigged]
    ids = [pool.add_object(rigged[m][0], world, mtl) for m, world, mtl in objs]
    clips = [pool.add_object_clip(m) for m in _motions()]
    pool.compose()
    tree = BVHTree()
    tree.build()
    built = _records(_ctx())
    before = pool.to_numpy()[0]
    for o, b in ((2, (0.0, 1.0, True)), (5, (0.6, -0.5, True)), (8, (0.1, 2.0, False))):
        pool.set_animation(ids[o], rigged[objs[o][0]][1], *b)
        pool.set_animation_blend(ids[o], second[objs[o][0]], 0.2, 1.0, True, weight=(0.0, 1.0), fade=(0.0, 1.0))
    for o, k in ((1, 0), (5, 1)):
        pool.set_motion(ids[o], clips[k], 0.0, 1.0, True, base=objs[o][1])
    pool.set_time(0.35)
    pool.compose()
    s = pool.anim_blend_stats()
    assert (s.evaluated_blended, s.evaluated_moved) == (3, 2) and pool.deform_stats().deformed_objects == 3 and pool.compose_stats().dirty_objects == 4
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
    bad = qr.errors(ref, tree.intersect(o, d), 'blended and moved %s' % mode, first=first)
    assert not bad, bad[:4]


# ---------------------------------------------------------------- 6: refusals, clearing, a pool that is replaced, the worker
def test_refusals_name_their_argument(fresh, gold):      # noqa: F811
    meshes, worlds = gold
    pool = _start()
    tk = ar.track
    case = BCASES[BNAMES.index('three joints, disjoint')]
    name, skel, T, a, b = case[:5]
    mesh, ca, cb, _ = _rigged2(pool, meshes[3], case, 1)
    mesh2, ca2, cb2, _ = _rigged2(pool, meshes[4], case, 2)
    plain = pool.add_mesh(*deform_ref.split(meshes[3]))
    assert (ca, cb, ca2, cb2) == (0, 1, 2, 3)
    for tr, words in (([tk(1, 'T', [0], np.zeros((1, 3)))], r'tracks\[0\] names joint 1, beyond njoints 1'),
                      ([tk(None, 'W', [0], np.ones((1, 1)))], 'morph weights of a mesh without morph targets'),
                      ([tk(0, 'R', [0, 1], [[0, 0, 0, 1], [0, 0, 0, 0]])], r'rotation values of key 1 of tracks\[0\] are zero'),
                      ([tk(0, 'T', [0], np.zeros((1, 3))), tk(0, 'T', [1], np.zeros((1, 3)))], 'animate the same target and path')):
        with pytest.raises(RuntimeError, match='mpt_scene_add_object_clip: clip: .*' + words):
            pool.add_object_clip(tr)
    with pytest.raises(RuntimeError, match='no row on the device yet'):
        pool.add_object(plain, worlds[0], 0)
        pool.world_to_numpy(0)
    pool.clear_objects()
    obj = pool.add_object(mesh, worlds[0], 0)
    rigid = pool.add_object(plain, worlds[1], 0)
    oc = pool.add_object_clip([tk(0, 'T', [0, 1], [[0, 0, 0], [1, 0, 0]])])      # at any time: objects exist already
    assert oc == 4 and pool.anim_blend_stats().object_clips == 1 and pool.anim_stats().clips == 5
    with pytest.raises(RuntimeError, match='mpt_object_set_animation_blend: object %d is not bound to a clip' % obj):
        pool.set_animation_blend(obj, cb)
    with pytest.raises(RuntimeError, match='mpt_object_set_animation: clip 4 is an object clip'):
        pool.set_animation(obj, oc)
    pool.set_animation(obj, ca)
    with pytest.raises(RuntimeError, match='mpt_object_set_animation_blend: clip 4 is an object clip'):
        pool.set_animation_blend(obj, oc)
    with pytest.raises(RuntimeError, match='clip 3 is a clip of mesh %d, object %d an object of mesh %d' % (mesh2, obj, mesh)):
        pool.set_animation_blend(obj, cb2)
    with pytest.raises(RuntimeError, match=r'unknown clip 5 \(5 clips\)'):
        pool.set_animation_blend(obj, 5)
    with pytest.raises(RuntimeError, match='object %d has neither morph targets nor a skin' % rigid):
        pool.set_animation_blend(rigid, cb)
    for kw, words in ((dict(weight=-0.25), 'w0 lies outside'), (dict(weight=(0.5, 1.5)), 'w1 lies outside'), (dict(weight=np.nan), 'w0 lies outside'),
                      (dict(fade=(0.0, -1.0)), 'fade_duration is negative'), (dict(fade=(np.inf, 1.0)), 'fade_start is not finite'),
                      (dict(fade=(0.0, np.inf)), 'fade_duration is not finite'), (dict(offset=np.nan), 'offset is not finite'), (dict(speed=np.inf), 'speed is not finite')):
        with pytest.raises(RuntimeError, match='mpt_object_set_animation_blend: ' + words):
            pool.set_animation_blend(obj, cb, **kw)
    with pytest.raises(RuntimeError, match='mpt_object_set_motion: clip 1 is a clip of mesh %d' % mesh):
        pool.set_motion(rigid, cb)
    with pytest.raises(RuntimeError, match=r'mpt_object_set_motion: unknown clip 9 \(5 clips\)'):
        pool.set_motion(rigid, 9)
    with pytest.raises(ValueError, match='unknown object'):
        pool.set_motion(99, oc)
    for kw, words in ((dict(rest=[0, 0, 0, 0, 0, 0, 0, 1, 1, 1]), r'the rest rotation rest\[3..6\] is zero'), (dict(rest=[0, np.nan, 0, 0, 0, 0, 1, 1, 1, 1]), r'rest\[1\] is not finite'),
                      (dict(base=np.full((4, 4), np.inf)), r'base\[0\] is not finite'), (dict(offset=np.inf), 'offset is not finite'), (dict(speed=np.nan), 'speed is not finite')):
        with pytest.raises(RuntimeError, match='mpt_object_set_motion: ' + words):
            pool.set_motion(rigid, oc, **kw)
    with pytest.raises(ValueError, match='rest must hold 10 numbers'):
        pool.set_motion(rigid, oc, rest=[0, 0, 0])
    pool.set_motion(rigid, oc)
    with pytest.raises(RuntimeError, match='mpt_object_set_world: object %d is bound to object clip 4.*unbind it first' % rigid):
        pool.set_world(rigid, worlds[2])
    pool.set_animation_blend(obj, cb, 0.1, weight=0.5)
    pool.set_animation(obj, ca, 0.3)                                       # binding A again leaves B
    pool.set_time(0.5)
    pool.compose()
    s = pool.anim_blend_stats()
    assert (s.object_clips, s.blended_objects, s.moved_objects, s.evaluated_blended, s.evaluated_moved) == (1, 1, 1, 1, 1)
    br.check_blend(pool.pose_to_numpy(obj), skel, T, a, (0.3, 1.0, True), b, (0.1, 1.0, True), (0.5, 0.5, 0.0, 0.0), 0.5, DEV, 'A bound again')
    want = np.eye(4)
    want[0, 3] = 0.5
    assert br.same_bits(pool.world_to_numpy(rigid), want)
    pool.set_animation(obj, None)                                          # removes both bindings
    assert pool.anim_blend_stats().blended_objects == 0 and pool.anim_stats().bound_objects == 0
    pool.set_animation(obj, ca)
    pool.compose()
    assert pool.anim_blend_stats().evaluated_blended == 0 and pool.anim_stats().evaluated_objects == 1
    # clear_objects drops the bindings and keeps the clips; clear_meshes drops both; a new pool starts empty and works
    pool.clear_objects()
    s = pool.anim_blend_stats()
    assert (s.object_clips, s.blended_objects, s.moved_objects) == (1, 0, 0) and pool.anim_stats().clips == 5
    rigid = pool.add_object(plain, worlds[1], 0)
    pool.compose()
    assert br.same_bits(pool.world_to_numpy(rigid), worlds[1]) and pool.anim_blend_stats().evaluated_moved == 0
    pool.set_world(rigid, worlds[2])                                       # no binding: set_world takes it
    pool.set_motion(rigid, oc, 0.25)
    pool.compose()
    want[0, 3] = 0.25
    assert br.same_bits(pool.world_to_numpy(rigid), want)
    pool.clear_meshes()
    s = pool.anim_blend_stats()
    assert (s.object_clips, s.blended_objects, s.moved_objects) == (0, 0, 0) and pool.anim_stats().clips == 0
    pool = _start()
    assert pool.anim_blend_stats().object_clips == 0
    rigid = pool.add_object(pool.add_mesh(*deform_ref.split(meshes[3])), worlds[1], 0)
    pool.set_motion(rigid, pool.add_object_clip([tk(0, 'T', [0, 1], [[0, 0, 0], [1, 0, 0]])]), 0.25)
    pool.set_time(0.5)
    pool.compose()
    assert br.same_bits(pool.world_to_numpy(rigid), want), 'a new pool evaluates the same clip to the same matrix'


def test_worker_facade_through_the_thread_proxy(fresh, gold):      # noqa: F811
    import threading
    from ptina_amd.common import reset_all
    from ptina_amd.tools.mtworker import DaemonModule, OnDemandProxy
    meshes, worlds = gold
    case = BCASES[BNAMES.index('three joints, disjoint')]
    name, skel, T, a, b = case[:5]
    motion = _motions()[0]
    pool = _start()
    mesh, ca, cb, _ = _rigged2(pool, meshes[2], case, 5)
    obj = pool.add_object(mesh, worlds[0], 0)
    _bind2(pool, obj, ca, cb, (0.3, -1.25, True), (0.1, 1.0, True), (0.25, 0.75, 1.0, 0.5))
    pool.set_motion(obj, pool.add_object_clip(motion), 0.2, base=worlds[0])
    pool.set_time(1.1)
    pool.compose()
    direct_v, direct_m = pool.to_numpy()
    direct_pose, direct_world = pool.pose_to_numpy(obj), pool.world_to_numpy(obj)
    reset_all()
    seen = []

    def module():
        seen.append(threading.get_ident())
        from ptina_amd import worker
        ns = types.SimpleNamespace(**{k: getattr(worker, k) for k in dir(worker) if not k.startswith('_')})

        def rig():
            p = worker.ModelPool()
            k = meshes[2].shape[0] // 3
            dp, dn, jt, wt = deform_ref.random_rig(np.random.default_rng(5), k, T, 3)
            m = p.add_mesh(*deform_ref.split(meshes[2]))
            p.add_morph_targets(m, dp, dn)
            p.add_skin(m, jt, wt, 3)
            return m
        ns.rig = rig
        ns.add = lambda m: worker.ModelPool().add_object(m, worlds[0], 0)
        ns.fetch = lambda: worker.ModelPool().to_numpy()
        ns.pose = lambda o: worker.ModelPool().pose_to_numpy(o)
        ns.world = lambda o: worker.ModelPool().world_to_numpy(o)
        return ns
    w = OnDemandProxy(lambda: DaemonModule(module))
    w.init()
    m = w.rig()
    w.set_mesh_skeleton(m, skel[0], skel[1][:, :3], skel[1][:, 3:7], rest_scale=skel[1][:, 7:], inverse_bind=skel[2])
    c1, c2 = w.add_mesh_clip(mesh=m, tracks=a), w.add_mesh_clip(mesh=m, tracks=b)
    o = w.add(m)
    w.set_object_animation(o, c1, offset=0.3, speed=-1.25)
    w.set_object_animation_blend(o, c2, offset=0.1, weight=(0.25, 0.75), fade=(1.0, 0.5))
    oc = w.add_object_clip(tracks=motion)
    w.set_object_motion(o, oc, 0.2, base=worlds[0])
    w.set_scene_time(t=1.1)
    w.compose_model()
    assert seen and seen[0] != threading.get_ident()
    got_v, got_m = w.fetch()
    assert _same(got_v, direct_v) and np.array_equal(got_m, direct_m)
    gw, gp = w.pose(o)
    assert br.same_bits(gw, direct_pose[0]) and br.same_bits(gp, direct_pose[1]) and br.same_bits(w.world(o), direct_world)
    w.synchronize()

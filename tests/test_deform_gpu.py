'''
GPU tests (-m gpu) of mesh deformation on the device (ModelPool.add_morph_targets / add_skin / set_morph_weights / set_joints /
deformed_to_numpy / deform_stats, mpt_mesh_set_* ... mpt_deform_stats; ptina_amd/csrc/deform.hip, scene_deform.cpp; DESIGN.md
section 3.17).

The kernel is held to tests/deform_ref.py BIT FOR BIT, with no margin rule: both sides evaluate the same expressions in f64 in the
same order, every operation a correctly rounded IEEE + * / sqrt, and round to f32 once.  The meshes are those of
tests/golden/reference_compose.npz -- 0, 1, 21, 22, 85, 86 and 300 faces: 256 corners are 85 1/3 faces, so the seams between
lanes' corners and waves occur inside every larger mesh.  A workgroup takes a chunk of 1024 corners and the largest fixture mesh
has 900, so the objects of several chunks -- a chunk index above 0, the tail in a later chunk, runs that start at later blocks --
are stacks of the fixture meshes: 1200 faces (three chunks and a tail of 528 corners) and 1024 faces (3072 corners: the last
chunk ends exactly on its boundary).
'''

import ctypes as C
import os
import types

import numpy as np
import pytest

import compose_ref
import deform_ref

pytestmark = pytest.mark.gpu
u32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20


@pytest.fixture(scope='module')
def gold():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_compose.npz'))
    meshes = [deform_ref.records(g['mesh%d_p' % i], g['mesh%d_n' % i], g['mesh%d_t' % i]) for i in range(int(g['nmeshes']))]
    objs = [(int(m), np.array(g['obj_world'][o], np.float64), None if g['obj_mtl_none'][o] else int(g['obj_mtl'][o]))
            for o, m in enumerate(g['obj_mesh'])]
    assert sorted(r.shape[0] // 3 for r in meshes) == [0, 1, 21, 22, 85, 86, 300] and len(objs) == 9
    return meshes, objs


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u32), b.view(u32))


def _pool():
    from ptina_amd.things import ModelPool
    return ModelPool()


def _ctx():
    from ptina_amd.common import ctx
    return ctx()


def _start(mode=None):
    from ptina_amd import _lib
    from ptina_amd.common import reset_all
    from ptina_amd.things import init_things
    reset_all()
    init_things()
    if mode is not None:                 # what the batch queries ask for beside the tree: an engine's build, a film, a camera
        from ptina_amd import scenes
        from ptina_amd.engine.path import PathEngine
        from ptina_amd.things import FilmTable, Camera
        PathEngine()
        _ctx().set_option('mode', _lib.MODE_STRICT if mode == 'strict' else _lib.MODE_FAST)
        FilmTable().set_size(32, 32)
        Camera().set_perspective(scenes.BENCH_CAMERA)
    return _pool()


def _mesh_of(meshes, faces):
    return next(i for i, r in enumerate(meshes) if r.shape[0] == 3 * faces)


def _sphere(info):
    return np.array([*info.scene_cen, info.scene_rad], np.float64).view(np.uint64).tolist()


# ---------------------------------------------------------------- rigs, poses and the expected copies (fixed seeds)
def _rig(rec, T, nj, seed):
    '''deltas [T,m,6], joints [m,4], weights [m,4] for the records rec (None where T / nj is 0).  With a skin, corner 0 puts all its
    weight on joint nj - 1 and the four indices of corner 1 are equal'''
    g = np.random.default_rng(seed)
    k = rec.shape[0] // 3
    dp, dn, jt, wt = deform_ref.random_rig(g, k, T, nj)
    rig = dict(T=T, nj=nj, dp=dp, dn=dn, jt=jt, wt=wt, deltas=None, joints=None, weights=None)
    if T:
        rig['deltas'] = np.ascontiguousarray(np.concatenate([dp.reshape(T, k * 3, 3), dn.reshape(T, k * 3, 3)], axis=2))
    if nj:
        if k > 0:
            jt[0, 0], wt[0, 0] = [nj - 1, 0, 0, 0], [1, 0, 0, 0]
            jt[0, 1] = int(g.integers(0, nj))
        rig['joints'], rig['weights'] = jt.reshape(k * 3, 4), wt.reshape(k * 3, 4)
    return rig


def _pose(rig, seed, rest=False):
    '''(w [T] or None, mats [nj,4,4] or None): of three weights the middle one is exactly 0'''
    g = np.random.default_rng(seed)
    w = mats = None
    if rig['T']:
        w = np.zeros(rig['T']) if rest else g.uniform(-1.0, 1.5, rig['T'])
        if rig['T'] == 3:
            w[1] = 0.0
    if rig['nj']:
        mats = np.tile(np.eye(4), (rig['nj'], 1, 1)) if rest else deform_ref.random_joints(g, rig['nj'])
    return w, mats


def _expected(rec, rig, pose):
    return deform_ref.deform(rec, rig['deltas'], pose[0], rig['joints'], rig['weights'], pose[1])


def _add_rigged_mesh(pool, rec, rig):
    mesh = pool.add_mesh(*deform_ref.split(rec))
    if rig['T']:
        pool.add_morph_targets(mesh, rig['dp'], rig['dn'])
    if rig['nj']:
        pool.add_skin(mesh, rig['jt'], rig['wt'], rig['nj'])
    return mesh


def _set_pose(pool, obj, pose):
    if pose[0] is not None:
        pool.set_morph_weights(obj, pose[0])
    if pose[1] is not None:
        pool.set_joints(obj, pose[1])


def _build_scene(pool, gold, rigs, poses):
    '''the fixture's nine objects with mesh i rigged by rigs[i] and object o posed by poses[o]; composes.  Returns the object ids'''
    meshes, objs = gold
    ids = [_add_rigged_mesh(pool, rec, rigs[i]) for i, rec in enumerate(meshes)]
    out = []
    for o, (m, world, mtl) in enumerate(objs):
        obj = pool.add_object(ids[m], world, mtl)
        _set_pose(pool, obj, poses[o])
        out.append(obj)
    pool.compose()
    return out


def _rigs(gold, kinds):
    '''kinds: one (T, nj) for every mesh, or a list per mesh'''
    meshes, _ = gold
    kinds = [kinds] * len(meshes) if isinstance(kinds, tuple) else kinds
    return [_rig(rec, *kinds[i], seed=SEED + i) for i, rec in enumerate(meshes)]


def _poses(gold, rigs, salt=0, rest=()):
    _, objs = gold
    return [_pose(rigs[m], 1000 + 17 * o + salt, rest=o in rest) for o, (m, _, _) in enumerate(objs)]


def _plain_prims(gold, rigs, poses):
    '''the (p, n, t, w, m) tuples of plain meshes made from the expected copies (objects that are not deformable: their mesh)'''
    meshes, objs = gold
    prims = []
    for o, (m, world, mtl) in enumerate(objs):
        rec = _expected(meshes[m], rigs[m], poses[o]) if rigs[m]['T'] or rigs[m]['nj'] else meshes[m]
        prims.append((*deform_ref.split(rec), world, mtl))
    return prims


MIXED = [(0, 1), (0, 0), (2, 0), (0, 7), (1, 64), (3, 0), (3, 5)]          # per mesh: skin only, neither, morph only, ..., both (the largest)


# ---------------------------------------------------------------- 1: the deformed copies, bit for bit
@pytest.mark.parametrize('T,nj', [(1, 0), (3, 0), (0, 1), (0, 5), (0, 256), (3, 5), (1, 256)])
def test_deformed_copies_equal_the_restatement_bit_for_bit(fresh, gold, T, nj):
    '''morph only, skin only and both; one weight of three exactly 0; 1, 5 and 256 joints; a corner with all its weight on the last
    joint and one whose four indices are equal; objects of one mesh in different poses'''
    meshes, objs = gold
    pool = _start()
    rigs = _rigs(gold, (T, nj))
    poses = _poses(gold, rigs)
    ids = _build_scene(pool, gold, rigs, poses)
    shared = [m for m, _, _ in objs]
    assert any(shared.count(m) > 1 and meshes[m].shape[0] > 0 for m in shared), 'no two objects of one mesh'
    if nj:
        big = rigs[int(np.argmax([r.shape[0] for r in meshes]))]
        assert big['joints'][0].tolist() == [nj - 1, 0, 0, 0] and big['weights'][0].tolist() == [1, 0, 0, 0] and len(set(big['joints'][1].tolist())) == 1
    if T == 3:
        assert all(p[0][1] == 0.0 and p[0][0] != 0.0 and p[0][2] != 0.0 for p in poses)
    seen = {}
    for o, obj in enumerate(ids):
        m = objs[o][0]
        got = pool.deformed_to_numpy(obj)
        want = _expected(meshes[m], rigs[m], poses[o])
        bad = np.flatnonzero((got.view(u32) != want.view(u32)).any(axis=1))
        print('T %d nj %d object %d (%d corners): %d records differ' % (T, nj, o, want.shape[0], bad.size))
        assert got.dtype == np.float32 and got.shape == want.shape and bad.size == 0, (o, bad[:8], got[bad[:2]], want[bad[:2]])
        if m in seen and want.shape[0]:
            assert not _same(got, seen[m]), 'two objects of one mesh share a pose'
        seen[m] = got
    info = pool.deform_stats()
    corners = sum(meshes[m].shape[0] for m, _, _ in objs)
    assert (info.deformable_objects, info.deformed_objects, info.deformed_corners, info.copy_verts) == (9, 9, corners, corners)


# ---------------------------------------------------------------- 1b: objects of several chunks
def _stacked(meshes, faces):
    '''records of `faces` faces: the fixture meshes, largest first, one after the other and over again'''
    order = sorted((r for r in meshes if r.shape[0]), key=lambda r: -r.shape[0])
    rec = np.concatenate(order * (1 + 3 * faces // sum(r.shape[0] for r in order)))
    return np.ascontiguousarray(rec[:3 * faces])


@pytest.mark.parametrize('T,nj', [(3, 0), (0, 5), (3, 5), (1, 256)])
def test_objects_of_several_chunks_equal_the_restatement_bit_for_bit(fresh, gold, T, nj):
    '''a chunk index above 0, a tail inside the fourth chunk, a last chunk that ends on its boundary, and runs that start at blocks
    4, 7, 8 and 12: 1200-face and 1024-face objects side by side, with a one-chunk object between them; then two of the five posed
    again, so that a run table with gaps maps later blocks to later objects'''
    from ptina_amd import _lib
    meshes, objs = gold
    chunk = _lib.DEFORM_CHUNK
    recs = [_stacked(meshes, 1200), _stacked(meshes, 1024), meshes[_mesh_of(meshes, 300)]]
    assert [r.shape[0] for r in recs] == [3 * chunk + 528, 3 * chunk, 900] and chunk == 1024
    rigs = [_rig(rec, T, nj, seed=SEED + 40 + i) for i, rec in enumerate(recs)]
    layout = [0, 1, 2, 0, 1]                                                   # the mesh of every object
    corners = [recs[m].shape[0] for m in layout]
    runs, blocks = _lib.deform_plan(corners)
    assert runs == [(0, 0), (1, 4), (2, 7), (3, 8), (4, 12)] and blocks == 15
    pool = _start()
    ids = [_add_rigged_mesh(pool, rec, rigs[i]) for i, rec in enumerate(recs)]
    poses, out = [], []
    for o, m in enumerate(layout):
        poses.append(_pose(rigs[m], 300 + o))
        out.append(pool.add_object(ids[m], objs[o][1], o % 3))
        _set_pose(pool, out[-1], poses[-1])
    _ctx().timer('mpt_deform_kernel_time')
    pool.compose()
    ms, launches = _ctx().timer('mpt_deform_kernel_time')
    assert launches == 1 and ms > 0, 'one launch per compose covers every posed object'
    info = pool.deform_stats()
    assert (info.deformed_objects, info.deformed_corners, info.copy_verts) == (5, sum(corners), sum(corners))

    def check(what):
        prims = []
        for o, m in enumerate(layout):
            got = pool.deformed_to_numpy(out[o])
            want = _expected(recs[m], rigs[m], poses[o])
            bad = np.flatnonzero((got.view(u32) != want.view(u32)).any(axis=1))
            print('%s T %d nj %d object %d (%d corners): %d records differ' % (what, T, nj, o, want.shape[0], bad.size))
            assert got.shape == want.shape and bad.size == 0, (what, o, bad[:8], (bad // chunk)[:8], got[bad[:2]], want[bad[:2]])
            prims.append((*deform_ref.split(want), objs[o][1], o % 3))
        return prims
    check('all')
    assert not _same(pool.deformed_to_numpy(out[0]), pool.deformed_to_numpy(out[3]))
    for o in (1, 3):                                                           # runs (1, 0) and (3, 3): block 3 is object 3's first
        poses[o] = _pose(rigs[layout[o]], 400 + o)
        _set_pose(pool, out[o], poses[o])
    assert _lib.deform_plan(corners, [0, 1, 0, 1, 0]) == ([(1, 0), (3, 3)], 7)
    pool.compose()
    ms, launches = _ctx().timer('mpt_deform_kernel_time')
    assert launches == 1
    info = pool.deform_stats()
    assert (info.deformed_objects, info.deformed_corners) == (2, corners[1] + corners[3])
    prims = check('two of five')
    got_v, got_m = pool.to_numpy()
    pool.compose()                                                             # nothing changed: no launch at all
    assert _ctx().timer('mpt_deform_kernel_time')[1] == 0 and pool.deform_stats().deformed_objects == 0
    plain = _start()
    plain.load_meshes(prims)
    want_v, want_m = plain.to_numpy()
    assert _same(got_v, want_v) and np.array_equal(got_m, want_m)


# ---------------------------------------------------------------- 2: end to end through compose_kernel
def test_composed_model_equals_the_plain_meshes_of_the_copies(fresh, gold):
    pool = _start()
    rigs = _rigs(gold, MIXED)
    poses = _poses(gold, rigs)
    ids = _build_scene(pool, gold, rigs, poses)
    meshes, objs = gold
    prims = _plain_prims(gold, rigs, poses)
    deformable = 0
    for o, obj in enumerate(ids):
        m = objs[o][0]
        if rigs[m]['T'] or rigs[m]['nj']:
            deformable += 1
            assert _same(pool.deformed_to_numpy(obj), deform_ref.records(*prims[o][:3]))
        else:
            with pytest.raises(RuntimeError, match='neither morph targets nor a skin'):
                pool.deformed_to_numpy(obj)
    assert 0 < deformable < 9 and pool.deform_stats().deformable_objects == deformable
    got_v, got_m = pool.to_numpy()
    sphere = _sphere(pool.compose_stats())
    plain = _start()
    plain.load_meshes(prims)
    want_v, want_m = plain.to_numpy()
    assert plain.deform_stats().deformable_objects == 0
    assert _same(got_v, want_v) and np.array_equal(got_m, want_m) and got_v.shape[0] == 621 * 3
    assert sphere == _sphere(plain.compose_stats())


# ---------------------------------------------------------------- 3: one pose of nine
@pytest.mark.parametrize('changed', [0, 4, 7, 8])      # (object 4: a mesh without faces; 7: shares its mesh with 3)
def test_pose_change_deforms_and_recomposes_that_object_alone(fresh, gold, changed):
    meshes, objs = gold
    pool = _start()
    rigs = _rigs(gold, (3, 5))
    poses = _poses(gold, rigs)
    ids = _build_scene(pool, gold, rigs, poses)
    before, _ = pool.to_numpy()
    faces = meshes[objs[changed][0]].shape[0] // 3
    final = list(poses)
    final[changed] = _pose(rigs[objs[changed][0]], 777)
    _set_pose(pool, ids[changed], final[changed])
    pool.compose()
    d, c = pool.deform_stats(), pool.compose_stats()
    assert (d.deformable_objects, d.deformed_objects, d.deformed_corners) == (9, 1, 3 * faces)
    assert (c.faces, c.recomposed, c.dirty_objects) == (621, faces, 1)
    got_v, got_m = pool.to_numpy()
    sphere = _sphere(c)
    first = np.concatenate([[0], np.cumsum([meshes[m].shape[0] for m, _, _ in objs])])
    differs = (got_v.view(u32) != before.view(u32)).any(axis=1)
    assert not differs[:first[changed]].any() and not differs[first[changed + 1]:].any() and (faces == 0 or differs.any())
    # a set_world on a deformable object recomposes it without deforming it again
    world = compose_ref.grid_world(np.random.default_rng(9), 1, 1) @ objs[changed][1]
    pool.set_world(ids[changed], world)
    pool.compose()
    d, c = pool.deform_stats(), pool.compose_stats()
    assert (d.deformed_objects, d.deformed_corners) == (0, 0) and (c.recomposed, c.dirty_objects) == (faces, 1)
    moved_v, _ = pool.to_numpy()
    pool.set_world(ids[changed], objs[changed][1])
    pool.compose()
    assert _same(pool.to_numpy()[0], got_v)
    # from scratch with the final poses
    scratch = _start()
    _build_scene(scratch, gold, rigs, final)
    want_v, want_m = scratch.to_numpy()
    assert _same(got_v, want_v) and np.array_equal(got_m, want_m) and sphere == _sphere(scratch.compose_stats())
    scratch.set_world(ids[changed], world)
    scratch.compose()
    assert _same(moved_v, scratch.to_numpy()[0])


# ---------------------------------------------------------------- 4: build, pose, compose, refit
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_pose_change_then_refit(fresh, gold, mode):
    import query_ref as qr
    import refit_ref
    import visibility_ref as vr
    from test_refit_gpu import _records, _same_records
    from ptina_amd.things import BVHTree
    meshes, objs = gold
    pool = _start(mode)
    rigs = _rigs(gold, (3, 5))
    rest = _poses(gold, rigs, rest=range(9))
    ids = _build_scene(pool, gold, rigs, rest)
    tree = BVHTree()
    tree.build()
    built = _records(_ctx())
    posed = _poses(gold, rigs, salt=5)
    for o in (2, 5, 8):
        _set_pose(pool, ids[o], posed[o])
    pool.compose()
    assert pool.deform_stats().deformed_objects == 3
    assert tree.refit_stats().allowed and tree.can_refit()
    growth = tree.refit()
    print('deform %s: growth %.6f after the refit' % (mode, growth))
    assert tree.refit_stats().host_fetches == 0
    got = _records(_ctx())
    model, _ = pool.to_numpy()
    pos = vr.positions(model)
    assert pos.shape[0] == 621
    bmin, bmax, w, q = refit_ref.refit_ref(built['child'], built['leaf'], built['wnode'], built['qnode'], 621, pos)
    _same_records(got, dict(built, bmin=bmin, bmax=bmax, wnode=w, qnode=q), 'refit after a pose change (%s)' % mode)
    first = np.concatenate([[0], np.cumsum([meshes[m].shape[0] // 3 for m, _, _ in objs])])[:9]
    o, d = qr.rays(pos, 4, 512)
    ref = qr.classify(pos, o, d)
    dec = ref['decided']
    assert dec.mean() >= 0.9 and (dec & ref['hit']).any() and (dec & ~ref['hit']).any()
    bad = qr.errors(ref, tree.intersect(o, d), 'deformed %s' % mode, first=first)
    assert not bad, bad[:4]
    # the same pose through update(), with a max_growth below the measured growth: builds instead
    for o in (2, 5, 8):
        _set_pose(pool, ids[o], rest[o])
    pool.compose()
    tree.build()
    for o in (2, 5, 8):
        _set_pose(pool, ids[o], posed[o])
    pool.compose()
    assert _same(pool.to_numpy()[0], model)
    assert tree.update(max_growth=float(np.nextafter(growth, 0.0))) == 'build' and tree.refit_stats().refits == 0


# ---------------------------------------------------------------- 5: refusals
def test_refusals_name_their_argument_and_leave_the_scene(fresh, gold):
    meshes, objs = gold
    pool = _start()
    rigs = _rigs(gold, MIXED)
    poses = _poses(gold, rigs)
    ids = _build_scene(pool, gold, rigs, poses)
    before_v, before_m = pool.to_numpy()
    c = _ctx()
    f32p, u16p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_double)
    fp = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(f32p)     # noqa: E731
    up = lambda a: np.ascontiguousarray(a, np.uint16).ctypes.data_as(u16p)      # noqa: E731
    dp = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(f64p)     # noqa: E731
    rec = meshes[_mesh_of(meshes, 21)]
    k3 = rec.shape[0]
    used = objs[0][0]                                                          # a mesh that has an object
    both = next(o for o, (m, _, _) in enumerate(objs) if MIXED[m] == (3, 5))
    with pytest.raises(RuntimeError, match='mpt_get_deformed: room for -1 faces'):
        c.call('mpt_get_deformed', ids[both], None, -1)
    with pytest.raises(RuntimeError, match='mpt_get_deformed: unknown object 9'):
        c.call('mpt_get_deformed', 9, None, 0)
    fresh_mesh = pool.add_mesh(*deform_ref.split(rec))                         # (a mesh while copies exist: their room is assigned again)
    d1, j1, w1 = np.zeros((1, k3, 6), np.float32), np.zeros((k3, 4), np.uint16), np.full((k3, 4), 0.25, np.float32)

    def refused(words, fn, *args):
        with pytest.raises(RuntimeError, match=words):
            c.call(fn, *args)
    # the meshes
    refused('mpt_mesh_set_morph: unknown mesh 99', 'mpt_mesh_set_morph', 99, fp(d1), 1)
    refused('mpt_mesh_set_skin: unknown mesh -1', 'mpt_mesh_set_skin', -1, up(j1), fp(w1), 4)
    refused('mpt_mesh_set_morph: mesh %d already has an object' % used, 'mpt_mesh_set_morph', used, fp(d1), 1)
    refused('mpt_mesh_set_skin: mesh %d already has an object' % used, 'mpt_mesh_set_skin', used, up(j1), fp(w1), 4)
    refused('no deformed copy yet', 'mpt_get_deformed', ids[both], None, 0)     # (the added mesh took the copies' room)
    for T in (0, -3, 65):
        refused(r'mpt_mesh_set_morph: T %d outside \[1, 64\]' % T, 'mpt_mesh_set_morph', fresh_mesh, fp(d1), T)
    for nj in (0, 257):
        refused(r'mpt_mesh_set_skin: skin: njoints %d outside \[1, 256\]' % nj, 'mpt_mesh_set_skin', fresh_mesh, up(j1), fp(w1), nj)
    bad = j1.copy()
    bad[5, 2] = 4
    refused(r'mpt_mesh_set_skin: skin: joints\[5\]\[2\] names joint 4', 'mpt_mesh_set_skin', fresh_mesh, up(bad), fp(w1), 4)
    for value in (np.nan, np.inf):
        bad = d1.copy()
        bad[0, 7, 4] = value
        refused(r'mpt_mesh_set_morph: deltas\[0\]\[7\]\[4\] is not finite', 'mpt_mesh_set_morph', fresh_mesh, fp(bad), 1)
        bad = w1.copy()
        bad[k3 - 1, 3] = value
        refused(r'mpt_mesh_set_skin: skin: weights\[%d\]\[3\] is not finite' % (k3 - 1), 'mpt_mesh_set_skin', fresh_mesh, up(j1), fp(bad), 4)
    bad = w1.copy()
    bad[0, 0] = -0.25
    refused(r'mpt_mesh_set_skin: skin: weights\[0\]\[0\] is negative', 'mpt_mesh_set_skin', fresh_mesh, up(j1), fp(bad), 4)
    with pytest.raises(ValueError, match=r'joint indices must lie in \[0, 4\)'):
        pool.add_skin(fresh_mesh, np.full((k3 // 3, 3, 4), 65536 + 1), w1.reshape(-1, 3, 4), 4)      # (would wrap to 1 in the cast)
    with pytest.raises(ValueError, match='already has an object'):
        pool.add_morph_targets(used, np.zeros((1, meshes[used].shape[0] // 3, 3, 3)))
    # the objects: MIXED makes object o's mesh (T, nj)
    neither = next(o for o, (m, _, _) in enumerate(objs) if MIXED[m] == (0, 0))
    morph_only = next(o for o, (m, _, _) in enumerate(objs) if MIXED[m][0] and not MIXED[m][1])
    skin_only = next(o for o, (m, _, _) in enumerate(objs) if MIXED[m][1] and not MIXED[m][0])
    eye5 = np.tile(np.eye(4), (5, 1, 1))
    refused('mpt_object_set_morph_weights: unknown object 9', 'mpt_object_set_morph_weights', 9, dp(np.zeros(3)), 3)
    refused('mpt_object_set_joints: unknown object -1', 'mpt_object_set_joints', -1, dp(eye5), 5)
    refused('mpt_object_set_morph_weights: n 2, the mesh of object %d has 3 morph targets' % both, 'mpt_object_set_morph_weights', ids[both], dp(np.zeros(2)), 2)
    refused('mpt_object_set_joints: n 6, the skin of the mesh of object %d has 5 joints' % both, 'mpt_object_set_joints', ids[both], dp(np.tile(np.eye(4), (6, 1, 1))), 6)
    for o in (neither, skin_only):
        refused('mpt_object_set_morph_weights: the mesh of object %d has no morph targets' % o, 'mpt_object_set_morph_weights', ids[o], dp(np.zeros(3)), 3)
    for o in (neither, morph_only):
        refused('mpt_object_set_joints: the mesh of object %d has no skin' % o, 'mpt_object_set_joints', ids[o], dp(eye5), 5)
    refused(r'mpt_object_set_morph_weights: w\[2\] is not finite', 'mpt_object_set_morph_weights', ids[both], dp([0.5, 0.5, np.nan]), 3)
    bad = eye5.copy()
    bad[3, 1, 2] = -np.inf
    refused(r'mpt_object_set_joints: mats\[3\]\[6\] is not finite', 'mpt_object_set_joints', ids[both], dp(bad), 5)
    for r, value in ((0, 1e-300), (3, 1.0 + 2.0 ** -52), (1, -1.0)):
        bad = eye5.copy()
        bad[4, 3, r] = value
        refused(r'mpt_object_set_joints: the bottom row of mats\[4\] is not 0 0 0 1', 'mpt_object_set_joints', ids[both], dp(bad), 5)
    with pytest.raises(ValueError, match=r'\[njoints,4,4\]'):
        pool.set_joints(ids[both], np.eye(4))
    # the scene still composes to what it was
    pool.compose()
    info = pool.deform_stats()
    assert info.deformed_objects == info.deformable_objects > 0           # (the added mesh took the copies' room: all again)
    after_v, after_m = pool.to_numpy()
    assert _same(after_v, before_v) and np.array_equal(after_m, before_m)


# ---------------------------------------------------------------- 6: the pool buffer is replaced between two compositions
def test_growing_the_pool_keeps_everything_right(fresh, gold):
    meshes, objs = gold
    big = int(np.argmax([r.shape[0] for r in meshes]))
    pool = _start()
    rigs = _rigs(gold, (2, 4))
    ids = [_add_rigged_mesh(pool, rec, rigs[i]) for i, rec in enumerate(meshes)]
    held = sum(r.shape[0] for r in meshes)
    scene = [(big, objs[0][1], 1, _pose(rigs[big], 1))]
    obj0 = pool.add_object(ids[big], scene[0][1], 1)
    _set_pose(pool, obj0, scene[0][3])
    pool.compose()
    assert pool.deform_stats().copy_verts == 900 and pool.deform_stats().deformed_objects == 1
    first = pool.deformed_to_numpy(obj0)
    # 24 more objects of the largest mesh: twelve times the vertices the pool held (it grows by doubling, so it is replaced)
    for k in range(24):
        world = compose_ref.grid_world(np.random.default_rng(100 + k), k % 3, k // 8)
        scene.append((big, world, k % 3, _pose(rigs[big], 50 + k)))
        _set_pose(pool, pool.add_object(ids[big], world, k % 3), scene[-1][3])
    assert held + 25 * 900 > 4 * (held + 900)
    pool.compose()
    info = pool.deform_stats()
    assert (info.deformable_objects, info.deformed_objects, info.deformed_corners, info.copy_verts) == (25, 25, 25 * 900, 25 * 900)
    assert _same(pool.deformed_to_numpy(obj0), first)
    prims = []
    for o, (m, world, mtl, pose) in enumerate(scene):
        want = _expected(meshes[m], rigs[m], pose)
        assert _same(pool.deformed_to_numpy(o), want), o
        prims.append((*deform_ref.split(want), world, mtl))
    got_v, got_m = pool.to_numpy()
    plain = _start()
    plain.load_meshes(prims)
    want_v, want_m = plain.to_numpy()
    assert _same(got_v, want_v) and np.array_equal(got_m, want_m)


# ---------------------------------------------------------------- 7: clear_objects gives the copies' room back
def test_clear_objects_returns_the_copies_room(fresh, gold):
    meshes, objs = gold
    pool = _start()
    rigs = _rigs(gold, (1, 3))
    _build_scene(pool, gold, rigs, _poses(gold, rigs))
    assert pool.deform_stats().copy_verts == 621 * 3
    pool.clear_objects()
    info = pool.deform_stats()
    assert (info.copy_verts, info.deformable_objects) == (0, 0)
    rec, m_old = meshes[_mesh_of(meshes, 85)], _mesh_of(meshes, 22)
    rig = _rig(rec, 2, 6, seed=3)
    mesh = _add_rigged_mesh(pool, rec, rig)
    pose = _pose(rig, 4)
    obj = pool.add_object(mesh, objs[4][1], 2)
    old = pool.add_object(m_old, objs[0][1], 1)                                 # ... beside an object of a mesh from before, at rest
    _set_pose(pool, obj, pose)
    pool.compose()
    info = pool.deform_stats()
    assert (info.deformable_objects, info.deformed_objects, info.copy_verts) == (2, 2, rec.shape[0] + 66)
    want = _expected(rec, rig, pose)
    assert _same(pool.deformed_to_numpy(obj), want)
    want_old = _expected(meshes[m_old], rigs[m_old], _pose(rigs[m_old], 0, rest=True))
    assert _same(pool.deformed_to_numpy(old), want_old)
    got_v, got_m = pool.to_numpy()
    plain = _start()
    plain.load_meshes([(*deform_ref.split(want), objs[4][1], 2), (*deform_ref.split(want_old), objs[0][1], 1)])
    want_v, want_m = plain.to_numpy()
    assert _same(got_v, want_v) and np.array_equal(got_m, want_m)


# ---------------------------------------------------------------- 8: the worker facade
def test_worker_facade_through_the_thread_proxy(fresh, gold):
    import threading
    from ptina_amd.common import reset_all
    from ptina_amd.tools.mtworker import DaemonModule, OnDemandProxy
    meshes, objs = gold
    rigs = _rigs(gold, (3, 5))
    rest = _poses(gold, rigs, rest=range(9))
    posed = _poses(gold, rigs, salt=3)
    pool = _start()
    ids = _build_scene(pool, gold, rigs, rest)
    for o in (1, 6):
        _set_pose(pool, ids[o], posed[o])
    pool.compose()
    direct_v, direct_m = pool.to_numpy()
    reset_all()
    seen = []

    def module():
        seen.append(threading.get_ident())
        from ptina_amd import worker
        ns = types.SimpleNamespace(**{k: getattr(worker, k) for k in dir(worker) if not k.startswith('_')})
        ns.rig_scene = lambda: _build_scene(worker.ModelPool(), gold, rigs, rest)      # (what an add-on does with ModelPool on its worker thread)
        ns.fetch = lambda: worker.ModelPool().to_numpy()
        ns.stats = lambda: worker.ModelPool().deform_stats().deformed_objects
        return ns
    w = OnDemandProxy(lambda: DaemonModule(module))
    w.init()
    ids = w.rig_scene()
    assert ids == list(range(9)) and seen and seen[0] != threading.get_ident()
    for o in (1, 6):
        w.set_object_morph_weights(ids[o], posed[o][0])
        w.set_object_joints(obj=ids[o], mats=posed[o][1])
    w.compose_model()
    assert w.stats() == 2
    got_v, got_m = w.fetch()
    assert _same(got_v, direct_v) and np.array_equal(got_m, direct_m)
    w.synchronize()

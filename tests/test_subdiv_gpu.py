'''
GPU tests (-m gpu) of Loop subdivision on the device (ModelPool.add_subdivision / subdivided_to_numpy / subdiv_stats,
mpt_mesh_set_subdivision ... mpt_subdiv_kernel_time; ptina_amd/csrc/subdiv.hip, scene_subdiv.cpp).

The kernels are held to tests/subdiv_ref.py BIT FOR BIT, NaN positions included, with no margin: both sides evaluate the same
expressions in f64 in the same order, every operation a correctly rounded IEEE + - * / sqrt, and round to f32 once.  A workgroup
takes 256 items (vertices of a level, or faces of the last).  The meshes are subdiv_ref's procedural fixtures; the largest job is
the 50-triangle grid at level 3: 3200 faces and 1681 vertices, several blocks and a tail in every launch; the tetrahedron at level
3 has 256 faces and the octahedron 512: the record launch's last block of those jobs ends exactly on its boundary.
'''

import types

import numpy as np
import pytest

import compose_ref
import deform_ref
import subdiv_ref as sr

pytestmark = pytest.mark.gpu
u32 = np.uint32
EYE = np.eye(4)


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


def _world(seed):
    return compose_ref.grid_world(np.random.default_rng(seed), seed % 3, seed % 2)


def _add(pool, name, levels, rig=None):
    rec = sr.fixture(name)
    mesh = pool.add_mesh(*deform_ref.split(rec))
    if rig is not None and rig['first'] == 'levels':
        pool.add_subdivision(mesh, levels)
    if rig is not None:
        pool.add_morph_targets(mesh, rig['dp'], rig['dn'])
        pool.add_skin(mesh, rig['jt'], rig['wt'], rig['nj'])
    if levels and (rig is None or rig['first'] != 'levels'):
        pool.add_subdivision(mesh, levels)
    return mesh


def _launches():
    *ms, n = _ctx().timer('mpt_subdiv_kernel_time', 3)                    # (refine levels, normals, records; kernels launched)
    assert all(m >= 0 for m in ms)
    return n


def _sphere(info):
    return np.array([*info.scene_cen, info.scene_rad], np.float64).view(np.uint64).tolist()


def _differ(got, want, what):
    '''bit for bit; a NaN must stand where the restatement has one (its sign and payload are the processor's, not the definition's)'''
    bad = np.flatnonzero(((got.view(u32) != want.view(u32)) & ~(np.isnan(got) & np.isnan(want))).any(axis=1))
    print('%s (%d corners): %d records differ' % (what, want.shape[0], bad.size))
    assert got.dtype == np.float32 and got.shape == want.shape and bad.size == 0, (what, bad[:8], got[bad[:2]], want[bad[:2]])


# ---------------------------------------------------------------- rigs and poses for the meshes that deform
def _rig(name, seed, first='rig', T=2, nj=4):
    g = np.random.default_rng(seed)
    k = sr.fixture(name).shape[0] // 3
    dp, dn, jt, wt = deform_ref.random_rig(g, k, T, nj)
    return dict(T=T, nj=nj, dp=dp, dn=dn, jt=jt, wt=wt, first=first, deltas=np.ascontiguousarray(np.concatenate([dp.reshape(T, k * 3, 3), dn.reshape(T, k * 3, 3)], axis=2)),
                joints=jt.reshape(k * 3, 4), weights=wt.reshape(k * 3, 4))


def _pose(seed, rest=False, T=2, nj=4):
    g = np.random.default_rng(seed)
    if rest:
        return np.zeros(T), np.tile(EYE, (nj, 1, 1))
    return g.uniform(-1.0, 1.5, T), deform_ref.random_joints(g, nj)


def _deformed(name, rig, pose):
    return deform_ref.deform(sr.fixture(name), rig['deltas'], pose[0], rig['joints'], rig['weights'], pose[1])


def _expected(name, levels, rig=None, pose=None):
    if rig is None:
        return sr.fixture_subdivided(name, levels)
    return sr.subdivide(sr.fixture(name), levels, sr.fixture_topology(name, levels), control=_deformed(name, rig, pose))


def _set_pose(pool, obj, pose):
    pool.set_morph_weights(obj, pose[0])
    pool.set_joints(obj, pose[1])


# ---------------------------------------------------------------- 1: every fixture, bit for bit
@pytest.mark.parametrize('levels', [1, 2, 3])
def test_subdivided_copies_equal_the_restatement_bit_for_bit(fresh, levels):
    '''every fixture at this level, one object each, one compose: valence 3, 7 and 12, boundaries and corners, uv seams; at level
    3 the grid's 3200 faces (12 blocks and a tail of 128) and the tetrahedron's 256 and the octahedron's 512 (whole blocks)'''
    pool = _start()
    objs = [pool.add_object(_add(pool, name, levels), _world(i), i % 3) for i, name in enumerate(sr.NAMES)]
    pool.compose()
    faces = 0
    for name, obj in zip(sr.NAMES, objs):
        want = _expected(name, levels)
        assert want.shape[0] == sr.fixture(name).shape[0] * 4 ** levels
        _differ(pool.subdivided_to_numpy(obj), want, '%s at level %d' % (name, levels))
        faces += want.shape[0] // 3
    if levels == 3:
        sizes = [_expected(n, 3).shape[0] // 3 for n in ('grid', 'tetrahedron', 'octahedron')]
        assert sizes == [3200, 256, 512] and 3200 % sr.CHUNK and 256 % sr.CHUNK == 0
    info = pool.subdiv_stats()
    assert (info.subdivided_objects, info.copies, info.refined_copies, info.refined_faces, info.copy_verts) == (9, 9, 9, faces, 3 * faces)
    assert pool.nfaces == faces and _launches() == levels + 2


def test_a_nan_normal_comes_out_as_the_restatement_has_it(fresh):
    '''joint matrices of scale zero collapse a skinned cylinder onto one point: every normal sum is zero and every normal a NaN, on
    both sides, in the same places; positions and texcoords stay numbers'''
    rig = _rig('cylinder', 2)
    mats = np.zeros((4, 4, 4))
    mats[:, :3, 3], mats[:, 3, 3] = [0.25, -1.0, 2.0], 1.0
    pose = (np.zeros(2), mats)
    want = _expected('cylinder', 2, rig, pose)
    assert np.isnan(want[:, 3:6]).all() and np.isfinite(want[:, [0, 1, 2, 6, 7]]).all()
    pool = _start()
    obj = pool.add_object(_add(pool, 'cylinder', 2, rig), EYE)
    _set_pose(pool, obj, pose)
    pool.compose()
    got = pool.subdivided_to_numpy(obj)
    _differ(got, want, 'collapsed cylinder')
    assert np.isnan(got[:, 3:6]).all()


# ---------------------------------------------------------------- 2: launches do not grow with the objects
def test_five_objects_of_different_levels_take_the_launches_of_one(fresh):
    pool = _start()
    obj = pool.add_object(_add(pool, 'icosahedron', 3), EYE)
    pool.compose()
    one = _launches()
    assert one == 5                                                       # three refine launches, the normals, the records
    _differ(pool.subdivided_to_numpy(obj), _expected('icosahedron', 3), 'one object')
    pool = _start()
    scene = [('grid', 1), ('fan7', 3), ('cylinder', 2), ('pair', 1), ('icosahedron', 3)]
    objs = [pool.add_object(_add(pool, name, L), _world(i)) for i, (name, L) in enumerate(scene)]
    pool.compose()
    assert _launches() == one
    for (name, L), obj in zip(scene, objs):
        _differ(pool.subdivided_to_numpy(obj), _expected(name, L), '%s at level %d beside four others' % (name, L))
    assert pool.subdiv_stats().refined_copies == 5
    pool.compose()                                                        # nothing changed: nothing launched
    assert _launches() == 0 and pool.subdiv_stats().refined_copies == 0


# ---------------------------------------------------------------- 3: behind the deformation
def _posed_scene(pool, poses):
    '''grid (level 2, level set before the rig) twice and cylinder (level 2, level set after the rig) once, each in its own pose,
    beside a rigid subdivided tetrahedron and a plain octahedron.  Returns (rigs, objects)'''
    rigs = dict(grid=_rig('grid', 1, first='levels'), cylinder=_rig('cylinder', 2))
    mg, mc = _add(pool, 'grid', 2, rigs['grid']), _add(pool, 'cylinder', 2, rigs['cylinder'])
    mt, mo = _add(pool, 'tetrahedron', 2), _add(pool, 'octahedron', 0)
    objs = [pool.add_object(m, _world(10 + i), i % 3) for i, m in enumerate((mg, mt, mg, mc, mo))]
    for o, pose in poses.items():
        _set_pose(pool, objs[o], pose)
    pool.compose()
    return rigs, objs


POSED = {0: 'grid', 2: 'grid', 3: 'cylinder'}


def _posed_expected(rigs, poses):
    out = {o: _expected(name, 2, rigs[name], poses[o]) for o, name in POSED.items()}
    out[1] = _expected('tetrahedron', 2)
    out[4] = sr.fixture('octahedron')
    return out


def test_subdivision_behind_skinning_and_morphing(fresh):
    '''poses from deform_ref; the restatement is fed the deformed copy.  The rigs move every corner on its own, so welded corners
    come apart and the first corner speaks for its vertex.  One object of several posed again: it alone is subdivided again;
    set_world alone subdivides nothing'''
    pool = _start()
    poses = {0: _pose(31), 2: _pose(32), 3: _pose(33)}
    rigs, objs = _posed_scene(pool, poses)
    want = _posed_expected(rigs, poses)
    copy = pool.deformed_to_numpy(objs[0])
    assert _same(copy, _deformed('grid', rigs['grid'], poses[0]))
    faces, first = sr.weld(sr.fixture('grid'))
    apart = [v for v in range(first.size) if np.unique(copy[np.flatnonzero(faces.reshape(-1) == v), :3], axis=0).shape[0] > 1]
    assert len(apart) > 10, 'the pose leaves the welded corners together'
    for o in POSED:
        _differ(pool.subdivided_to_numpy(objs[o]), want[o], 'posed object %d' % o)
    _differ(pool.subdivided_to_numpy(objs[1]), want[1], 'rigid object')
    assert not _same(pool.subdivided_to_numpy(objs[0]), pool.subdivided_to_numpy(objs[2])), 'two objects of one mesh share a pose'
    with pytest.raises(RuntimeError, match='no subdivision level'):
        pool.subdivided_to_numpy(objs[4])
    info = pool.subdiv_stats()
    assert (info.subdivided_objects, info.copies, info.refined_copies, info.copy_verts) == (4, 4, 4, 3 * 16 * (50 + 50 + 32 + 4))
    assert _launches() == 4
    # the composed model: what load_meshes makes of plain meshes made from the copies, bounding sphere included
    got_v, got_m = pool.to_numpy()
    sphere = _sphere(pool.compose_stats())
    # one pose of three
    poses[2] = _pose(77)
    _set_pose(pool, objs[2], poses[2])
    pool.compose()
    info, d = pool.subdiv_stats(), pool.deform_stats()
    assert (info.refined_copies, info.refined_faces, d.deformed_objects) == (1, 800, 1) and _launches() == 4
    again = _posed_expected(rigs, poses)
    for o in (0, 1, 2, 3):
        _differ(pool.subdivided_to_numpy(objs[o]), again[o], 'object %d after object 2 was posed' % o)
    posed_v, _ = pool.to_numpy()
    pool.set_world(objs[2], _world(5))
    pool.set_material(objs[0], 2)
    pool.compose()
    info, c = pool.subdiv_stats(), pool.compose_stats()
    assert (info.refined_copies, info.refined_faces) == (0, 0) and _launches() == 0 and (c.dirty_objects, c.recomposed) == (2, 1600)
    pool.set_world(objs[2], _world(12))
    pool.set_material(objs[0], 0)
    pool.compose()
    assert _same(pool.to_numpy()[0], posed_v)
    plain = _start()
    first_poses = {0: poses[0], 2: _pose(32), 3: poses[3]}
    first_want = _posed_expected(rigs, first_poses)
    plain.load_meshes([(*deform_ref.split(first_want[i]), _world(10 + i), i % 3) for i in range(5)])
    want_v, want_m = plain.to_numpy()
    assert _same(got_v, want_v) and np.array_equal(got_m, want_m) and got_v.shape[0] == 3 * (16 * 136 + 8)
    assert sphere == _sphere(plain.compose_stats())


# ---------------------------------------------------------------- 4: a rigid mesh has one copy
def test_a_rigid_mesh_with_three_objects_has_one_copy(fresh):
    pool = _start()
    mesh = _add(pool, 'fan12', 2)
    objs = [pool.add_object(mesh, _world(i), i) for i in range(3)]
    pool.compose()
    info = pool.subdiv_stats()
    assert (info.subdivided_objects, info.copies, info.refined_copies, info.refined_faces, info.copy_verts) == (3, 1, 1, 384, 1152)
    want = _expected('fan12', 2)
    for obj in objs:
        _differ(pool.subdivided_to_numpy(obj), want, 'object %d of the shared copy' % obj)
    got_v, got_m = pool.to_numpy()
    assert pool.nfaces == 3 * 384 and pool.compose_stats().faces == 3 * 384
    plain = _start()
    plain.load_meshes([(*deform_ref.split(want), _world(i), i) for i in range(3)])
    assert _same(got_v, plain.to_numpy()[0]) and np.array_equal(got_m, plain.to_numpy()[1])


# ---------------------------------------------------------------- 5: build, pose, compose, update: a refit
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_pose_change_then_update_refits(fresh, mode):
    import query_ref as qr
    import refit_ref
    import visibility_ref as vr
    from test_refit_gpu import _records, _same_records
    from ptina_amd.things import BVHTree
    pool = _start(mode)
    rest = {o: _pose(0, rest=True) for o in POSED}
    rigs, objs = _posed_scene(pool, rest)
    nfaces = 16 * 136 + 8
    tree = BVHTree()
    tree.build()
    built = _records(_ctx())
    g = np.random.default_rng(4)
    posed = {o: (0.2 * g.uniform(-1, 1, 2), deform_ref.random_joints(g, 4, amount=0.05)) for o in POSED}
    for o in (0, 3):
        _set_pose(pool, objs[o], posed[o])
    pool.compose()
    assert pool.subdiv_stats().refined_copies == 2 and pool.nfaces == nfaces
    assert tree.update(max_growth=float('inf')) == 'refit' and tree.refit_stats().refits == 1 and tree.refit_stats().host_fetches == 0
    got = _records(_ctx())
    model, _ = pool.to_numpy()
    want = _posed_expected(rigs, {0: posed[0], 2: rest[2], 3: posed[3]})
    for o in POSED:
        _differ(pool.subdivided_to_numpy(objs[o]), want[o], 'posed object %d before the refit' % o)
    pos = vr.positions(model)
    assert pos.shape[0] == nfaces
    bmin, bmax, w, q = refit_ref.refit_ref(built['child'], built['leaf'], built['wnode'], built['qnode'], nfaces, pos)
    _same_records(got, dict(built, bmin=bmin, bmax=bmax, wnode=w, qnode=q), 'refit after a pose change of subdivided objects (%s)' % mode)
    first = np.concatenate([[0], np.cumsum([want[i].shape[0] // 3 for i in range(5)])])[:5]
    o, d = qr.rays(pos, 4, 512)
    ref = qr.classify(pos, o, d)
    dec = ref['decided']
    assert dec.mean() >= 0.9 and (dec & ref['hit']).any() and (dec & ~ref['hit']).any()
    bad = qr.errors(ref, tree.intersect(o, d), 'subdivided %s' % mode, first=first)
    assert not bad, bad[:4]


# ---------------------------------------------------------------- 6: refusals
def test_refusals_say_what_is_wrong_and_leave_the_scene(fresh):
    from test_subdiv_cpu import REFUSALS
    pool = _start()
    good = _add(pool, 'octahedron', 0)
    for kind, (code, words, make) in sorted(REFUSALS.items()):
        rec = make()
        if kind == 'finite':
            continue                                                      # (add_mesh takes it, see below)
        mesh = pool.add_mesh(*deform_ref.split(rec))
        with pytest.raises(RuntimeError, match=words):
            pool.add_subdivision(mesh, 2)
    mesh = pool.add_mesh(*deform_ref.split(REFUSALS['finite'][2]()))
    with pytest.raises(RuntimeError, match='corner 1 of face 1 is not finite'):
        pool.add_subdivision(mesh, 1)
    c = _ctx()
    with pytest.raises(RuntimeError, match=r'levels 0 outside \[1, 5\]'):
        c.call('mpt_mesh_set_subdivision', good, 0)
    with pytest.raises(RuntimeError, match=r'levels 6 outside \[1, 5\]'):
        c.call('mpt_mesh_set_subdivision', good, 6)
    with pytest.raises(RuntimeError, match='unknown mesh'):
        c.call('mpt_mesh_set_subdivision', 99, 1)
    with pytest.raises(ValueError):
        pool.add_subdivision(good, 6)
    with pytest.raises(ValueError):
        pool.add_subdivision(99, 1)
    big = pool.add_mesh(*deform_ref.split(sr.mesh_records(*sr.grid(32, 32))))                  # 2048 faces: 2^21 at level 5
    with pytest.raises(RuntimeError, match='too many faces: 2097152 at level 5'):
        c.call('mpt_mesh_set_subdivision', big, 5)
    with pytest.raises(ValueError, match='too many faces'):
        pool.add_subdivision(big, 5)
    pool.add_subdivision(good, 1)
    with pytest.raises(RuntimeError, match='already has a subdivision level'):
        c.call('mpt_mesh_set_subdivision', good, 1)
    obj = pool.add_object(good, EYE)
    other = _add(pool, 'pair', 0)
    plain = pool.add_object(other, EYE)
    with pytest.raises(RuntimeError, match='already has an object'):
        c.call('mpt_mesh_set_subdivision', other, 1)
    with pytest.raises(RuntimeError, match='no subdivided copy yet'):
        pool.subdivided_to_numpy(obj)
    pool.compose()
    with pytest.raises(RuntimeError, match='no subdivision level'):
        pool.subdivided_to_numpy(plain)
    with pytest.raises(RuntimeError, match='room for 3 faces'):
        c.call('mpt_get_subdivided', obj, None, 3)
    with pytest.raises(RuntimeError, match='unknown object'):
        c.call('mpt_get_subdivided', 7, None, 0)
    # an object budget counts k 4^L
    tiny = type(pool).__new__(type(pool))
    type(pool).__init__(tiny, 30)
    tiny._mesh_faces, tiny._mesh_levels = [8], {0: 1}
    with pytest.raises(ValueError, match='too many faces: 32 with this object'):
        tiny.add_object(0, EYE)
    _differ(pool.subdivided_to_numpy(obj), _expected('octahedron', 1), 'after the refusals')
    assert pool.nfaces == 32 + 2


# ---------------------------------------------------------------- 7: the copies' room is assigned again
def test_clear_and_mesh_add_while_copies_exist(fresh):
    pool = _start()
    rig = _rig('cylinder', 2)
    pose = _pose(8)
    mc, mi = _add(pool, 'cylinder', 2, rig), _add(pool, 'icosahedron', 1)
    oc, oi = pool.add_object(mc, _world(1)), pool.add_object(mi, _world(2))
    _set_pose(pool, oc, pose)
    pool.compose()
    want_c, want_i = _expected('cylinder', 2, rig, pose), _expected('icosahedron', 1)
    _differ(pool.subdivided_to_numpy(oc), want_c, 'cylinder')
    assert pool.subdiv_stats().copy_verts == 3 * (512 + 80)
    # a mesh joins the pool where the copies lay: the next compose assigns their room again and makes them again
    mg = _add(pool, 'grid', 3)
    assert pool.subdiv_stats().copy_verts == 0
    with pytest.raises(RuntimeError, match='no subdivided copy yet'):
        pool.subdivided_to_numpy(oc)
    og = pool.add_object(mg, _world(3))
    pool.compose()
    info = pool.subdiv_stats()
    assert (info.copies, info.refined_copies, info.copy_verts) == (3, 3, 3 * (512 + 80 + 3200))
    _differ(pool.subdivided_to_numpy(oc), want_c, 'cylinder after a mesh was added')
    _differ(pool.subdivided_to_numpy(oi), want_i, 'icosahedron after a mesh was added')
    _differ(pool.subdivided_to_numpy(og), _expected('grid', 3), 'the new grid')
    assert _same(pool.deformed_to_numpy(oc), _deformed('cylinder', rig, pose))
    # clear_objects: the copies go, the meshes and their levels stay
    pool.clear_objects()
    info = pool.subdiv_stats()
    assert (info.subdivided_objects, info.copies, info.copy_verts) == (0, 0, 0)
    oi = pool.add_object(mi, _world(4))
    oi2 = pool.add_object(mi, _world(5))
    pool.compose()
    info = pool.subdiv_stats()
    assert (info.subdivided_objects, info.copies, info.copy_verts, pool.nfaces) == (2, 1, 240, 160)
    _differ(pool.subdivided_to_numpy(oi2), want_i, 'icosahedron after clear_objects')
    # clear_meshes: everything goes; a new mesh starts from nothing
    pool.clear_meshes()
    assert pool.subdiv_stats().copies == 0
    obj = pool.add_object(_add(pool, 'fan7', 2), EYE)
    pool.compose()
    _differ(pool.subdivided_to_numpy(obj), _expected('fan7', 2), 'fan7 after clear_meshes')
    assert pool.nfaces == 14 * 16


# ---------------------------------------------------------------- 8: the worker facade
def test_worker_facade_through_the_thread_proxy(fresh):
    import threading
    from ptina_amd.common import reset_all
    from ptina_amd.tools.mtworker import DaemonModule, OnDemandProxy
    reset_all()
    rig = _rig('grid', 1)
    pose = _pose(21)
    seen = []

    def module():
        seen.append(threading.get_ident())
        from ptina_amd import worker
        ns = types.SimpleNamespace(**{k: getattr(worker, k) for k in dir(worker) if not k.startswith('_')})

        def rig_mesh():                                                   # (what an add-on does with ModelPool on its worker thread)
            pool = worker.ModelPool()
            mesh = pool.add_mesh(*deform_ref.split(sr.fixture('grid')))
            pool.add_morph_targets(mesh, rig['dp'], rig['dn'])
            pool.add_skin(mesh, rig['jt'], rig['wt'], rig['nj'])
            return mesh
        ns.rig_mesh = rig_mesh
        ns.add_object = lambda mesh: worker.ModelPool().add_object(mesh, _world(1))
        ns.fetch = lambda obj: worker.ModelPool().subdivided_to_numpy(obj)
        ns.stats = lambda: worker.ModelPool().subdiv_stats().refined_faces
        return ns
    w = OnDemandProxy(lambda: DaemonModule(module))
    w.init()
    mesh = w.rig_mesh()
    w.set_mesh_subdivision(mesh=mesh, levels=2)
    obj = w.add_object(mesh)
    assert seen and seen[0] != threading.get_ident()
    w.set_object_morph_weights(obj, pose[0])
    w.set_object_joints(obj=obj, mats=pose[1])
    w.compose_model()
    assert w.stats() == 800
    _differ(w.fetch(obj), _expected('grid', 2, rig, pose), 'through the worker')
    w.synchronize()

'''
GPU tests (-m gpu) of semi-sharp creases, corners and hard edges of Loop subdivision on the device (ModelPool.add_subdivision with
creases and corners, mpt_mesh_set_subdivision_creased; ptina_amd/csrc/subdiv.hip, scene_subdiv.cpp).

The kernels are held to tests/subdiv_crease_ref.py BIT FOR BIT with no margin, as tests/test_subdiv_gpu.py holds the uncreased
ones to subdiv_ref: both sides evaluate the same expressions in f64 in the same order and round to f32 once.  The largest job is
the creased 50-triangle grid at level 3 (3200 faces: 12 blocks and a tail); the cube at level 2 has 192 faces, less than a block.
'''

import types

import numpy as np
import pytest

import compose_ref
import deform_ref
import displace_ref
import subdiv_ref as sr
import subdiv_crease_ref as ref
from test_subdiv_gpu import _start, _ctx, _same, _differ, _launches, _world, _sphere, _rig, _pose, _set_pose, EYE

pytestmark = pytest.mark.gpu
u32 = np.uint32


def _add(pool, name, levels, rig=None):
    rec, creases, corners = ref.fixture(name)
    mesh = pool.add_mesh(*deform_ref.split(rec))
    if rig is not None:
        pool.add_morph_targets(mesh, rig['dp'], rig['dn'])
        pool.add_skin(mesh, rig['jt'], rig['wt'], rig['nj'])
    pool.add_subdivision(mesh, levels, creases=creases, corners=corners)
    return mesh


def _grid_rig(seed):
    g = np.random.default_rng(seed)
    dp, dn, jt, wt = deform_ref.random_rig(g, 50, 2, 4)
    return dict(T=2, nj=4, dp=dp, dn=dn, jt=jt, wt=wt, deltas=np.ascontiguousarray(np.concatenate([dp.reshape(2, 150, 3), dn.reshape(2, 150, 3)], axis=2)),
                joints=jt.reshape(150, 4), weights=wt.reshape(150, 4))


def _posed(name, levels, rig, pose):
    rec = ref.fixture(name)[0]
    control = deform_ref.deform(rec, rig['deltas'], pose[0], rig['joints'], rig['weights'], pose[1])
    return ref.subdivide(rec, levels, topo=ref.fixture_topology(name, levels), control=control)


# ---------------------------------------------------------------- 1: every fixture, bit for bit
@pytest.mark.parametrize('levels', [1, 2, 3])
def test_creased_copies_equal_the_restatement_bit_for_bit(fresh, levels):
    pool = _start()
    objs = [pool.add_object(_add(pool, name, levels), _world(i), i % 3) for i, name in enumerate(ref.NAMES)]
    pool.compose()
    for name, obj in zip(ref.NAMES, objs):
        want = ref.fixture_subdivided(name, levels)
        assert want.shape[0] == ref.fixture(name)[0].shape[0] * 4 ** levels
        _differ(pool.subdivided_to_numpy(obj), want, '%s at level %d' % (name, levels))
    assert _launches() == levels + 2
    sizes = {2: ('cube_inf', 192), 3: ('grid_line', 3200)}
    if levels in sizes:
        name, faces = sizes[levels]
        assert ref.fixture_subdivided(name, levels).shape[0] == 3 * faces and (faces < sr.CHUNK or faces % sr.CHUNK)


@pytest.mark.parametrize('levels', [1, 2, 3])
def test_inf_cube_normals_are_its_faces_axes(fresh, levels):
    '''every corner normal is exactly the axis of the cube face its triangle lies in; a cube corner carries three normals; every
    position lies on the cube'''
    pool = _start()
    obj = pool.add_object(_add(pool, 'cube_inf', levels), EYE)
    pool.compose()
    got = pool.subdivided_to_numpy(obj).reshape(-1, 3, 8)
    pos, nrm = got[:, :, :3], got[:, :, 3:6]
    assert (np.abs(pos).max(axis=2) == 1.0).all()
    on = (np.abs(pos) == 1.0).all(axis=1)                                # [F,3]: the axes the whole triangle is at +-1 of
    assert (on.sum(axis=1) == 1).all()
    axis = np.where(on[:, None, :], np.sign(pos), 0.0).astype(np.float32)
    assert np.array_equal(nrm, axis) and not np.signbit(nrm[nrm == 0]).any()
    flat_p, flat_n = pos.reshape(-1, 3), nrm.reshape(-1, 3)
    for corner in np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32):
        here = (flat_p == corner).all(axis=1)
        assert np.unique(flat_n[here], axis=0).shape[0] == 3


# ---------------------------------------------------------------- 2: no crease, no difference
def test_zero_creases_equal_the_uncreased_call_record_for_record(fresh):
    pool = _start()
    objs = []
    for i, (name, levels) in enumerate((('grid', 3), ('fan7', 2), ('cylinder', 1))):
        rec = sr.fixture(name)
        k = rec.shape[0] // 3
        for creases, corners in ((None, None), (np.zeros((k, 3), np.float32), None), (None, np.zeros((k, 3), bool)), (np.zeros((k, 3)), np.zeros((k, 3), np.uint8))):
            mesh = pool.add_mesh(*deform_ref.split(rec))
            if creases is None and corners is None:
                pool.add_subdivision(mesh, levels)
            else:
                pool.add_subdivision(mesh, levels, creases=creases, corners=corners)
            objs.append((name, levels, pool.add_object(mesh, _world(i))))
    pool.compose()
    plain = {}
    for name, levels, obj in objs:
        got = pool.subdivided_to_numpy(obj)
        _differ(got, sr.fixture_subdivided(name, levels), 'zero creases on %s' % name)
        assert _same(got, plain.setdefault(name, got))
    assert _launches() == 5


def test_a_creased_and_an_uncreased_mesh_in_one_compose(fresh):
    pool = _start()
    mesh = pool.add_mesh(*deform_ref.split(sr.fixture('icosahedron')))
    pool.add_subdivision(mesh, 3)
    a = pool.add_object(mesh, _world(1))
    b = pool.add_object(_add(pool, 'grid_corners', 2), _world(2))
    c = pool.add_object(_add(pool, 'cube_1p5', 1), _world(3))
    pool.compose()
    assert _launches() == 3 + 2
    _differ(pool.subdivided_to_numpy(a), sr.fixture_subdivided('icosahedron', 3), 'the uncreased mesh')
    _differ(pool.subdivided_to_numpy(b), ref.fixture_subdivided('grid_corners', 2), 'the creased grid')
    _differ(pool.subdivided_to_numpy(c), ref.fixture_subdivided('cube_1p5', 1), 'the creased cube')
    info = pool.subdiv_stats()
    assert (info.copies, info.refined_copies, info.refined_faces) == (3, 3, 20 * 64 + 50 * 16 + 12 * 4)
    pool.compose()
    assert _launches() == 0


def test_refusals_through_the_pool(fresh):
    pool = _start()
    rec, creases, _ = ref.fixture('octa_dart')
    mesh = pool.add_mesh(*deform_ref.split(rec))
    bad = creases.copy()
    bad[5, 2] = -0.5
    with pytest.raises(RuntimeError, match='mpt_mesh_set_subdivision_creased: mesh 0: subdivision: the crease of edge 2 of face 5 is negative'):
        pool.add_subdivision(mesh, 2, creases=bad)
    bad[5, 2] = np.nan
    with pytest.raises(RuntimeError, match='the crease of edge 2 of face 5 is not a number'):
        pool.add_subdivision(mesh, 2, creases=bad)
    with pytest.raises(ValueError, match=r'creases must be \[8,3\]'):
        pool.add_subdivision(mesh, 2, creases=np.zeros((7, 3)))
    with pytest.raises(ValueError, match=r'corners must be \[8,3\]'):
        pool.add_subdivision(mesh, 2, corners=np.zeros((8, 2)))
    pool.add_subdivision(mesh, 2, creases=creases)                        # (the refusals left the mesh without a level)
    obj = pool.add_object(mesh, EYE)
    pool.compose()
    _differ(pool.subdivided_to_numpy(obj), ref.fixture_subdivided('octa_dart', 2), 'after the refusals')


# ---------------------------------------------------------------- 3: behind the deformation
def test_a_skinned_creased_grid(fresh):
    '''two objects of the skinned creased grid, each in its pose; one posed again: it alone is refined again'''
    pool = _start()
    rig = _grid_rig(5)
    mesh = _add(pool, 'grid_line', 2, rig)
    objs = [pool.add_object(mesh, _world(i)) for i in range(2)]
    poses = [_pose(41), _pose(42)]
    for obj, pose in zip(objs, poses):
        _set_pose(pool, obj, pose)
    pool.compose()
    for obj, pose in zip(objs, poses):
        _differ(pool.subdivided_to_numpy(obj), _posed('grid_line', 2, rig, pose), 'posed object %d' % obj)
    assert pool.subdiv_stats().refined_copies == 2 and _launches() == 4
    poses[1] = _pose(43)
    _set_pose(pool, objs[1], poses[1])
    pool.compose()
    info = pool.subdiv_stats()
    assert (info.refined_copies, info.refined_faces) == (1, 800) and _launches() == 4
    for obj, pose in zip(objs, poses):
        _differ(pool.subdivided_to_numpy(obj), _posed('grid_line', 2, rig, pose), 'object %d after object 1 was posed' % obj)


# ---------------------------------------------------------------- 4: a displacement takes its direction from the whole ring
@pytest.mark.parametrize('mode', ['normal', 'vector'])
def test_a_creased_displaced_grid(fresh, mode):
    from ptina_amd.things import ImagePool
    image = displace_ref.random_image(3, 9, 7)
    levels, strength, midlevel = 2, 0.3, 0.4
    rec, creases, corners = ref.fixture('grid_corners')
    topo = ref.fixture_topology('grid_corners', levels)
    P = ref.fixture_positions('grid_corners', levels)[-1]
    uv = displace_ref.vertex_uv(rec, dict(faces=topo['vfaces'], rings=topo['rings']), levels)
    rgba = displace_ref.sample(image, uv[:, 0], uv[:, 1])
    if mode == 'normal':
        n = sr.normals(P, topo['rings'])                                  # the whole ring: one direction per vertex, no crack
        Pd = P + (strength * (displace_ref.height(rgba, displace_ref.MEAN) - midlevel))[:, None] * n
    else:
        Pd = P + strength * (rgba[:, :3] - midlevel)
    want = ref.records_of(rec, topo, Pd)
    pool = _start()
    ImagePool().load([image])
    mesh = pool.add_mesh(*deform_ref.split(rec))
    pool.add_subdivision(mesh, levels, creases=creases, corners=corners)
    pool.add_displacement(mesh, 0, strength, midlevel, mode, 'mean')
    obj = pool.add_object(mesh, EYE)
    pool.compose()
    got = pool.subdivided_to_numpy(obj)
    _differ(got, want, 'creased grid displaced (%s)' % mode)
    # no crack: the corners on a vertex share its position, and the crease line splits their normals
    assert not _same(got, ref.fixture_subdivided('grid_corners', levels))
    flat = topo['faces'].reshape(-1)
    vert = np.array([r[0] for r in topo['records']])[flat]
    first = displace_ref.first_corners(vert, P.shape[0])
    assert np.array_equal(got[:, :3].view(u32), got[first[vert], :3].view(u32))
    assert len(topo['records']) > P.shape[0]


# ---------------------------------------------------------------- 5: build, pose, compose, update: a refit
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_pose_change_then_update_refits(fresh, mode):
    import query_ref as qr
    import refit_ref
    import visibility_ref as vr
    from test_refit_gpu import _records, _same_records
    from ptina_amd.things import BVHTree
    pool = _start(mode)
    rig = _grid_rig(6)
    mesh = _add(pool, 'grid_line', 2, rig)
    objs = [pool.add_object(mesh, _world(10)), pool.add_object(_add(pool, 'cube_inf', 2), _world(11)), pool.add_object(mesh, _world(12))]
    rest = _pose(0, rest=True)
    for o in (0, 2):
        _set_pose(pool, objs[o], rest)
    pool.compose()
    nfaces = 800 + 192 + 800
    tree = BVHTree()
    tree.build()
    built = _records(_ctx())
    g = np.random.default_rng(4)
    posed = (0.2 * g.uniform(-1, 1, 2), deform_ref.random_joints(g, 4, amount=0.05))
    _set_pose(pool, objs[0], posed)
    pool.compose()
    assert pool.subdiv_stats().refined_copies == 1 and pool.nfaces == nfaces
    assert tree.update(max_growth=float('inf')) == 'refit' and tree.refit_stats().refits == 1 and tree.refit_stats().host_fetches == 0
    got = _records(_ctx())
    model, _ = pool.to_numpy()
    want = [_posed('grid_line', 2, rig, posed), ref.fixture_subdivided('cube_inf', 2), _posed('grid_line', 2, rig, rest)]
    for obj, w in zip(objs, want):
        _differ(pool.subdivided_to_numpy(obj), w, 'object %d before the refit' % obj)
    pos = vr.positions(model)
    assert pos.shape[0] == nfaces
    bmin, bmax, w, q = refit_ref.refit_ref(built['child'], built['leaf'], built['wnode'], built['qnode'], nfaces, pos)
    _same_records(got, dict(built, bmin=bmin, bmax=bmax, wnode=w, qnode=q), 'refit after a pose change of a creased object (%s)' % mode)
    first = np.array([0, 800, 992])
    o, d = qr.rays(pos, 4, 512)
    hits = qr.classify(pos, o, d)
    dec = hits['decided']
    assert dec.mean() >= 0.9 and (dec & hits['hit']).any() and (dec & ~hits['hit']).any()
    bad = qr.errors(hits, tree.intersect(o, d), 'creased %s' % mode, first=first)
    assert not bad, bad[:4]


# ---------------------------------------------------------------- 6: the composed model
def test_the_composed_model_is_that_of_the_plain_meshes(fresh):
    pool = _start()
    names = (('cube_inf', 2), ('grid_corners', 1), ('fan7_spokes', 2))
    objs = [pool.add_object(_add(pool, name, levels), _world(i), i % 3) for i, (name, levels) in enumerate(names)]
    pool.compose()
    got_v, got_m = pool.to_numpy()
    sphere = _sphere(pool.compose_stats())
    copies = [pool.subdivided_to_numpy(obj) for obj in objs]
    for (name, levels), copy in zip(names, copies):
        _differ(copy, ref.fixture_subdivided(name, levels), name)
    plain = _start()
    plain.load_meshes([(*deform_ref.split(copy), _world(i), i % 3) for i, copy in enumerate(copies)])
    want_v, want_m = plain.to_numpy()
    assert _same(got_v, want_v) and np.array_equal(got_m, want_m) and got_v.shape[0] == 3 * (192 + 200 + 224)
    assert sphere == _sphere(plain.compose_stats())


# ---------------------------------------------------------------- 7: the worker facade
def test_worker_facade_through_the_thread_proxy(fresh):
    import threading
    from ptina_amd.common import reset_all
    from ptina_amd.tools.mtworker import DaemonModule, OnDemandProxy
    from ptina_amd.tools.crease import blender_crease
    reset_all()
    rec, creases, corners = ref.fixture('grid_corners')
    soft = np.where(creases > 0, blender_crease(0.4), np.float32(0)).astype(np.float32)      # 1.6: sharp, fractional, smooth
    seen = []

    def module():
        seen.append(threading.get_ident())
        from ptina_amd import worker
        ns = types.SimpleNamespace(**{k: getattr(worker, k) for k in dir(worker) if not k.startswith('_')})
        ns.add_mesh = lambda: worker.ModelPool().add_mesh(*deform_ref.split(rec))
        ns.add_object = lambda mesh: worker.ModelPool().add_object(mesh, _world(1))
        ns.fetch = lambda obj: worker.ModelPool().subdivided_to_numpy(obj)
        return ns
    w = OnDemandProxy(lambda: DaemonModule(module))
    w.init()
    a, b, c = w.add_mesh(), w.add_mesh(), w.add_mesh()
    w.set_mesh_subdivision(mesh=a, levels=2, creases=soft, corners=corners)
    w.set_mesh_subdivision(b, 3, creases)
    w.set_mesh_subdivision(c, 1)
    objs = [w.add_object(m) for m in (a, b, c)]
    assert seen and seen[0] != threading.get_ident()
    w.compose_model()
    _differ(w.fetch(objs[0]), ref.subdivide(rec, 2, soft, corners), 'soft creases through the worker')
    _differ(w.fetch(objs[1]), ref.fixture_subdivided('grid_line', 3), 'creases alone through the worker')
    _differ(w.fetch(objs[2]), sr.fixture_subdivided('grid', 1), 'no creases through the worker')
    w.synchronize()

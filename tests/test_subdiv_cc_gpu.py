'''
GPU tests (-m gpu) of Catmull-Clark subdivision of quad and polygon cages on the device (ModelPool.add_subdivision with
scheme='catmull-clark', mpt_mesh_set_subdivision_cc; ptina_amd/csrc/subdiv.hip, subdiv_walk.h, scene_subdiv.cpp; DESIGN.md section
3.19.2).

The kernels are held to tests/subdiv_cc_ref.py BIT FOR BIT with no margin, as tests/test_subdiv_gpu.py holds Loop's to subdiv_ref:
both sides evaluate the same expressions in f64 in the same order and round to f32 once.  The largest job is the 25-quad grid at
level 3 (3200 faces: 12 blocks and a tail); the cube at level 3 has 768 faces and ends on a block boundary.  A compose takes
L_max + 2 launches of subdiv.hip whatever the schemes and the number of copies: the face points are lanes of the refine launches.
'''

import types

import numpy as np
import pytest

import deform_ref
import displace_ref
import subdiv_ref as sr
import subdiv_crease_ref as scr
import subdiv_cc_ref as ref
from test_subdiv_gpu import _start, _ctx, _same, _differ, _launches, _world, _sphere, _pose, _set_pose, EYE

pytestmark = pytest.mark.gpu
u32 = np.uint32
CC = 'catmull-clark'


def _add(pool, name, levels, rig=None):
    rec, polys, creases, corners = ref.fixture(name)
    mesh = pool.add_mesh(*deform_ref.split(rec))
    if rig is not None:
        pool.add_morph_targets(mesh, rig['dp'], rig['dn'])
        pool.add_skin(mesh, rig['jt'], rig['wt'], rig['nj'])
    pool.add_subdivision(mesh, levels, creases=creases, corners=corners, scheme=CC, polys=polys)
    return mesh


def _grid_rig(seed):
    g = np.random.default_rng(seed)
    dp, dn, jt, wt = deform_ref.random_rig(g, 50, 2, 4)
    return dict(T=2, nj=4, dp=dp, dn=dn, jt=jt, wt=wt, deltas=np.ascontiguousarray(np.concatenate([dp.reshape(2, 150, 3), dn.reshape(2, 150, 3)], axis=2)),
                joints=jt.reshape(150, 4), weights=wt.reshape(150, 4))


def _posed(name, levels, rig, pose):
    rec = ref.fixture(name)[0]
    control = deform_ref.deform(rec, rig['deltas'], pose[0], rig['joints'], rig['weights'], pose[1])
    return ref.records_of(rec, ref.fixture_topology(name, levels), ref.positions(rec, ref.fixture_topology(name, levels), control)[-1], control)


def _faces(name, levels):
    return 2 * int(ref.fixture(name)[1].sum()) * 4 ** (levels - 1)


# ---------------------------------------------------------------- 1: every fixture, bit for bit
@pytest.mark.parametrize('levels', [1, 2, 3])
def test_copies_equal_the_restatement_bit_for_bit(fresh, levels):
    pool = _start()
    names = ref.NAMES + ref.CREASED
    objs = [pool.add_object(_add(pool, name, levels), _world(i), i % 3) for i, name in enumerate(names)]
    pool.compose()
    assert _launches() == levels + 2
    for name, obj in zip(names, objs):
        want = ref.fixture_subdivided(name, levels)
        assert want.shape[0] == 3 * _faces(name, levels)
        _differ(pool.subdivided_to_numpy(obj), want, '%s at level %d' % (name, levels))
    assert pool.nfaces == sum(_faces(name, levels) for name in names)
    if levels == 3:
        assert _faces('grid', 3) == 3200 == 12 * sr.CHUNK + 128 and _faces('cube', 3) == 768 == 3 * sr.CHUNK
    info = pool.subdiv_stats()
    assert (info.copies, info.refined_copies, info.refined_faces) == (len(names), len(names), pool.nfaces)


@pytest.mark.parametrize('levels', [1, 2, 3])
def test_inf_cube_stays_the_cube(fresh, levels):
    '''every position lies on the cube, the eight corners stay, every corner normal is exactly the axis of the cube face its triangle
    lies in, and a cube corner carries three normals'''
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
        assert here.sum() == 6 and np.unique(flat_n[here], axis=0).shape[0] == 3


@pytest.mark.parametrize('levels', [1, 2, 3])
def test_a_planar_pentagon_stays_planar(fresh, levels):
    from ptina_amd.tools.polys import fan
    ang = 2 * np.pi * np.arange(5) / 5
    p = np.stack([np.cos(ang), np.sin(ang), np.zeros(5)], axis=1)
    rec, polys = fan([range(5)], p, t=0.5 + 0.25 * p[:, :2])
    assert rec.shape == (9, 8) and polys.tolist() == [5]
    pool = _start()
    mesh = pool.add_mesh(*deform_ref.split(rec))
    pool.add_subdivision(mesh, levels, scheme=CC, polys=polys)
    obj = pool.add_object(mesh, EYE)
    pool.compose()
    got = pool.subdivided_to_numpy(obj)
    assert got.shape[0] == 3 * 10 * 4 ** (levels - 1)
    assert (got[:, 2] == 0).all() and np.array_equal(got[:, 3:6], np.tile(np.float32([0, 0, 1]), (got.shape[0], 1)))
    _differ(got, ref.subdivide(rec, levels, polys), 'the planar pentagon')


# ---------------------------------------------------------------- 2: no crease, no difference; the schemes side by side
def test_zero_creases_equal_the_uncreased_call_record_for_record(fresh):
    pool = _start()
    objs = []
    for i, (name, levels) in enumerate((('grid', 3), ('cap5', 2), ('pyramid', 1))):
        rec, polys, _, _ = ref.fixture(name)
        n = int(polys.sum())
        for creases, corners in ((None, None), (np.zeros(n, np.float32), None), (None, np.zeros(n, bool)), (np.zeros(n), np.zeros(n, np.uint8))):
            mesh = pool.add_mesh(*deform_ref.split(rec))
            pool.add_subdivision(mesh, levels, creases=creases, corners=corners, scheme=CC, polys=polys)
            objs.append((name, levels, pool.add_object(mesh, _world(i))))
    pool.compose()
    plain = {}
    for name, levels, obj in objs:
        got = pool.subdivided_to_numpy(obj)
        _differ(got, ref.fixture_subdivided(name, levels), 'zero creases on %s' % name)
        assert _same(got, plain.setdefault(name, got))
    assert _launches() == 5


def test_triangles_without_polys_are_polygons_of_their_own(fresh):
    pool = _start()
    rec = sr.fixture('octahedron')
    mesh = pool.add_mesh(*deform_ref.split(rec))
    pool.add_subdivision(mesh, 2, scheme=CC)
    obj = pool.add_object(mesh, EYE)
    pool.compose()
    _differ(pool.subdivided_to_numpy(obj), ref.subdivide(rec, 2), 'the octahedron, every triangle a polygon')
    assert pool.nfaces == 2 * 24 * 4


def test_loop_creased_loop_and_catmull_clark_in_one_compose(fresh):
    '''meshes of both schemes and of different levels share the launches: L_max + 2 of them'''
    pool = _start()
    mesh = pool.add_mesh(*deform_ref.split(sr.fixture('icosahedron')))
    pool.add_subdivision(mesh, 2)
    a = pool.add_object(mesh, _world(1))
    rec, creases, corners = scr.fixture('grid_corners')
    mesh = pool.add_mesh(*deform_ref.split(rec))
    pool.add_subdivision(mesh, 1, creases=creases, corners=corners)
    b = pool.add_object(mesh, _world(2))
    c = pool.add_object(_add(pool, 'cap5', 3), _world(3))
    d = pool.add_object(_add(pool, 'grid_corners', 2), _world(4))
    e = pool.add_object(_add(pool, 'pentagon', 1), _world(5))
    pool.compose()
    assert _launches() == 3 + 2
    _differ(pool.subdivided_to_numpy(a), sr.fixture_subdivided('icosahedron', 2), 'the Loop mesh')
    _differ(pool.subdivided_to_numpy(b), scr.fixture_subdivided('grid_corners', 1), 'the creased Loop grid')
    _differ(pool.subdivided_to_numpy(c), ref.fixture_subdivided('cap5', 3), 'the cap')
    _differ(pool.subdivided_to_numpy(d), ref.fixture_subdivided('grid_corners', 2), 'the creased quad grid')
    _differ(pool.subdivided_to_numpy(e), ref.fixture_subdivided('pentagon', 1), 'the pentagon')
    info = pool.subdiv_stats()
    assert (info.copies, info.refined_copies, info.refined_faces) == (5, 5, 20 * 16 + 50 * 4 + _faces('cap5', 3) + 800 + 10)
    pool.compose()
    assert _launches() == 0


# ---------------------------------------------------------------- 3: behind the deformation
def test_a_skinned_grid_and_set_world(fresh):
    '''two objects of the skinned quad grid, each in its pose; one posed again: it alone is refined again; set_world alone refines
    nothing'''
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
    pool.set_world(objs[0], _world(9))
    pool.compose()
    info = pool.subdiv_stats()
    assert (info.refined_copies, info.refined_faces) == (0, 0) and _launches() == 0 and pool.compose_stats().dirty_objects == 1


# ---------------------------------------------------------------- 4: a displacement and a scatter behind it
def _vertex_uv(rec, topo):
    '''[V_L,2] f64: the uv of every last-level vertex's first corner among the emitted triangles'''
    vert = np.array([r[0] for r in topo['records']], np.int64)[topo['faces'].reshape(-1)]
    first = displace_ref.first_corners(vert, len(topo['rings']))
    return ref.face_uvs(rec, topo).reshape(-1, 2)[first], vert, first


@pytest.mark.parametrize('mode', ['normal', 'vector'])
def test_a_displaced_grid(fresh, mode):
    from ptina_amd.things import ImagePool
    image = displace_ref.random_image(3, 9, 7)
    levels, strength, midlevel = 2, 0.3, 0.4
    rec, polys, creases, corners = ref.fixture('grid_corners')
    topo = ref.fixture_topology('grid_corners', levels)
    P = ref.fixture_positions('grid_corners', levels)[-1]
    uv, vert, first = _vertex_uv(rec, topo)
    rgba = displace_ref.sample(image, uv[:, 0], uv[:, 1])
    if mode == 'normal':
        n = sr.normals(P, topo['rings'])                                  # the whole ring of edge neighbours: one direction per vertex
        Pd = P + (strength * (displace_ref.height(rgba, displace_ref.MEAN) - midlevel))[:, None] * n
    else:
        Pd = P + strength * (rgba[:, :3] - midlevel)
    want = ref.records_of(rec, topo, Pd)
    pool = _start()
    ImagePool().load([image])
    mesh = pool.add_mesh(*deform_ref.split(rec))
    pool.add_subdivision(mesh, levels, creases=creases, corners=corners, scheme=CC, polys=polys)
    pool.add_displacement(mesh, 0, strength, midlevel, mode, 'mean')
    obj = pool.add_object(mesh, EYE)
    pool.compose()
    got = pool.subdivided_to_numpy(obj)
    _differ(got, want, 'quad grid displaced (%s)' % mode)
    assert not _same(got, ref.fixture_subdivided('grid_corners', levels))
    assert np.array_equal(got[:, :3].view(u32), got[first[vert], :3].view(u32))      # no crack
    assert len(topo['records']) > P.shape[0]


def test_a_scatter_over_a_catmull_clark_surface(fresh):
    import scatter_ref as sc
    import test_displace_gpu as dg
    from test_scatter_gpu import IMAGES, TUFT, _check, _plain
    pool = _start()
    dg._load_images(IMAGES)
    surf = pool.add_object(_add(pool, 'cap5', 2), sc.BENT, 1)
    tuft = _plain(pool, TUFT)
    sid, objs = pool.add_scatter(surf, tuft, 64, seed=sc.SEED, mtlid=2, scale=(0.05, 0.2))
    assert objs == range(1, 65)
    pool.compose()
    rec = ref.fixture_subdivided('cap5', 2)
    assert pool.nfaces == rec.shape[0] // 3 + 64 * 4
    points, _, q = _check(pool, sid, rec, sc.BENT, sc.SEED, 64, 'the cap at level 2', scale=(0.05, 0.2))
    assert (q[points['face']] > 0).all()


# ---------------------------------------------------------------- 5: the composed model; build, pose, compose, update
def test_the_composed_model_is_that_of_the_plain_meshes(fresh):
    pool = _start()
    names = (('cube_inf', 2), ('grid_corners', 1), ('cap5', 2), ('pyramid', 3))
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
    assert _same(got_v, want_v) and np.array_equal(got_m, want_m) and got_v.shape[0] == 3 * sum(_faces(n, l) for n, l in names)
    assert sphere == _sphere(plain.compose_stats())


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
    _same_records(got, dict(built, bmin=bmin, bmax=bmax, wnode=w, qnode=q), 'refit after a pose change of a Catmull-Clark object (%s)' % mode)
    first = np.array([0, 800, 992])
    o, d = qr.rays(pos, 4, 512)
    hits = qr.classify(pos, o, d)
    dec = hits['decided']
    assert dec.mean() >= 0.9 and (dec & hits['hit']).any() and (dec & ~hits['hit']).any()
    bad = qr.errors(hits, tree.intersect(o, d), 'catmull-clark %s' % mode, first=first)
    assert not bad, bad[:4]


# ---------------------------------------------------------------- 6: refusals, the copies' room, the worker
def test_refusals_through_the_pool(fresh):
    from test_subdiv_cc_cpu import REFUSALS
    pool = _start()
    c = _ctx()
    for kind, (code, words, make) in sorted(REFUSALS.items()):
        rec, polys, creases = make()
        mesh = pool.add_mesh(*deform_ref.split(rec))
        with pytest.raises(RuntimeError, match='mpt_mesh_set_subdivision_cc: mesh %d: subdivision: .*%s' % (mesh, words)):
            pool.add_subdivision(mesh, 2, creases=creases, scheme=CC, polys=polys)
    rec, polys, creases, _ = ref.fixture('cube_1p5')
    good = pool.add_mesh(*deform_ref.split(rec))
    with pytest.raises(ValueError, match="scheme 'bilinear': one of loop, catmull-clark"):
        pool.add_subdivision(good, 2, scheme='bilinear')
    with pytest.raises(ValueError, match="polys are the polygons of scheme 'catmull-clark'"):
        pool.add_subdivision(good, 2, polys=polys)
    with pytest.raises(ValueError, match=r'creases must be \[24\]'):
        pool.add_subdivision(good, 2, creases=np.zeros((12, 3)), scheme=CC, polys=polys)
    with pytest.raises(ValueError, match=r'corners must be \[24\]'):
        pool.add_subdivision(good, 2, corners=np.zeros(23), scheme=CC, polys=polys)
    with pytest.raises(ValueError):
        pool.add_subdivision(good, 6, scheme=CC, polys=polys)
    from ptina_amd._lib import iptr
    with pytest.raises(RuntimeError, match=r'mpt_mesh_set_subdivision_cc: levels 0 outside \[1, 5\]'):
        c.call('mpt_mesh_set_subdivision_cc', good, 0, iptr(np.ascontiguousarray(polys)), 6, None, None)
    with pytest.raises(RuntimeError, match='unknown mesh'):
        c.call('mpt_mesh_set_subdivision_cc', 99, 1, None, 0, None, None)
    big_rec, big_polys = ref.fan_records(*ref.grid(32, 32))                # 1024 quads: 2 * 4096 * 4^4 = 2^21 at level 5
    big = pool.add_mesh(*deform_ref.split(big_rec))
    with pytest.raises(RuntimeError, match='too many faces: 2097152 at level 5'):
        c.call('mpt_mesh_set_subdivision_cc', big, 5, iptr(np.ascontiguousarray(big_polys)), 1024, None, None)
    with pytest.raises(ValueError, match='too many faces'):
        pool.add_subdivision(big, 5, scheme=CC, polys=big_polys)
    pool.add_subdivision(good, 2, creases=creases, scheme=CC, polys=polys)     # (the refusals left the mesh without a level)
    with pytest.raises(RuntimeError, match='already has a subdivision level'):
        c.call('mpt_mesh_set_subdivision_cc', good, 1, None, 0, None, None)
    obj = pool.add_object(good, EYE)
    with pytest.raises(RuntimeError, match='already has an object'):
        c.call('mpt_mesh_set_subdivision', good, 1)
    pool.compose()
    with pytest.raises(RuntimeError, match='room for 3 faces'):
        c.call('mpt_get_subdivided', obj, None, 3)
    _differ(pool.subdivided_to_numpy(obj), ref.fixture_subdivided('cube_1p5', 2), 'after the refusals')
    assert pool.nfaces == 192


def test_clear_and_mesh_add_while_copies_exist(fresh):
    pool = _start()
    mc, mi = _add(pool, 'cylinder', 2), _add(pool, 'cap5', 1)
    oc, oi = pool.add_object(mc, _world(1)), pool.add_object(mi, _world(2))
    pool.compose()
    want_c, want_i = ref.fixture_subdivided('cylinder', 2), ref.fixture_subdivided('cap5', 1)
    _differ(pool.subdivided_to_numpy(oc), want_c, 'cylinder')
    assert pool.subdiv_stats().copy_verts == 3 * (512 + _faces('cap5', 1))
    mg = _add(pool, 'grid', 3)                                            # a mesh joins the pool where the copies lay
    assert pool.subdiv_stats().copy_verts == 0
    with pytest.raises(RuntimeError, match='no subdivided copy yet'):
        pool.subdivided_to_numpy(oc)
    og = pool.add_object(mg, _world(3))
    pool.compose()
    info = pool.subdiv_stats()
    assert (info.copies, info.refined_copies, info.copy_verts) == (3, 3, 3 * (512 + _faces('cap5', 1) + 3200))
    _differ(pool.subdivided_to_numpy(oc), want_c, 'cylinder after a mesh was added')
    _differ(pool.subdivided_to_numpy(oi), want_i, 'cap after a mesh was added')
    _differ(pool.subdivided_to_numpy(og), ref.fixture_subdivided('grid', 3), 'the new grid')
    pool.clear_objects()                                                  # the copies go, the meshes and their levels stay
    info = pool.subdiv_stats()
    assert (info.subdivided_objects, info.copies, info.copy_verts) == (0, 0, 0)
    oi = pool.add_object(mi, _world(4))
    oi2 = pool.add_object(mi, _world(5))
    pool.compose()
    info = pool.subdiv_stats()
    assert (info.subdivided_objects, info.copies, info.copy_verts, pool.nfaces) == (2, 1, 3 * _faces('cap5', 1), 2 * _faces('cap5', 1))
    _differ(pool.subdivided_to_numpy(oi2), want_i, 'cap after clear_objects')
    pool.clear_meshes()                                                   # everything goes; a new mesh starts from nothing
    assert pool.subdiv_stats().copies == 0
    obj = pool.add_object(_add(pool, 'pyramid', 2), EYE)
    pool.compose()
    _differ(pool.subdivided_to_numpy(obj), ref.fixture_subdivided('pyramid', 2), 'pyramid after clear_meshes')
    assert pool.nfaces == _faces('pyramid', 2)


def test_worker_facade_through_the_thread_proxy(fresh):
    import threading
    from ptina_amd.common import reset_all
    from ptina_amd.tools.mtworker import DaemonModule, OnDemandProxy
    from ptina_amd.tools.crease import blender_crease
    reset_all()
    rec, polys, creases, corners = ref.fixture('grid_corners')
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
    w.set_mesh_subdivision(mesh=a, levels=2, creases=soft, corners=corners, scheme=CC, polys=polys)
    w.set_mesh_subdivision(b, 3, creases, None, CC, polys)
    w.set_mesh_subdivision(c, 1, scheme=CC, polys=polys)
    objs = [w.add_object(m) for m in (a, b, c)]
    assert seen and seen[0] != threading.get_ident()
    w.compose_model()
    _differ(w.fetch(objs[0]), ref.subdivide(rec, 2, polys, soft, corners), 'soft creases through the worker')
    _differ(w.fetch(objs[1]), ref.fixture_subdivided('grid_line', 3), 'creases alone through the worker')
    _differ(w.fetch(objs[2]), ref.fixture_subdivided('grid', 1), 'no creases through the worker')
    w.synchronize()

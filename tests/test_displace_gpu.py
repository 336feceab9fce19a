'''
GPU tests (-m gpu) of texture displacement of subdivided meshes on the device (ModelPool.add_displacement / set_displacement /
displace_stats, mpt_mesh_set_displacement ... mpt_displace_kernel_time; ptina_amd/csrc/displace.hip, scene_subdiv.cpp; DESIGN.md
section 3.20).

The kernel is held to tests/displace_ref.py BIT FOR BIT, NaN positions included, with no margin (test_subdiv_gpu.py's _differ):
both sides evaluate the same expressions in f64 in the same order, every operation a correctly rounded IEEE + - * / sqrt floor,
and round to f32 once.  A workgroup takes 256 vertices of one copy's last level: the grid at level 3 has 1681 (six blocks and a tail
of 145), the tetrahedron at level 1 is a job far smaller than a block.  The images are 4 x 3 and 5 x 7 (not square: an x / y swap
cannot pass), the uvs the fixtures' own and those scaled to 3 uv - 1.25, which leave the image on both sides.
'''

import types

import numpy as np
import pytest

import deform_ref
import displace_ref as dr
import subdiv_ref as sr
from test_subdiv_gpu import EYE, _ctx, _deformed, _differ, _pose, _rig, _same, _set_pose, _sphere, _start, _world

pytestmark = pytest.mark.gpu

IMAGES = [dr.random_image(11, 4, 3), dr.random_image(12, 5, 7)]
CHANNELS = ('r', 'g', 'b', 'a', 'mean')
MODES = ('normal', 'vector')


def _load_images(images=IMAGES):
    from ptina_amd.things import ImagePool
    ImagePool().load(list(images))


def _records(name, scaled):
    return dr.scaled_uv(sr.fixture(name)) if scaled else sr.fixture(name)


def _add(pool, name, levels, disp, rig=None, scaled=False):
    '''a mesh of fixture `name` with its level, its rig and -- disp = (image, mode, channel, strength, midlevel) or None -- its
    displacement (before the rig when the rig says 'levels' first)'''
    mesh = pool.add_mesh(*deform_ref.split(_records(name, scaled)))
    pool.add_subdivision(mesh, levels)
    early = rig is not None and rig['first'] == 'levels'
    if disp is not None and early:
        pool.add_displacement(mesh, disp[0], disp[3], disp[4], MODES[disp[1]], CHANNELS[disp[2]])
    if rig is not None:
        pool.add_morph_targets(mesh, rig['dp'], rig['dn'])
        pool.add_skin(mesh, rig['jt'], rig['wt'], rig['nj'])
    if disp is not None and not early:
        pool.add_displacement(mesh, disp[0], disp[3], disp[4], MODES[disp[1]], CHANNELS[disp[2]])
    return mesh


def _expected(name, levels, disp, rig=None, pose=None, scaled=False, images=IMAGES):
    rec = _records(name, scaled)
    topo = sr.fixture_topology(name, levels)                              # (the topology is the positions': the scaled records share it)
    control = None
    if rig is not None:
        control = deform_ref.deform(rec, rig['deltas'], pose[0], rig['joints'], rig['weights'], pose[1])
    if disp is None:
        return sr.subdivide(rec, levels, topo, control=control)
    return dr.displace(rec, levels, images[disp[0]], disp[1], disp[2], disp[3], disp[4], control=control, topo=topo)


def _launches():
    *ms, n = _ctx().timer('mpt_subdiv_kernel_time', 3)
    ms_d, n_d = _ctx().timer('mpt_displace_kernel_time')
    assert all(m >= 0 for m in ms) and ms_d >= 0
    return n, n_d


def _stats(pool):
    s = pool.displace_stats()
    return s.displaced_meshes, s.copies, s.displaced_copies, s.displaced_verts


def _nverts(name, levels):
    return len(sr.fixture_topology(name, levels)['rings'])


# ---------------------------------------------------------------- 1: fixtures, modes and block shapes
@pytest.mark.parametrize('levels', [1, 2, 3])
def test_displaced_copies_equal_the_restatement_bit_for_bit(fresh, levels):
    '''every fixture in both modes; over the fixtures the normal mode sees the channels r, a and mean, and each mode both images and
    both uv scalings'''
    pool = _start()
    _load_images()
    ch = (dr.R, dr.A, dr.MEAN)
    cases = []
    for i, name in enumerate(sr.NAMES):
        cases.append((name, (i % 2, dr.NORMAL, ch[i % 3], 0.35, 0.5), i // 2 % 2 == 1))
        cases.append((name, ((i + 1) % 2, dr.VECTOR, ch[(i + 1) % 3], -0.6, 0.25), i // 2 % 2 == 0))
    assert {(d[1], d[0], s) for _, d, s in cases} == {(m, im, s) for m in (0, 1) for im in (0, 1) for s in (False, True)}
    assert {d[2] for _, d, _ in cases if d[1] == dr.NORMAL} == set(ch)
    objs = [pool.add_object(_add(pool, name, levels, disp, scaled=scaled), _world(i), i % 3) for i, (name, disp, scaled) in enumerate(cases)]
    pool.compose()
    verts = 0
    for (name, disp, scaled), obj in zip(cases, objs):
        want = _expected(name, levels, disp, scaled=scaled)
        plain = sr.fixture_subdivided(name, levels)
        assert want.shape == plain.shape and not _same(want[:, :3], plain[:, :3])
        _differ(pool.subdivided_to_numpy(obj), want, '%s at level %d, %s' % (name, levels, disp))
        verts += _nverts(name, levels)
    if levels == 3:
        assert _nverts('grid', 3) == 1681 == 6 * sr.CHUNK + 145
    if levels == 1:
        assert _nverts('tetrahedron', 1) == 10
    n = len(cases)
    assert _stats(pool) == (n, n, n, verts)
    assert _launches() == (levels + 2, 1)
    pool.compose()                                                        # nothing changed: nothing launched
    assert _launches() == (0, 0) and _stats(pool) == (n, n, 0, 0)


# ---------------------------------------------------------------- 2: a mixed compose
def test_mixed_compose_takes_one_displacement_launch(fresh):
    pool = _start()
    _load_images()
    scene = [('grid', 3, (0, dr.NORMAL, dr.MEAN, 0.4, 0.5)), ('icosahedron', 1, (1, dr.VECTOR, dr.R, 0.3, 0.5)), ('fan7', 2, (1, dr.NORMAL, dr.G, -0.8, 0.1)),
             ('cylinder', 2, None)]
    objs = [pool.add_object(_add(pool, name, L, disp), _world(i)) for i, (name, L, disp) in enumerate(scene)]
    plain = pool.add_object(pool.add_mesh(*deform_ref.split(sr.fixture('octahedron'))), _world(7))
    pool.compose()
    assert _launches() == (3 + 2, 1)
    for (name, L, disp), obj in zip(scene, objs):
        _differ(pool.subdivided_to_numpy(obj), _expected(name, L, disp), '%s at level %d beside the others' % (name, L))
    _differ(pool.subdivided_to_numpy(objs[3]), sr.fixture_subdivided('cylinder', 2), 'the copy without a displacement')
    with pytest.raises(RuntimeError, match='no subdivision level'):
        pool.subdivided_to_numpy(plain)
    assert _stats(pool) == (3, 3, 3, _nverts('grid', 3) + _nverts('icosahedron', 1) + _nverts('fan7', 2))
    assert pool.subdiv_stats().refined_copies == 4 and pool.nfaces == 50 * 64 + 20 * 4 + 14 * 16 + 32 * 16 + 8


# ---------------------------------------------------------------- 3: behind skinning and morphing
def test_displacement_behind_skinning_and_morphing(fresh):
    '''poses from deform_ref that pull welded corners apart: positions and uvs are read from the deformed copy, the first corner
    speaks for its vertex.  Two objects of one mesh in different poses; one posed again: it alone is displaced again'''
    pool = _start()
    _load_images()
    rigs = dict(grid=_rig('grid', 1, first='levels'), cylinder=_rig('cylinder', 2))
    disp = dict(grid=(1, dr.NORMAL, dr.A, 0.3, 0.45), cylinder=(0, dr.VECTOR, dr.R, 0.25, 0.5))
    mg = _add(pool, 'grid', 2, disp['grid'], rigs['grid'])
    mc = _add(pool, 'cylinder', 2, disp['cylinder'], rigs['cylinder'], scaled=True)
    names = ['grid', 'cylinder', 'grid']
    objs = [pool.add_object(m, _world(20 + i), i % 3) for i, m in enumerate((mg, mc, mg))]
    poses = [_pose(41), _pose(42), _pose(43)]
    for obj, pose in zip(objs, poses):
        _set_pose(pool, obj, pose)
    pool.compose()

    def check(what):
        for o, name in enumerate(names):
            want = _expected(name, 2, disp[name], rigs[name], poses[o], scaled=name == 'cylinder')
            _differ(pool.subdivided_to_numpy(objs[o]), want, 'posed object %d %s' % (o, what))
    check('at first')
    copy = pool.deformed_to_numpy(objs[0])
    assert _same(copy, _deformed('grid', rigs['grid'], poses[0]))
    faces, first = sr.weld(sr.fixture('grid'))
    apart = [v for v in range(first.size) if np.unique(copy[np.flatnonzero(faces.reshape(-1) == v), :3], axis=0).shape[0] > 1]
    assert len(apart) > 10, 'the pose leaves the welded corners together'
    assert not _same(pool.subdivided_to_numpy(objs[0]), pool.subdivided_to_numpy(objs[2])), 'two objects of one mesh share a pose'
    assert _stats(pool) == (2, 3, 3, 2 * _nverts('grid', 2) + _nverts('cylinder', 2)) and _launches() == (4, 1)
    poses[2] = _pose(99)
    _set_pose(pool, objs[2], poses[2])
    pool.compose()
    assert _stats(pool) == (2, 3, 1, _nverts('grid', 2)) and _launches() == (4, 1)
    assert pool.subdiv_stats().refined_copies == 1 and pool.deform_stats().deformed_objects == 1
    check('after object 2 was posed again')


# ---------------------------------------------------------------- 4: set_displacement on a rigid mesh with three objects
def test_set_displacement_on_a_rigid_mesh_with_three_objects(fresh):
    pool = _start()
    _load_images()
    disp = (1, dr.NORMAL, dr.MEAN, 0.5, 0.5)
    mesh = _add(pool, 'fan12', 2, disp)
    other = _add(pool, 'pair', 1, None)
    objs = [pool.add_object(mesh, _world(i), i) for i in range(3)] + [pool.add_object(other, _world(5), 1)]
    pool.compose()
    assert _stats(pool) == (1, 1, 1, _nverts('fan12', 2)) and _launches() == (4, 1)

    def check(disp, what):
        want = _expected('fan12', 2, disp)
        for obj in objs[:3]:
            _differ(pool.subdivided_to_numpy(obj), want, 'object %d of the shared copy %s' % (obj, what))
        got_v, got_m = pool.to_numpy()
        sphere = _sphere(pool.compose_stats())
        return want, got_v, got_m, sphere
    first = check(disp, 'at first')
    pool.set_displacement(mesh, -0.3)                                     # (the midlevel stays)
    pool.compose()
    c = pool.compose_stats()
    assert _stats(pool) == (1, 1, 1, _nverts('fan12', 2)) and _launches() == (2 + 2, 1) and (c.dirty_objects, c.recomposed) == (3, 3 * 384)
    second = check((1, dr.NORMAL, dr.MEAN, -0.3, 0.5), 'after set_displacement')
    assert not _same(first[0], second[0])
    pool.set_displacement(mesh, 0.7, 0.2)
    pool.compose()
    third = check((1, dr.NORMAL, dr.MEAN, 0.7, 0.2), 'after set_displacement with a midlevel')
    assert _launches() == (4, 1)
    pool.set_world(objs[1], _world(9))
    pool.compose()
    assert _stats(pool) == (1, 1, 0, 0) and _launches() == (0, 0) and pool.compose_stats().dirty_objects == 1
    pool.set_world(objs[1], _world(1))
    pool.compose()
    assert _same(pool.to_numpy()[0], third[1])
    # the composed model: what load_meshes makes of plain meshes made from the restatement, bounding sphere included
    small = sr.fixture_subdivided('pair', 1)
    for want, got_v, got_m, sphere in (first, second, third):
        plain = _start()
        plain.load_meshes([(*deform_ref.split(want), _world(i), i) for i in range(3)] + [(*deform_ref.split(small), _world(5), 1)])
        want_v, want_m = plain.to_numpy()
        assert _same(got_v, want_v) and np.array_equal(got_m, want_m) and got_v.shape[0] == 3 * (3 * 384 + 8)
        assert sphere == _sphere(plain.compose_stats())


# ---------------------------------------------------------------- 5: image reload
def test_image_reload_displaces_again_and_a_missing_image_refuses(fresh):
    from ptina_amd.things import ImagePool
    pool = _start()
    _load_images()
    disp = (0, dr.NORMAL, dr.R, 0.4, 0.5)
    mesh = _add(pool, 'icosahedron', 2, disp)
    still = _add(pool, 'tetrahedron', 1, None)
    obj, obj2 = pool.add_object(mesh, _world(1)), pool.add_object(still, _world(2))
    pool.compose()
    _differ(pool.subdivided_to_numpy(obj), _expected('icosahedron', 2, disp), 'first image')
    gen = pool.displace_stats().image_generation
    _launches()
    # another image of the same size in its place
    other = [dr.random_image(21, 4, 3), IMAGES[1]]
    _load_images(other)
    assert pool.displace_stats().image_generation > gen
    pool.compose()
    c = pool.compose_stats()
    assert _stats(pool) == (1, 1, 1, _nverts('icosahedron', 2)) and _launches() == (4, 1) and (c.dirty_objects, c.recomposed) == (1, 320)
    want = _expected('icosahedron', 2, disp, images=other)
    assert not _same(want, _expected('icosahedron', 2, disp))
    _differ(pool.subdivided_to_numpy(obj), want, 'second image')
    model = pool.to_numpy()[0]
    # no image: compose refuses and changes nothing
    ImagePool().load([])
    with pytest.raises(RuntimeError, match='mesh 0 reads image 0'):
        pool.compose()
    with pytest.raises(RuntimeError, match='mesh 0 reads image 0'):
        pool.compose()
    assert _launches() == (0, 0) and _same(pool.to_numpy()[0], model)
    _differ(pool.subdivided_to_numpy(obj), want, 'after the refused compose')
    # an image of another size arrives
    third = [dr.random_image(22, 6, 2)]
    _load_images(third)
    pool.compose()
    assert _stats(pool) == (1, 1, 1, _nverts('icosahedron', 2)) and _launches() == (4, 1)
    _differ(pool.subdivided_to_numpy(obj), _expected('icosahedron', 2, disp, images=third), 'third image')
    _differ(pool.subdivided_to_numpy(obj2), sr.fixture_subdivided('tetrahedron', 1), 'the copy without a displacement')
    assert not _same(pool.to_numpy()[0], model)


# ---------------------------------------------------------------- 6: a collapsed pose
def test_a_collapsed_pose_gives_nan_where_the_restatement_has_it(fresh):
    '''joint matrices of scale zero collapse a skinned cylinder onto one point: every normal sum is zero, so the normal mode moves
    every vertex to NaN; the vector mode does not ask for the normal and its positions stay numbers'''
    rig = _rig('cylinder', 2)
    mats = np.zeros((4, 4, 4))
    mats[:, :3, 3], mats[:, 3, 3] = [0.25, -1.0, 2.0], 1.0
    pose = (np.zeros(2), mats)
    dn, dv = (0, dr.NORMAL, dr.MEAN, 0.4, 0.5), (0, dr.VECTOR, dr.R, 0.4, 0.5)
    want_n, want_v = _expected('cylinder', 2, dn, rig, pose), _expected('cylinder', 2, dv, rig, pose)
    assert np.isnan(want_n[:, :6]).all() and np.isfinite(want_n[:, 6:]).all()
    assert np.isfinite(want_v[:, [0, 1, 2, 6, 7]]).all()
    pool = _start()
    _load_images()
    on, ov = pool.add_object(_add(pool, 'cylinder', 2, dn, rig), EYE), pool.add_object(_add(pool, 'cylinder', 2, dv, rig), EYE)
    _set_pose(pool, on, pose)
    _set_pose(pool, ov, pose)
    pool.compose()
    got_n, got_v = pool.subdivided_to_numpy(on), pool.subdivided_to_numpy(ov)
    _differ(got_n, want_n, 'collapsed cylinder, normal mode')
    _differ(got_v, want_v, 'collapsed cylinder, vector mode')
    assert np.isnan(got_n[:, :6]).all() and np.isfinite(got_v[:, :3]).all()


# ---------------------------------------------------------------- 7: build, strength change, compose, update: a refit
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_strength_change_then_update_refits(fresh, mode):
    import query_ref as qr
    import refit_ref
    import visibility_ref as vr
    from test_refit_gpu import _records as _tree_records, _same_records
    from ptina_amd.things import BVHTree
    pool = _start(mode)
    _load_images()
    disp = [(1, dr.NORMAL, dr.MEAN, 0.2, 0.5), (0, dr.VECTOR, dr.R, 0.1, 0.5)]
    mg, mi = _add(pool, 'grid', 2, disp[0]), _add(pool, 'icosahedron', 2, disp[1])
    mo = pool.add_mesh(*deform_ref.split(sr.fixture('octahedron')))
    objs = [pool.add_object(m, _world(10 + i), i % 3) for i, m in enumerate((mg, mi, mo))]
    pool.compose()
    nfaces = 16 * (50 + 20) + 8
    tree = BVHTree()
    tree.build()
    built = _tree_records(_ctx())
    disp[0] = (1, dr.NORMAL, dr.MEAN, 0.3, 0.5)
    pool.set_displacement(mg, 0.3)
    pool.compose()
    assert _stats(pool)[2] == 1 and pool.nfaces == nfaces and pool.compose_stats().dirty_objects == 1
    assert tree.update(max_growth=float('inf')) == 'refit' and tree.refit_stats().refits == 1 and tree.refit_stats().host_fetches == 0
    got = _tree_records(_ctx())
    model, _ = pool.to_numpy()
    want = [_expected('grid', 2, disp[0]), _expected('icosahedron', 2, disp[1]), sr.fixture('octahedron')]
    for o in (0, 1):
        _differ(pool.subdivided_to_numpy(objs[o]), want[o], 'object %d before the refit' % o)
    pos = vr.positions(model)
    assert pos.shape[0] == nfaces
    bmin, bmax, w, q = refit_ref.refit_ref(built['child'], built['leaf'], built['wnode'], built['qnode'], nfaces, pos)
    _same_records(got, dict(built, bmin=bmin, bmax=bmax, wnode=w, qnode=q), 'refit after a strength change (%s)' % mode)
    first = np.concatenate([[0], np.cumsum([x.shape[0] // 3 for x in want])])[:3]
    o, d = qr.rays(pos, 4, 512)
    ref = qr.classify(pos, o, d)
    dec = ref['decided']
    assert dec.mean() >= 0.9 and (dec & ref['hit']).any() and (dec & ~ref['hit']).any()
    bad = qr.errors(ref, tree.intersect(o, d), 'displaced %s' % mode, first=first)
    assert not bad, bad[:4]


# ---------------------------------------------------------------- 8: refusals
def test_refusals_say_what_is_wrong_and_leave_the_scene(fresh):
    pool = _start()
    _load_images()
    c = _ctx()
    disp = (0, dr.NORMAL, dr.MEAN, 0.4, 0.5)
    good = _add(pool, 'octahedron', 1, None)
    flat = pool.add_mesh(*deform_ref.split(sr.fixture('pair')))

    def call(mesh, image=0, mode=0, channel=4, strength=0.4, midlevel=0.5):
        c.call('mpt_mesh_set_displacement', mesh, image, mode, channel, strength, midlevel)
    with pytest.raises(RuntimeError, match='unknown mesh 99'):
        call(99)
    with pytest.raises(RuntimeError, match='displacement needs a subdivided mesh'):
        call(flat)
    for mode in (-1, 2):
        with pytest.raises(RuntimeError, match=r'mode %d outside \[0, 1\]' % mode):
            call(good, mode=mode)
    for channel in (-1, 5):
        with pytest.raises(RuntimeError, match=r'channel %d outside \[0, 4\]' % channel):
            call(good, channel=channel)
    with pytest.raises(RuntimeError, match='image id -1 is negative'):
        call(good, image=-1)
    for bad in (float('nan'), float('inf'), -float('inf')):
        with pytest.raises(RuntimeError, match='strength is not finite'):
            call(good, strength=bad)
        with pytest.raises(RuntimeError, match='midlevel is not finite'):
            call(good, midlevel=bad)
    # the uvs: finite and at most 2^20 in magnitude, the corner named
    for value, ok in ((np.nan, False), (np.inf, False), (2.0 ** 20 + 1, False), (-2.0 ** 20 - 1, False), (2.0 ** 20, True), (-2.0 ** 20, True)):
        rec = np.array(sr.fixture('octahedron'))
        rec[3 * 2 + 1, 7] = value
        mesh = pool.add_mesh(*deform_ref.split(rec))
        pool.add_subdivision(mesh, 1)
        if ok:
            call(mesh)
            continue
        with pytest.raises(RuntimeError, match='the uv of corner 1 of face 2 is not finite or exceeds 2\\^20'):
            call(mesh)
    # the Python side keeps the books add_subdivision keeps
    with pytest.raises(ValueError, match='unknown mesh'):
        pool.add_displacement(99, 0)
    with pytest.raises(ValueError, match='needs a subdivided mesh'):
        pool.add_displacement(flat, 0)
    with pytest.raises(ValueError, match='mode'):
        pool.add_displacement(good, 0, mode='tangent')
    with pytest.raises(ValueError, match='channel'):
        pool.add_displacement(good, 0, channel='luma')
    with pytest.raises(ValueError, match='negative'):
        pool.add_displacement(good, -1)
    with pytest.raises(ValueError, match='finite'):
        pool.add_displacement(good, 0, strength=float('nan'))
    with pytest.raises(ValueError, match='has no displacement'):
        pool.set_displacement(good, 1.0)
    with pytest.raises(RuntimeError, match='mesh %d has no displacement' % good):
        c.call('mpt_mesh_set_displacement_params', good, 1.0, 0.5)
    with pytest.raises(RuntimeError, match='unknown mesh 99'):
        c.call('mpt_mesh_set_displacement_params', 99, 1.0, 0.5)
    pool.add_displacement(good, *disp[:1], disp[3], disp[4], MODES[disp[1]], CHANNELS[disp[2]])
    with pytest.raises(RuntimeError, match='already has a displacement'):
        call(good)
    with pytest.raises(ValueError, match='already has a displacement'):
        pool.add_displacement(good, 0)
    with pytest.raises(RuntimeError, match='strength is not finite'):
        c.call('mpt_mesh_set_displacement_params', good, float('nan'), 0.5)
    with pytest.raises(ValueError, match='finite'):
        pool.set_displacement(good, 1.0, float('inf'))
    late = _add(pool, 'tetrahedron', 1, None)
    obj, obj_late = pool.add_object(good, EYE), pool.add_object(late, EYE)
    with pytest.raises(RuntimeError, match='already has an object'):
        call(late)
    with pytest.raises(ValueError, match='already has an object'):
        pool.add_displacement(late, 0)
    pool.compose()
    _differ(pool.subdivided_to_numpy(obj), _expected('octahedron', 1, disp), 'after the refusals')
    _differ(pool.subdivided_to_numpy(obj_late), sr.fixture_subdivided('tetrahedron', 1), 'the mesh that was refused')
    assert _stats(pool) == (3, 1, 1, _nverts('octahedron', 1)) and pool.nfaces == 32 + 16


# ---------------------------------------------------------------- 9: lifecycle
def test_clear_and_mesh_add_while_displaced_copies_exist(fresh):
    pool = _start()
    _load_images()
    rig = _rig('cylinder', 2)
    pose = _pose(8)
    dc, di = (0, dr.NORMAL, dr.B, 0.3, 0.5), (1, dr.VECTOR, dr.R, 0.2, 0.4)
    mc, mi = _add(pool, 'cylinder', 2, dc, rig), _add(pool, 'icosahedron', 1, di)
    oc, oi = pool.add_object(mc, _world(1)), pool.add_object(mi, _world(2))
    _set_pose(pool, oc, pose)
    pool.compose()
    want_c, want_i = _expected('cylinder', 2, dc, rig, pose), _expected('icosahedron', 1, di)
    _differ(pool.subdivided_to_numpy(oc), want_c, 'cylinder')
    _differ(pool.subdivided_to_numpy(oi), want_i, 'icosahedron')
    # a mesh joins the pool where the copies lay (its topology and its corner table behind the others' in the arena)
    dg = (1, dr.NORMAL, dr.MEAN, -0.25, 0.5)
    mg = _add(pool, 'grid', 3, dg)
    with pytest.raises(RuntimeError, match='no subdivided copy yet'):
        pool.subdivided_to_numpy(oc)
    og = pool.add_object(mg, _world(3))
    pool.compose()
    assert _stats(pool) == (3, 3, 3, _nverts('cylinder', 2) + _nverts('icosahedron', 1) + 1681)
    _differ(pool.subdivided_to_numpy(oc), want_c, 'cylinder after a mesh was added')
    _differ(pool.subdivided_to_numpy(oi), want_i, 'icosahedron after a mesh was added')
    _differ(pool.subdivided_to_numpy(og), _expected('grid', 3, dg), 'the new grid')
    # clear_objects: the copies go, the meshes keep their levels and displacements
    pool.clear_objects()
    assert _stats(pool)[:2] == (3, 0)
    oi, oi2 = pool.add_object(mi, _world(4)), pool.add_object(mi, _world(5))
    pool.compose()
    assert _stats(pool) == (3, 1, 1, _nverts('icosahedron', 1)) and pool.nfaces == 160
    _differ(pool.subdivided_to_numpy(oi2), want_i, 'icosahedron after clear_objects')
    pool.set_displacement(mi, 0.5)
    pool.compose()
    _differ(pool.subdivided_to_numpy(oi), _expected('icosahedron', 1, (1, dr.VECTOR, dr.R, 0.5, 0.4)), 'icosahedron after set_displacement')
    # clear_meshes: everything goes; a new mesh starts from nothing
    pool.clear_meshes()
    assert _stats(pool)[:2] == (0, 0)
    with pytest.raises(ValueError, match='has no displacement'):
        pool.set_displacement(0, 1.0)
    df = (0, dr.NORMAL, dr.R, 0.6, 0.5)
    obj = pool.add_object(_add(pool, 'fan7', 2, df), EYE)
    plain = pool.add_object(_add(pool, 'fan7', 2, None), EYE)
    pool.compose()
    _differ(pool.subdivided_to_numpy(obj), _expected('fan7', 2, df), 'fan7 after clear_meshes')
    _differ(pool.subdivided_to_numpy(plain), sr.fixture_subdivided('fan7', 2), 'fan7 without a displacement after clear_meshes')
    assert pool.nfaces == 2 * 14 * 16 and _stats(pool) == (1, 1, 1, _nverts('fan7', 2))


# ---------------------------------------------------------------- 10: the worker facade
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
        ns.add_mesh = lambda: worker.ModelPool().add_mesh(*deform_ref.split(sr.fixture('grid')))
        ns.add_object = lambda mesh: worker.ModelPool().add_object(mesh, _world(1))
        ns.fetch = lambda obj: worker.ModelPool().subdivided_to_numpy(obj)
        ns.stats = lambda: worker.ModelPool().displace_stats().displaced_verts
        return ns
    w = OnDemandProxy(lambda: DaemonModule(module))
    w.init()
    w.load_images(images=list(IMAGES))
    mesh = w.add_mesh()
    w.set_mesh_subdivision(mesh=mesh, levels=2)
    w.set_mesh_displacement(mesh=mesh, image=1, strength=0.3, mode='vector')
    obj = w.add_object(mesh)
    assert seen and seen[0] != threading.get_ident()
    w.compose_model()
    assert w.stats() == _nverts('grid', 2)
    _differ(w.fetch(obj), _expected('grid', 2, (1, dr.VECTOR, dr.MEAN, 0.3, 0.5)), 'through the worker')
    w.set_mesh_displacement_params(mesh, -0.2)
    w.compose_model()
    _differ(w.fetch(obj), _expected('grid', 2, (1, dr.VECTOR, dr.MEAN, -0.2, 0.5)), 'through the worker, after the strength changed')
    w.set_mesh_displacement_params(mesh=mesh, strength=0.1, midlevel=0.25)
    w.compose_model()
    _differ(w.fetch(obj), _expected('grid', 2, (1, dr.VECTOR, dr.MEAN, 0.1, 0.25)), 'through the worker, after the midlevel changed')
    w.synchronize()

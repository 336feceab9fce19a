'''
CPU tests of the device composition (ModelPool.load_meshes): the layout and launch plan as a pure function,
the new entry points' refusals without a context, the Python layer's argument checks (which raise before any device call), and the
fixture's own precondition.
'''

import ctypes as C
import os

import numpy as np
import pytest

import compose_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'reference_compose.npz')


def plan(faces, dirty=None):
    from ptina_amd import _lib
    return _lib.compose_plan(faces, dirty)


def test_plan_offsets_and_full_launch():
    first, runs = plan([1, 21, 22, 85, 0, 21, 86, 85, 300])
    assert first.tolist() == [0, 1, 22, 44, 129, 129, 150, 236, 321, 621]
    assert runs == [(0, (621 * 3 + 255) // 256)]                     # all dirty: every workgroup of the output, one run
    first, runs = plan([])
    assert first.tolist() == [0] and runs == []
    first, runs = plan([0, 0])
    assert first.tolist() == [0, 0, 0] and runs == []


def test_plan_none_one_and_all_dirty():
    faces = [100, 200, 300, 400]                                     # vertices [0,300) [300,900) [900,1800) [1800,3000)
    assert plan(faces, [0, 0, 0, 0])[1] == []
    assert plan(faces, [0, 1, 0, 0])[1] == [(1, 3)]                  # workgroups 1..3 hold vertices 256..1023
    assert plan(faces, [1, 0, 0, 0])[1] == [(0, 2)]
    assert plan(faces, [0, 0, 0, 1])[1] == [(7, 5)]                  # 1800 // 256 = 7 .. 2999 // 256 = 11
    assert plan(faces, [1, 0, 0, 1])[1] == [(0, 2), (7, 5)]
    assert plan(faces, [1, 1, 1, 1])[1] == plan(faces)[1] == [(0, 12)]
    assert plan(faces, [1, 1, 0, 1])[1] == [(0, 4), (7, 5)]          # runs that share workgroup 1 are one run
    assert plan([256, 256, 256], [1, 0, 1])[1] == [(0, 3), (6, 3)]
    assert plan([256, 256, 256], [1, 1, 0])[1] == [(0, 6)]           # runs that touch are one run


def test_plan_workgroup_boundaries():
    '''256 faces are 768 vertices, exactly three workgroups: the object ends on a boundary; one more face reaches into the fourth.
    After 85 faces (255 vertices) a one-face object holds vertices 255..257: the last lane of workgroup 0 and two of workgroup 1'''
    assert plan([256, 5], [1, 0])[1] == [(0, 3)]
    assert plan([257, 5], [1, 0])[1] == [(0, 4)]
    assert plan([256, 5], [0, 1])[1] == [(3, 1)]
    assert plan([85, 1, 500], [0, 1, 0])[1] == [(0, 2)]
    assert plan([85, 1, 500], [1, 0, 0])[1] == [(0, 1)]
    assert plan([86, 1, 500], [0, 1, 0])[1] == [(1, 1)]              # vertices 258..260


def test_plan_empty_objects_launch_nothing():
    first, runs = plan([10, 0, 10], [0, 1, 0])
    assert first.tolist() == [0, 10, 10, 20] and runs == []
    assert plan([0, 300, 0], [1, 0, 1])[1] == []
    assert plan([0, 300, 0], [1, 1, 1])[1] == [(0, 4)]


def test_plan_refusals_and_capacity():
    from ptina_amd import _lib
    lib = _lib.load_library()
    with pytest.raises(ValueError):
        plan([3, -1])
    with pytest.raises(ValueError):
        plan([2 ** 30, 2 ** 30])                                     # 3 x total beyond 31 bits
    with pytest.raises(ValueError):
        plan([1, 2], [1])
    assert lib.mpt_compose_plan(None, None, 1, None, None, None, 0) == -1
    assert lib.mpt_compose_plan(None, None, -1, None, None, None, 0) == -1
    assert lib.mpt_compose_plan(None, None, 0, None, None, None, 0) == 0
    # cap = 0 counts the runs; a smaller cap writes the first ones only
    f = np.array([256, 256, 256, 256, 256], np.int32)
    d = np.array([1, 0, 1, 0, 1], np.int32)
    assert lib.mpt_compose_plan(_lib.iptr(f), _lib.iptr(d), 5, None, None, None, 0) == 3
    begin, count = np.full(2, -7, np.int64), np.full(2, -7, np.int64)
    p64 = C.POINTER(C.c_int64)
    assert lib.mpt_compose_plan(_lib.iptr(f), _lib.iptr(d), 5, None, begin.ctypes.data_as(p64), count.ctypes.data_as(p64), 1) == 3
    assert begin.tolist() == [0, -7] and count.tolist() == [3, -7]


def test_new_symbols_exist_and_refuse_a_null_context():
    from ptina_amd import _lib
    lib = _lib.load_library()
    w = (C.c_double * 16)(*np.eye(4).ravel())
    v = np.zeros((3, 8), np.float32)
    out = C.c_int(0)
    info = _lib.ComposeInfo()
    ms = C.c_double(0)
    calls = [('mpt_mesh_add', (_lib.fptr(v), 1, C.byref(out))), ('mpt_object_add', (0, w, -1, C.byref(out))),
             ('mpt_object_set_world', (0, w)), ('mpt_object_set_material', (0, 0)), ('mpt_scene_clear', (1,)), ('mpt_compose', ()),
             ('mpt_compose_stats', (C.byref(info),)), ('mpt_get_model', (None, None, 0, C.byref(out))),
             ('mpt_compose_kernel_time', (C.byref(ms), C.byref(out)))]
    for name, args in calls:
        assert getattr(lib, name)(None, *args) != 0, name
        assert b'null' in lib.mpt_last_error(), name
    assert C.sizeof(_lib.ComposeInfo) == 64


def pool(size=2 ** 21):
    from ptina_amd.model import ModelPool
    m = ModelPool.__new__(ModelPool)
    ModelPool.__init__(m, size)
    return m


def test_python_argument_checks_raise_before_any_device_call(monkeypatch):
    from ptina_amd import model

    def no_device():
        raise AssertionError('a device call was made')
    monkeypatch.setattr(model, 'ctx', no_device)
    m = pool(size=100)
    p, n, t = np.zeros((4, 3, 3)), np.ones((4, 3, 3)), np.zeros((4, 3, 2))
    for bad in ((p[:, :2], n, t), (p, n[:3], t), (p, n, np.zeros((4, 3, 3))), (np.zeros(5), n, None), (np.float32(1.0), n, None)):
        with pytest.raises(ValueError, match='must be'):
            m.add_mesh(*bad)
    with pytest.raises(ValueError, match='too many faces'):
        m.add_mesh(np.zeros((100, 3, 3)), np.zeros((100, 3, 3)))
    with pytest.raises(ValueError, match='unknown mesh'):
        m.add_object(0, np.eye(4))
    m._mesh_faces = [60, 40]                                         # two meshes, as if added
    with pytest.raises(ValueError, match='unknown mesh'):
        m.add_object(2, np.eye(4))
    with pytest.raises(ValueError, match='unknown mesh'):
        m.add_object(-1, np.eye(4))
    with pytest.raises(ValueError, match='4x4'):
        m.add_object(0, np.eye(3))
    w = np.eye(4)
    w[1, 2] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        m.add_object(0, w)
    m._obj_mesh = [0]                                                # one object of 60 faces, as if added
    with pytest.raises(ValueError, match='too many faces'):
        m.add_object(0, np.eye(4))                                   # 120 faces
    with pytest.raises(ValueError, match='too many faces'):
        m.add_object(1, np.eye(4))                                   # 100 faces: 99 is the most a pool of 100 takes (model.py:84: n < size)
    for obj in (1, -1):
        with pytest.raises(ValueError, match='unknown object'):
            m.set_world(obj, np.eye(4))
        with pytest.raises(ValueError, match='unknown object'):
            m.set_material(obj, 0)
    with pytest.raises(ValueError, match='not finite'):
        m.set_world(0, w)
    with pytest.raises(ValueError, match='4x4'):
        m.set_world(0, np.zeros(16))
    with pytest.raises(ValueError, match='no primitives'):
        m.load_meshes([])


def test_worker_names_the_composition_entries():
    from ptina_amd import worker
    import inspect
    assert list(inspect.signature(worker.load_meshes).parameters) == ['primitives']
    assert list(inspect.signature(worker.set_object_world).parameters) == ['obj', 'world']
    assert callable(worker.compose_model)
    import importlib
    assert importlib.import_module('ptina.worker') is worker


def test_fixture_precondition_holds():
    '''every position and normal component of the reference's output lies more than MARGIN a-priori error bounds of an f64
    evaluation away from an f32 rounding boundary, so its f32 bits do not depend on the order of the evaluation'''
    g = np.load(GOLD)
    prims = compose_ref.fixture_primitives(g)
    assert [np.asarray(p[0]).shape[0] for p in prims] == [1, 21, 22, 85, 0, 21, 86, 85, 300]
    assert prims[1][0] is prims[5][0] and prims[3][0] is prims[7][0]              # two pairs share a mesh
    assert all(p[0].dtype == np.float32 for p in prims) and g['obj_world'].dtype == np.float64
    assert g['obj_world'][3][3].tolist() == [0, 0, 0, 2] and g['obj_world'][6][3].tolist() == [0.01, -0.02, 0.03, 1]
    assert g['obj_mtl_none'].sum() == 2
    worst, closest, count = compose_ref.margin(prims, g['out_verts'])
    print('fixture: %d values, the closest %.3g error bounds (%.3g f32 ulp) from a boundary' % (count, worst, closest))
    assert count == 11178 and worst > compose_ref.MARGIN
    assert np.isfinite(g['out_verts']).all()


def test_sequential_f64_evaluation_gives_the_reference_bits():
    '''the kernel's order of operations (csrc/compose.hip), restated in numpy: 0 differing f32 bits on the fixture; and the
    package's own compose_multiple_meshes agrees with the reference's output'''
    from ptina_amd.multimesh import compose_multiple_meshes
    g = np.load(GOLD)
    prims = compose_ref.fixture_primitives(g)
    rows = []
    for p, n, t, w, m in prims:
        p, n, t = (a.astype(np.float64).reshape(-1, a.shape[-1]) for a in (p, n, t))
        ph = [((p[:, 0] * w[j, 0] + p[:, 1] * w[j, 1]) + p[:, 2] * w[j, 2]) + w[j, 3] for j in range(4)]
        nh = [(n[:, 0] * w[j, 0] + n[:, 1] * w[j, 1]) + n[:, 2] * w[j, 2] for j in range(3)]
        ln = np.sqrt((nh[0] * nh[0] + nh[1] * nh[1]) + nh[2] * nh[2])
        rows.append(np.stack([ph[0] / ph[3], ph[1] / ph[3], ph[2] / ph[3], nh[0] / ln, nh[1] / ln, nh[2] / ln, t[:, 0], t[:, 1]], axis=1))
    got = np.concatenate(rows).astype(np.float32)
    want = g['out_verts'].astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    v, m = compose_multiple_meshes(prims)
    assert np.array_equal(v.astype(np.float32).view(np.uint32), want.view(np.uint32)) and np.array_equal(m, g['out_mtlids'])

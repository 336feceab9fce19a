'''
Every tree builder, held to tests/tree_checks.py (-m gpu): the reference LBVH (lbvh_build.hip), the SAH re-partition on
the host and on the device (sah_build.hip: the finish kernel up to 1024 triangles, binned levels above) and the 4-wide
collapse on the host and on the device (wide_build.hip) are built, downloaded and checked against the model's vertices:
child boxes exact and enclosing (E1-E4), 8-bit boxes rounded outwards and no looser than 1.26 steps (Q1-Q6), the LBVH
arrays (L1-L5), and the options the LDS kernel sizes its stack by (S1) recomputed from the records.  No case renders.

The binary `fnode` records (what the production build's preview, brute-force and Metropolis kernels and wide = 0 /
lds_wide = 0 walk), whose inner boxes the collapse drops, are not checked here: they are downloaded through
BVHTree().records() and held word for word by tests/record_checks.py in tests/test_records_gpu.py, with `snode` and the
triangle records.  Their walks are held to an exhaustive search, pixel for pixel, over the host's and the device's SAH pass:
tests/test_visibility_gpu.py (preview, brute, Metropolis door, kernels 0 and 1).
'''

import numpy as np
import pytest

import tree_checks as tc
from ptina_amd import scenes

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 4, 5, 7, 33, 64, 65, 300, 512, 513, 1023, 1024, 1025, 1100, 2049, 5000, 20000]
# (tree, sah_build, wide_build): tree 1 = SAH, 0 = the LBVH itself; sah_build 1 = device, 0 = host; wide_build 1 = device, 0 = host
BUILDERS = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, None, 1), (0, None, 0)]


def _positions(v):
    v = np.asarray(v, np.float32)
    return np.ascontiguousarray(v.reshape(-1, 3, 8)[:, :, :3])


def _wide_records(c):
    import ctypes as C
    from ptina_amd import _lib
    nw = C.c_int(0)
    c.call('mpt_get_wide', None, None, 0, C.byref(nw))
    assert nw.value > 0, 'the 4-wide collapse was not built'
    w = np.zeros((nw.value, 8, 4), np.float32)
    q = np.zeros((nw.value, 4, 4), np.float32)
    c.call('mpt_get_wide', _lib.fptr(w), _lib.fptr(q), nw.value, C.byref(nw))
    return w.view(np.uint32), q.view(np.uint32)


def _note_margins(what, t):
    '''the tightest Q4 margin and the loosest Q5 distance of the case, in steps: printed for profiles/r11_tree_margins.json
    (a record, not a bound)'''
    m = tc.q_margins(t)
    print(f'{what}: {t.nw} wide nodes, Q4 min margin {m["q4_min_steps"]}, Q5 max distance {m["q5_max_steps"]} steps')


def _load(v, m, n):
    from ptina_amd.things import init_things, ModelPool
    from ptina_amd.common import ctx
    init_things()
    ModelPool().load(v, m)
    return ctx()


def _build_and_check(c, pos, n, what, tree=None, sah=None, wide=None):
    '''build with the given options (None: the default), download, check everything; -> (wnode, qnode) bytes'''
    from ptina_amd.things import BVHTree
    for key, value in (('tree', tree), ('sah_build', sah), ('wide_build', wide)):
        if value is not None:
            c.set_option(key, value)
    BVHTree().build()
    if sah == 1 or (sah is None and tree != 0):
        assert c.get_option('sah_fallback') == 0, f'{what}: the device SAH pass fell back to the host pass'
    lb = BVHTree().to_numpy()
    w, q = _wide_records(c)
    try:
        tc.check_lbvh(pos, lb, n)
        t = tc.check_all(pos, lb['leaf'], w, q, n)
    except AssertionError as e:
        raise AssertionError(f'{what}: {e}') from None
    assert c.get_option('wide_nodes') == t.nw
    depth, stack, need = c.get_option('wide_depth'), c.get_option('wide_stack'), tc.stack_need(t.ids, n)
    assert depth == tc.levels(t.ids, n), f'{what}: wide_depth {depth}, the records have {tc.levels(t.ids, n)} levels'
    assert need <= stack <= 3 * depth + 2, f'{what}: wide_stack {stack}, a traversal can ask for {need}, the bound is {3 * depth + 2}'
    if c.get_option('wide_build') == 0:
        assert stack == need, f'{what}: the host collapse reports wide_stack {stack}, the records need {need}'
    _note_margins(what, t)
    return w, q


def _random_model(n):
    v, m, _, _ = scenes.scene_random_tris(n, seed=n, edge=0.05)
    if n >= 9:
        v[3 * 7:3 * 9] = v[3 * 5:3 * 7]            # exact duplicates -> equal boxes, equal centres, equal Morton codes
    elif n >= 7:
        v[3 * 6:3 * 7] = v[3 * 5:3 * 6]            # (seven triangles have no 7 and 8: the last one doubles its neighbour)
    return v, m


@pytest.mark.parametrize('n', SIZES)
def test_every_builder_at_every_size(fresh, n):
    '''n <= 1024: the device SAH pass is the finish kernel alone; above: binned levels first.  2 to 5 triangles give nodes
    with unused slots.  Every combination of SAH pass (device / host / none: the LBVH itself) and collapse (device / host)'''
    v, m = _random_model(n)
    c = _load(v, m, n)
    pos = _positions(v)
    for tree, sah, wide in BUILDERS:
        _build_and_check(c, pos, n, f'n {n} tree {tree} sah_build {sah} wide_build {wide}', tree, sah, wide)


def test_the_default_builders_at_the_size_of_config_4(fresh):
    n = 99382
    v, m = _random_model(n)
    c = _load(v, m, n)
    _build_and_check(c, _positions(v), n, f'n {n} defaults')


@pytest.mark.parametrize('name,kw', [('s34', {}), ('s978', {}), ('c4', {'n_side': 24}), ('c5', {'n': 60000})])
def test_the_projects_own_scenes(fresh, name, kw):
    v, m, _, _ = scenes.get_scene(name, **kw)
    n = m.shape[0]
    c = _load(v, m, n)
    _build_and_check(c, _positions(v), n, f'{name} {kw} defaults')


@pytest.mark.parametrize('kind', ['identical', 'on_a_line', 'huge', 'two_clusters'])
def test_degenerate_models(fresh, kind):
    '''the models of test_device_sah_pass_on_degenerate_models (no split can be chosen by cost), device SAH pass asked for.
    Every property applies to every kind: with coordinates around 1e18 the boxes' extents (1e17) and the steps (1e15) are
    finite f32 values, and the ulp terms of Q3 / Q4 carry the magnitude'''
    n = 3000
    v, m, _, _ = scenes.scene_random_tris(n, seed=7, edge=0.05)
    v = v.reshape(n, 3, 8).copy()
    if kind == 'identical':
        v[:] = v[0]
    elif kind == 'on_a_line':
        v[:, :, 1:3] = v[0, :, 1:3]
        v[:, :, 0] = v[0, :, 0] + np.arange(n, dtype=np.float32)[:, None] * 1e-3
    elif kind == 'huge':
        v[:, :, :3] *= np.float32(1e18)
    else:
        v[:] = v[0]
        v[n // 3:, :, :3] += np.float32(5.0)
    v = v.reshape(n * 3, 8)
    c = _load(v, m, n)
    pos = _positions(v)
    for wide in (1, 0):
        _build_and_check(c, pos, n, f'{kind} sah_build 1 wide_build {wide}', 1, 1, wide)


def _moved():
    v, m, _, _ = scenes.scene_s978()
    v = np.array(v, np.float32, copy=True)
    v[:, 0:3] += np.array([300.0, -200.0, 500.0], np.float32)
    return v, m


def _scaled(f):
    v, m, _, _ = scenes.scene_s978()
    v = np.array(v, np.float32, copy=True)
    v[:, 0:3] *= np.float32(f)
    return v, m


def _flat():
    '''200 triangles in the plane y = 1: every node is flat along y and takes the e == 0 branch of Q3'''
    v, m, _, _ = scenes.scene_random_tris(200, seed=200, edge=0.05)
    v = np.array(v, np.float32, copy=True)
    v[:, 1] = np.float32(1.0)
    return v, m


MODELS = {'moved': _moved, 'times_0.002': lambda: _scaled(0.002), 'times_50': lambda: _scaled(50.0), 'flat': _flat}


@pytest.mark.parametrize('name', list(MODELS))
def test_far_from_the_origin_and_other_scales(fresh, name):
    '''s978 moved by (300, -200, 500) as in test_quantised_boxes_far_from_the_origin (the quantised planes' f32 sums round
    at the size of the coordinates, not of the boxes), s978 at 0.002 and 50 times its size, and a flat model.  Default
    options, and the host collapse too.  The flat and the moved model are built twice: the same verdict, the same bytes'''
    v, m = MODELS[name]()
    n = m.shape[0]
    c = _load(v, m, n)
    pos = _positions(v)
    first = _build_and_check(c, pos, n, f'{name} defaults')
    if name == 'flat':
        t = tc.Tree(pos, np.arange(n), first[0], first[1], n)
        assert np.all(t.node_hi[:, 1] == t.origin[:, 1]), 'every node is flat along y'
    if name in ('flat', 'moved'):
        again = _build_and_check(c, pos, n, f'{name} defaults, built again')
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    host = _build_and_check(c, pos, n, f'{name} wide_build 0', wide=0)
    assert np.array_equal(first[0], host[0]) and np.array_equal(first[1], host[1])

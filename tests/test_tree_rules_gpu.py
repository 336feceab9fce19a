'''
The device passes of the tree build against the host passes, byte for byte (-m gpu): what mpt_get_tree, mpt_get_records and
mpt_get_wide read back after a device build equals what the stand-alone host program tools/tree_rules_check.cpp
(tests/tree_rules_tool.py: tree_host.h on tree_rules.h, compiled by the host compiler) writes for the same positions.

Two builders: the device LBVH and collapse around the host SAH pass (sah_build = 0), and around the device SAH pass
(sah_build = 1) up to 1024 triangles, where its finish kernel is the host pass node for node.  The shapes are the smallest at which
a shared rule can still go wrong: no internal node, fewer than four children, the empty slot, equal Morton codes, boxes without
extent, and the first size above one finish task.
'''

import ctypes as C

import numpy as np
import pytest

from tree_rules_tool import F, U, compile_tool, run_tool, coincident, flat
from test_tree_invariants_gpu import _positions, _random_model

pytestmark = pytest.mark.gpu

MODELS = {f'n{n}': (lambda n=n: _positions(_random_model(n)[0])) for n in (1, 2, 3, 4, 5, 33, 1024, 1025)}
MODELS.update(coincident8=lambda: coincident(8), flat64=lambda: flat(64))
CASES = [(name, sah) for name in MODELS for sah in (0, 1) if not (name == 'n1025' and sah == 1)]


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    return compile_tool(tmp_path_factory.mktemp('tree_rules'))


def _vertices(pos):
    '''[3n][8] vertices (pos3 nrm3 uv2) and [n] material ids around the positions'''
    n = pos.shape[0]
    v = np.zeros((n, 3, 8), F)
    v[:, :, 0:3] = pos
    v[:, :, 5] = F(1.0)
    return v.reshape(3 * n, 8), np.zeros(n, np.int32)


def _wide(c):
    from ptina_amd import _lib
    nw = C.c_int(0)
    c.call('mpt_get_wide', None, None, 0, C.byref(nw))
    w, q = np.zeros((nw.value, 8, 4), F), np.zeros((nw.value, 4, 4), F)
    if nw.value:
        c.call('mpt_get_wide', _lib.fptr(w), _lib.fptr(q), nw.value, C.byref(nw))
    return w.view(U), q.view(U)


def _words(a):
    return np.ascontiguousarray(a).view(U)


@pytest.mark.parametrize('name,sah', CASES)
def test_device_passes_leave_the_host_programs_bytes(fresh, tool, tmp_path, name, sah):
    from ptina_amd.things import init_things, ModelPool, BVHTree
    from ptina_amd.common import ctx
    pos = MODELS[name]()
    n = pos.shape[0]
    init_things()
    c = ctx()
    ModelPool().load(*_vertices(pos))
    for key, value in (('gpu_build', 1), ('tree', 1), ('sah_build', sah), ('wide_build', 1)):
        c.set_option(key, value)
    BVHTree().build()
    assert c.get_option('sah_fallback') == 0, 'the device SAH pass fell back to the host pass'
    want = run_tool(tool, tmp_path, pos, tree=1, sah_exact_max=c.get_option('sah_exact_max'))

    got = dict(BVHTree().to_numpy())
    got.update(BVHTree().records())
    got['wnode'], got['qnode'] = _wide(c)
    for a in (got, want):
        a['fnode'] = np.array(a['fnode'], copy=True)
        a['fnode'][:, 3, 2:4] = 0                            # (the two unspecified words of the id row)
    for key in ('child', 'leaf', 'mc', 'bmin', 'bmax', 'snode', 'fnode', 'wnode', 'qnode'):
        assert got[key].shape == want[key].shape, f'{name} sah_build {sah}: {key} has shape {got[key].shape}, the host program gives {want[key].shape}'
        bad = np.argwhere(_words(got[key]) != _words(want[key]))
        assert bad.shape[0] == 0, (f'{name} sah_build {sah}: {key} differs in {bad.shape[0]} words; first at {bad[0].tolist()}: '
                                   f'0x{int(_words(got[key])[tuple(bad[0])]):08x} != 0x{int(_words(want[key])[tuple(bad[0])]):08x}')
    assert int(got['depth']) == want['depth'] == c.get_option('tree_depth')
    assert c.get_option('fast_depth') == want['fast_depth']
    assert (c.get_option('wide_nodes'), c.get_option('wide_depth'), c.get_option('wide_stack')) == (want['nw'], want['wide_depth'], want['wide_stack'])

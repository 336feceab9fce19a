'''
The host passes of the tree build without a GPU: ptina_amd/csrc/tree_host.h on the rules of tree_rules.h, compiled into the
stand-alone program tools/tree_rules_check.cpp (tests/tree_rules_tool.py).  Their bytes are held to tests/golden/refit_records.npz
-- what the default builders (device LBVH, host SAH pass, device collapse) left on an MI355X -- and their trees to the numpy
checkers of tests/tree_checks.py, which restate nothing of the headers.
'''

import os

import numpy as np
import pytest

import tree_checks as tc
from tree_rules_tool import F, ROOT, compile_tool, run_tool, coincident, flat

RECORDED = ('child', 'leaf', 'bmin', 'bmax', 'mc', 'wnode', 'qnode')


@pytest.fixture(scope='module')
def tool(tmp_path_factory):
    return compile_tool(tmp_path_factory.mktemp('tree_rules'))


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'refit_records.npz'))


def _check(pos, got):
    '''the LBVH and the wide tree of `got` against the positions: every property of tests/tree_checks.py, and the two figures the
    program derives from the id rows'''
    n = len(pos)
    tc.check_lbvh(pos, got, n)
    t = tc.check_all(pos, got['leaf'], got['wnode'], got['qnode'], n)
    assert t.nw == got['nw']
    assert tc.levels(t.ids, n) == got['wide_depth']
    assert tc.stack_need(t.ids, n) == got['wide_stack']
    return t


@pytest.mark.parametrize('n', [5, 33, 300, 1025])
def test_the_host_passes_give_the_recorded_bytes(tool, golden, tmp_path, n):
    assert n in golden['sizes']
    pos = golden[f'pos_{n}']
    got = run_tool(tool, tmp_path, pos)
    for name in RECORDED:
        want = golden[f'{name}_{n}']
        assert got[name].shape == want.shape and got[name].dtype == want.dtype, f'n {n}: {name} is {got[name].shape} {got[name].dtype}'
        bad = np.argwhere(got[name].view(np.uint32) != want.view(np.uint32))
        assert bad.shape[0] == 0, f'n {n}: {name} differs from the recorded bytes in {bad.shape[0]} words, first at {bad[0].tolist()}'
    assert got['depth'] == int(golden[f'depth_{n}'])
    _check(pos, got)


@pytest.mark.parametrize('n', [1, 2])
def test_one_and_two_triangles(tool, golden, tmp_path, n):
    pos = golden['pos_5'][:n]
    got = run_tool(tool, tmp_path, pos)
    assert got['nw'] == n - 1 and got['fnode'].shape == (n - 1, 4, 4) and got['snode'].shape == (n - 1, 2, 4)
    assert sorted(got['leaf'].tolist()) == list(range(n))
    if n == 1:
        assert got['depth'] == 0 and got['wide_depth'] == 0 and got['wide_stack'] == 0
    else:
        assert got['depth'] == 1 and got['fast_depth'] == 1 and got['child'].tolist() == [[0, 1]]
        t = _check(pos, got)
        assert t.ids[0].tolist() == [~0, ~1, ~2, ~2]         # two leaves, two empty slots naming leaf n


@pytest.mark.parametrize('tree', [1, 0])
def test_eight_coincident_triangles(tool, tmp_path, tree):
    '''all Morton codes equal: the face index in the low word of the key is what keeps the hierarchy a tree'''
    pos = coincident(8)
    got = run_tool(tool, tmp_path, pos, tree=tree)
    assert (got['mc'] == got['mc'][0]).all() and got['leaf'].tolist() == list(range(8))
    _check(pos, got)
    assert (got['bmin'] == pos[0].min(axis=0)).all() and (got['bmax'] == pos[0].max(axis=0)).all()


def test_flat_triangles_take_the_positive_step_branch(tool, tmp_path):
    pos = flat(64)
    got = run_tool(tool, tmp_path, pos)
    t = _check(pos, got)
    assert (t.node_lo[:, 2] == t.node_hi[:, 2]).all()        # no node has an extent along z ...
    assert (t.scale[:, 2] == np.maximum(np.abs(t.origin[:, 2]) * F(1e-6), F(1e-30))).all() and (t.scale > 0).all()   # ... yet a step
    assert (t.node_lo[:, 0] == t.node_hi[:, 0]).any()        # and some have none along x either

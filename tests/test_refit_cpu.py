'''
tests/refit_ref.py -- the numpy statement of what BVHTree().refit() must write -- held to this project's own builders and to
the independent checker, without a GPU.  The fixture tests/golden/refit_records.npz was recorded from the build on the GPU
(tests/golden/make_refit_golden.py).

  * a refit to the SAME vertices gives the build's wnode, qnode, bmin and bmax back byte for byte: the restatement is the
    builders' arithmetic (the boxes' unions and tree_rules.h's quantisation, f32 operation for operation);
  * a refit to MOVED vertices -- the two start kinds of tests/test_refit_gpu.py, jitter and shuffle -- passes every property of
    tests/tree_checks.py against the moved vertices;
  * the checker sees a refit that is wrong: one box value or one quantised byte altered, and it names E1 / E2 / Q4;
  * the pure pieces of mpt_refit_tree, through the C ABI: the permission rule's verdicts and words, and the growth figure.
'''

import os

import numpy as np
import pytest

import refit_ref
import tree_checks as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (5, 33, 300, 1025)
F = np.float32


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'refit_records.npz'))


def _case(g, n):
    tree = {k: g[f'{k}_{n}'] for k in ('child', 'leaf', 'bmin', 'bmax', 'mc')}
    tree['depth'] = int(g[f'depth_{n}'])
    return g[f'pos_{n}'], tree, g[f'wnode_{n}'], g[f'qnode_{n}']


def jitter(pos, seed):
    '''every triangle translated by up to one edge length (its own longest edge), seeded'''
    pos = np.asarray(pos, F).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    edge = np.linalg.norm(pos - np.roll(pos, 1, axis=1), axis=2).max(axis=1)
    step = (rng.uniform(-1, 1, (pos.shape[0], 3)) / np.sqrt(3.0) * edge[:, None]).astype(F)
    return (pos + step[:, None, :]).astype(F)


def shuffled(pos, seed):
    '''face f placed where face perm[f] is'''
    pos = np.asarray(pos, F).reshape(-1, 3, 3)
    return np.ascontiguousarray(pos[np.random.default_rng(seed).permutation(pos.shape[0])])


@pytest.mark.parametrize('n', SIZES)
def test_same_vertices_give_the_builds_bytes(gold, n):
    pos, tree, w, q = _case(gold, n)
    bmin, bmax, w2, q2 = refit_ref.refit_ref(tree['child'], tree['leaf'], w, q, n, pos)
    assert np.array_equal(bmin.view(np.uint32), tree['bmin'].view(np.uint32))
    assert np.array_equal(bmax.view(np.uint32), tree['bmax'].view(np.uint32))
    assert np.array_equal(w2, w), f'{int((w2 != w).sum())} words of wnode differ'
    assert np.array_equal(q2, q), f'{int((q2 != q).sum())} words of qnode differ'


@pytest.mark.parametrize('kind', ['jitter', 'shuffled'])
@pytest.mark.parametrize('n', SIZES)
def test_moved_vertices_pass_the_checker(gold, n, kind):
    pos, tree, w, q = _case(gold, n)
    moved = jitter(pos, n) if kind == 'jitter' else shuffled(pos, n)
    assert not np.array_equal(moved, pos)
    bmin, bmax, w2, q2 = refit_ref.refit_ref(tree['child'], tree['leaf'], w, q, n, moved)
    t = tc.check_all(moved, tree['leaf'], w2, q2, n)
    assert np.array_equal(t.ids, tc.Tree(pos, tree['leaf'], w, q, n).ids), 'a refit keeps every id'
    tc.check_lbvh(moved, dict(tree, bmin=bmin, bmax=bmax), n)
    # ... and the build's own boxes do not enclose the moved model: the checker is looking at the positions
    assert tc.failing(moved, tree['leaf'], w, q, n)


def test_the_checker_names_a_wrong_refit(gold):
    n = 300
    pos, tree, w, q = _case(gold, n)
    moved = jitter(pos, 1)
    _, _, w2, q2 = refit_ref.refit_ref(tree['child'], tree['leaf'], w, q, n, moved)
    t = tc.Tree(moved, tree['leaf'], w2, q2, n)
    assert tc.failing(moved, tree['leaf'], w2, q2, n) == []
    node, slot = np.argwhere(t.leafc)[0]
    bad = w2.copy()
    bad[node, 0, slot] = np.nextafter(bad[node, 0, slot:slot + 1].view(F), F(np.inf)).view(np.uint32)[0]     # lo.x of a leaf child, one ulp up
    assert 'E1' in tc.failing(moved, tree['leaf'], bad, q2, n)
    node, slot = np.argwhere(t.inner)[0]
    bad = w2.copy()
    bad[node, 1, slot] = np.nextafter(bad[node, 1, slot:slot + 1].view(F), F(-np.inf)).view(np.uint32)[0]    # hi.x of an internal child, one ulp down
    assert 'E2' in tc.failing(moved, tree['leaf'], bad, q2, n)
    # a low byte that is not clamped, raised by two steps: the plane is inside the child
    at = np.argwhere(t.used[:, None, :] & (t.qlo > 0) & (t.qlo < 250))[0]
    node, axis, slot = (int(x) for x in at)
    row, col = ((1, 2), (2, 0), (2, 2))[axis]
    bad = q2.copy()
    bad[node, row, col] += np.uint32(2 << (8 * slot))
    assert 'Q4' in tc.failing(moved, tree['leaf'], w2, bad, n)


def test_the_permission_rule_and_the_growth_figure():
    import ctypes as C
    from ptina_amd import _lib
    lib = _lib.load_library()
    why = C.create_string_buffer(256)

    def rule(state, built, on_device, n):
        return lib.mpt_refit_allowed(state, built, on_device, n, why, len(why)), why.value.decode()
    assert rule(1, 34, 1, 34) == (0, '')
    for args, verdict, words in (((0, 0, 0, 34), 1, 'no tree was ever built'), ((2, 34, 1, 34), 2, 'option'),
                                 ((3, 34, 1, 34), 3, 'build failed'), ((1, 34, 0, 34), 4, 'gpu_build = 0'),
                                 ((1, 34, 1, 35), 5, '35 faces, the tree was built for 34'), ((7, 34, 1, 34), 1, 'no tree')):
        rc, msg = rule(*args)
        assert rc == verdict and words in msg and msg.endswith('call build_tree()'), (args, rc, msg)
    assert lib.mpt_refit_allowed(1, 5, 1, 6, None, 0) == 5                  # no room for the words: the verdict alone
    assert rule(1, 0, 1, 0) == (0, '') and rule(1, 1, 1, 1) == (0, '')      # 0 and 1 faces are legal
    assert lib.mpt_refit_growth(0, 0) == 1.0 and lib.mpt_refit_growth(0, 5) == 1.0
    assert lib.mpt_refit_growth(1 << 40, 1 << 40) == 1.0
    assert lib.mpt_refit_growth(1 << 40, 3 << 39) == 1.5
    assert lib.mpt_refit_growth(3, 2**64 - 1) == float(2**64 - 1) / 3.0


def test_the_facade_has_the_refit_calls():
    from ptina_amd import worker
    from ptina_amd.tree.lbvh import BVHTree, DEFAULT_MAX_GROWTH
    assert callable(worker.refit_tree) and callable(worker.update_tree)
    assert all(callable(getattr(BVHTree, k)) for k in ('refit', 'refit_stats', 'update', 'can_refit'))
    assert DEFAULT_MAX_GROWTH >= 1.0

'''
tests/record_checks.py earns its verdicts on the CPU: records built here by a small numpy builder (median split, DFS pre-order
numbering, boxes by min / max) are accepted, and one mutation per property is rejected by the property it breaks, by name.  The
numpy restatement of the triangle records is held word for word to ptina_amd/csrc/tri_records.h itself, compiled into the
stand-alone host program tools/tri_records_check.cpp.
'''

import os
import shutil
import subprocess

import numpy as np
import pytest

import record_checks as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32
SIZES = [2, 3, 33]


# ---------------------------------------------------------------- models and a builder
def _model(n, seed, duplicates=False):
    '''[3n][8] vertices (pos3 nrm3 uv2) and [n] material ids: triangles of edge ~0.05 in the unit cube'''
    rng = np.random.default_rng(seed)
    v = np.zeros((n, 3, 8), F)
    v[:, :, 0:3] = (rng.uniform(0, 1, (n, 1, 3)) + rng.uniform(-0.05, 0.05, (n, 3, 3))).astype(F)
    nrm = rng.normal(size=(n, 3, 3))
    v[:, :, 3:6] = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(F)
    v[:, :, 6:8] = rng.uniform(0, 1, (n, 3, 2)).astype(F)
    if duplicates:
        v[n // 2:n // 2 + 3] = v[1]                          # exact duplicates: equal boxes, equal centres
    return v.reshape(3 * n, 8), rng.integers(-1, 5, n).astype(np.int32)


def _build(verts, leaf):
    '''valid records over the leaf order `leaf` (slot -> face): a median split over the widest axis of the centres, ties by slot,
    numbered in DFS pre-order.  -> (records as BVHTree().records() gives them, the tree as to_numpy() gives it).  The reference
    arrays describe the same tree, so the records are valid for tree = 0 and for tree = 1'''
    n = len(leaf)
    ni = max(n - 1, 0)
    pos = rc.positions(verts)[np.asarray(leaf)]
    llo, lhi = pos.min(axis=1), pos.max(axis=1)
    ctr = (F(0.5) * (llo + lhi)).astype(F)
    ids = np.zeros((ni, 2), np.int64)
    blo, bhi = np.zeros((ni, 3), F), np.zeros((ni, 3), F)
    depth = 0
    todo = [(np.arange(n), 0, 1)] if ni else []
    while todo:
        slots, me, dep = todo.pop()
        depth = max(depth, dep)
        blo[me], bhi[me] = llo[slots].min(axis=0), lhi[slots].max(axis=0)
        axis = int(np.argmax(ctr[slots].max(axis=0) - ctr[slots].min(axis=0)))
        slots = slots[np.lexsort((slots, ctr[slots, axis]))]
        m = len(slots) // 2
        for k, (part, number) in enumerate(((slots[:m], me + 1), (slots[m:], me + m))):
            if len(part) == 1:
                ids[me, k] = ~part[0]
            else:
                ids[me, k] = number
                todo.append((part, number, dep + 1))
    fnode = np.zeros((ni, 4, 4), U)
    for i in range(ni):
        for k in range(2):
            c = ids[i, k]
            lo, hi = (llo[~c], lhi[~c]) if c < 0 else (blo[c], bhi[c])
            fnode[i, 0:3, k] = lo.view(U)
            fnode[i, 0:3, 2 + k] = hi.view(U)
            fnode[i, 3, k] = np.int32(c).view(U)
    fnode[:, 3, 2:4] = 0xdeadbeef                            # (unspecified words: the checker must not look)
    child = np.where(ids < 0, ~ids, ids + n).astype(np.int32)
    snode = np.zeros((ni, 2, 4), U)
    snode[:, 0, 0:3], snode[:, 1, 0:3] = blo.view(U), bhi.view(U)
    snode[:, :, 3] = child.view(U)
    rec = dict(fnode=fnode, snode=snode)
    tree = dict(child=child, leaf=np.asarray(leaf, np.int32), bmin=blo, bmax=bhi, depth=depth)
    return rec, tree


def _case(n, seed=None, duplicates=False):
    verts, mtl = _model(n, n if seed is None else seed, duplicates)
    leaf = np.random.default_rng(1000 + n).permutation(n)
    rec, tree = _build(verts, leaf)
    rec.update(rc.triangle_records(verts, mtl, leaf))
    return verts, mtl, rec, tree


def _check(verts, mtl, rec, tree, sah=True):
    n = len(tree['leaf'])
    return rc.check_all(verts, mtl, rec, tree, n, sah, fast_depth=tree['depth'])


def _scalar_cost(fnode, n):
    '''B6 once more, one child at a time in numpy scalars: what rc.cost is held to here'''
    f = np.ascontiguousarray(fnode).view(F).reshape(-1, 4, 4)

    def area(lo, hi):
        d = [max(F(hi[a] - lo[a]), F(0)) for a in range(3)]
        return F(F(F(d[0] * d[1]) + F(d[1] * d[2])) + F(d[2] * d[0]))
    root = area([min(f[0, a, 0], f[0, a, 1]) for a in range(3)], [max(f[0, a, 2], f[0, a, 3]) for a in range(3)])
    total = 0
    for i in range(n - 1):
        for k in range(2):
            r = float(area(f[i, 0:3, k], f[i, 0:3, 2 + k])) / float(root)
            total += int(min(max(r, 0.0), 1.0) * 2.0 ** 40)
    return total


# ---------------------------------------------------------------- valid records are accepted
@pytest.mark.parametrize('n', SIZES)
def test_valid_records_are_accepted(n):
    verts, mtl, rec, tree = _case(n)
    for sah in (True, False):
        b = _check(verts, mtl, rec, tree, sah)
        assert b.ni == n - 1
    assert rc.levels(b.ids) == tree['depth'] >= 1
    want = _scalar_cost(rec['fnode'], n)
    assert rc.cost(rec['fnode'], n) == want and want > 0
    rc.check_b6(rec['fnode'], n, want / 2.0 ** 40)


def test_a_model_with_exact_duplicates_is_accepted():
    verts, mtl, rec, tree = _case(33, duplicates=True)
    pos = rc.positions(verts)
    assert np.array_equal(pos[16], pos[1]) and np.array_equal(pos[18], pos[1])
    for sah in (True, False):
        _check(verts, mtl, rec, tree, sah)
    rc.check_b6(rec['fnode'], 33, _scalar_cost(rec['fnode'], 33) / 2.0 ** 40)


@pytest.mark.parametrize('n', [0, 1])
def test_no_nodes(n):
    verts, mtl = _model(n, 5)
    rec, tree = _build(verts, np.arange(n))
    rec.update(rc.triangle_records(verts, mtl, np.arange(n)))
    assert rec['tfast'].shape == (n + 1, 3, 4) and rec['fnode'].shape == (0, 4, 4)
    _check(verts, mtl, rec, tree)
    assert rc.cost(rec['fnode'], n) == 0 and rc.levels(np.zeros((0, 2))) == 0
    rc.check_b6(rec['fnode'], n, 0.0)


# ---------------------------------------------------------------- one mutation per property
def _ulp_step(word, up):
    x = np.array([word], U).view(F)
    return np.nextafter(x, F(np.inf) if up else F(-np.inf)).view(U)[0]


def _inner_child(rec, tree, which=0):
    '''(node, child) of the which-th internal child'''
    at = np.argwhere(tree['child'] >= len(tree['leaf']))
    return tuple(int(x) for x in at[which])


def _leaf_child(rec, tree, deep=True):
    '''(node, child, slot) of a leaf child, below the root's record if deep'''
    n = len(tree['leaf'])
    at = [a for a in np.argwhere(tree['child'] < n) if not deep or a[0] > 0][0]
    return int(at[0]), int(at[1]), int(tree['child'][at[0], at[1]])


def _copy(rec):
    return {k: np.array(v, copy=True) for k, v in rec.items()}


WHERE = r'node \d+ axis [xyz] child [01]: .*0x[0-9a-f]{8} \(.*\) != 0x[0-9a-f]{8}'


@pytest.mark.parametrize('side,up', [(0, False), (0, True), (2, True), (2, False)])
def test_an_inner_box_one_ulp_off_is_rejected_by_B3(side, up):
    '''lo lowered / hi raised: grown, still enclosing -- what no ray and no film can show; the other two: shrunk'''
    verts, mtl, rec, tree = _case(33)
    i, k = _inner_child(rec, tree, 3)
    bad = _copy(rec)
    bad['fnode'][i, 1, side + k] = _ulp_step(rec['fnode'][i, 1, side + k], up)
    with pytest.raises(AssertionError, match=r'^B3: ' + WHERE):
        _check(verts, mtl, bad, tree)


def test_a_leaf_box_from_the_wrong_face_is_rejected_by_B2():
    verts, mtl, rec, tree = _case(33)
    i, k, slot = _leaf_child(rec, tree)
    other = rc.positions(verts)[tree['leaf'][(slot + 1) % 33]]
    bad = _copy(rec)
    bad['fnode'][i, 0:3, k] = other.min(axis=0).view(U)
    bad['fnode'][i, 0:3, 2 + k] = other.max(axis=0).view(U)
    with pytest.raises(AssertionError, match=r'^B2: ' + WHERE):
        _check(verts, mtl, bad, tree)


def test_stale_boxes_after_a_vertex_moved_are_rejected_by_B2_and_B3():
    verts, mtl, rec, tree = _case(33)
    i, k, slot = _leaf_child(rec, tree)
    face = int(tree['leaf'][slot])
    moved = verts.copy()
    moved[3 * face + 1, 0:3] += F(2.0)
    stale = _copy(rec)
    stale.update(rc.triangle_records(moved, mtl, tree['leaf']))
    with pytest.raises(AssertionError, match=rf'^B2: node {i} axis [xyz] child {k}: .*leaf slot {slot} \(face {face}\)'):
        _check(moved, mtl, stale, tree)
    tri = rc.positions(moved)[face]                          # the leaf's own box fitted again, its ancestors' left as they were
    stale['fnode'][i, 0:3, k] = tri.min(axis=0).view(U)
    stale['fnode'][i, 0:3, 2 + k] = tri.max(axis=0).view(U)
    with pytest.raises(AssertionError, match=rf'^B3: .*the two boxes in node {i}\b'):
        _check(moved, mtl, stale, tree)
    fitted, _ = _build(moved, tree['leaf'])                  # (the same topology only if the split does not move: not assumed)
    fitted.update(rc.triangle_records(moved, mtl, tree['leaf']))
    _check(moved, mtl, fitted, _build(moved, tree['leaf'])[1])


def test_a_duplicated_slot_is_rejected_by_B1():
    verts, mtl, rec, tree = _case(33)
    i, k, slot = _leaf_child(rec, tree)
    bad = _copy(rec)
    bad['fnode'][i, 3, k] = np.int32(~((slot + 1) % 33)).view(U)
    with pytest.raises(AssertionError, match=rf'^B1: slot ({slot}|{(slot + 1) % 33}): appears (0|2) times'):
        _check(verts, mtl, bad, tree)


def test_topology_errors_are_rejected_by_B1():
    verts, mtl, rec, tree = _case(33)
    i, k = _inner_child(rec, tree, 2)
    for value, what in ((0, 'node 0 is named as a child'), (32, 'id out of range'), (-34, 'id out of range'),
                        (int(tree['child'][_inner_child(rec, tree, 4)] - 33), r'has (0|2) parents')):
        bad = _copy(rec)
        bad['fnode'][i, 3, k] = np.int32(value).view(U)
        with pytest.raises(AssertionError, match=r'^B1: .*' + what):
            _check(verts, mtl, bad, tree)


def test_two_sibling_subtrees_renumbered_are_rejected_by_B4():
    '''the right subtree's nodes numbered before the left one's: every box, every parent and every slot is still right'''
    verts, mtl, rec, tree = _case(33)
    n, ids = 33, np.where(tree['child'] < 33, -1, tree['child'] - 33)
    me = 0
    left, right = int(ids[me, 0]), int(ids[me, 1])
    assert left == me + 1 and right > left
    nl, nr = right - left, (n - 1) - right                   # nodes in the two subtrees of the root
    perm = np.arange(n - 1)
    perm[left:right] += nr
    perm[right:] -= nl
    bad = _copy(rec)
    bad['fnode'][perm] = rec['fnode']
    moved_ids = bad['fnode'][:, 3, 0:2].view(np.int32)
    moved_ids[moved_ids >= 0] = perm[moved_ids[moved_ids >= 0]]
    b = rc.Binary(bad['fnode'], n)
    rc.check_b1(b)
    rc.check_b2(b, rc.positions(verts), tree['leaf'])
    rc.check_b3(b)
    with pytest.raises(AssertionError, match=r'^B4: node 0 child 0: not the DFS pre-order number'):
        rc.check_binary(rc.positions(verts), tree['leaf'], bad['fnode'], n, True)
    assert rc.cost(bad['fnode'], n) == rc.cost(rec['fnode'], n)


def test_records_that_are_not_the_reference_trees_are_rejected_by_B4_and_N1():
    verts, mtl, rec, tree = _case(33)
    i, k = _inner_child(rec, tree, 1)
    other = dict(tree, bmin=tree['bmin'].copy())
    node = int(tree['child'][i, k]) - 33
    other['bmin'][node, 2] = np.nextafter(other['bmin'][node, 2], F(-1))
    with pytest.raises(AssertionError, match=r'^B4: ' + WHERE):
        rc.check_binary(rc.positions(verts), tree['leaf'], rec['fnode'], 33, False, other)
    with pytest.raises(AssertionError, match=rf'^N1: node {node} row 0 word 2: '):
        rc.check_n1(rec['snode'], other, 33)
    swapped = dict(tree, child=tree['child'][:, ::-1].copy())
    with pytest.raises(AssertionError, match=r'^B4: node 0 child 0: the id is not'):
        rc.check_binary(rc.positions(verts), tree['leaf'], rec['fnode'], 33, False, swapped)
    with pytest.raises(AssertionError, match=r'^N1: node 0 row 0 word 3: '):
        rc.check_n1(rec['snode'], swapped, 33)


def test_a_wrong_depth_is_rejected_by_B5():
    verts, mtl, rec, tree = _case(33)
    with pytest.raises(AssertionError, match=rf'^B5: the records have {tree["depth"]} levels, option fast_depth says {tree["depth"] + 1}'):
        rc.check_all(verts, mtl, rec, tree, 33, True, fast_depth=tree['depth'] + 1)
    with pytest.raises(AssertionError, match=r'^B5: .*tree_depth'):
        rc.check_all(verts, mtl, rec, dict(tree, depth=tree['depth'] - 1), 33, True)
    chain = np.array([[1, -1], [2, -2], [-3, -4]])           # a tree that is one path: three levels
    assert rc.levels(chain) == 3 and rc.levels(chain[2:]) == 1


@pytest.mark.parametrize('off', [1, -1])
def test_a_cost_off_by_one_is_rejected_by_B6(off):
    verts, mtl, rec, tree = _case(33)
    want = rc.cost(rec['fnode'], 33)
    rc.check_b6(rec['fnode'], 33, want / 2.0 ** 40)
    with pytest.raises(AssertionError, match=r'^B6: cost_now is .* the records give'):
        rc.check_b6(rec['fnode'], 33, (want + off) / 2.0 ** 40, 'cost_now')
    grown = _copy(rec)                                       # and a box one ulp larger is a different integer
    i, k = _inner_child(rec, tree, 3)
    grown['fnode'][i, 1, 2 + k] = _ulp_step(rec['fnode'][i, 1, 2 + k], True)
    assert rc.cost(grown['fnode'], 33) > want


def test_tfast_with_a_and_c_exchanged_is_rejected_by_T2():
    verts, mtl, rec, tree = _case(33)
    bad = _copy(rec)
    bad['tfast'][7, 1, 0:3], bad['tfast'][7, 2, 0:3] = rec['tfast'][7, 2, 0:3], rec['tfast'][7, 1, 0:3]
    with pytest.raises(AssertionError, match=rf'^T2: slot 7 row 1 word 0: tfast of face {tree["leaf"][7]}: 0x[0-9a-f]{{8}} .* != 0x[0-9a-f]{{8}}'):
        _check(verts, mtl, bad, tree)


@pytest.mark.parametrize('word', [0x3f800000, 0x7fc00000, 0])
def test_a_sentinel_that_is_not_all_ones_is_rejected_by_T2(word):
    '''finite, or a NaN of other bits: the sentinel's words are specified, the both-NaN rule does not apply to it'''
    verts, mtl, rec, tree = _case(33)
    bad = _copy(rec)
    bad['tfast'][33, 2, 1] = word
    with pytest.raises(AssertionError, match=r'^T2: sentinel 0 row 2 word 1: the sentinel record 33 is not all ones'):
        _check(verts, mtl, bad, tree)
    with pytest.raises(AssertionError, match=r'^T2: tfast has shape'):
        rc.check_t2(rec['tfast'][:33], rc.triangle_records(verts, mtl, tree['leaf']), tree['leaf'])


def test_tshade_with_uv_1_and_2_exchanged_is_rejected_by_T3():
    verts, mtl, rec, tree = _case(33)
    bad = _copy(rec)
    s = bad['tshade'].reshape(33, 16)
    s[5, 11:13], s[5, 13:15] = rec['tshade'].reshape(33, 16)[5, 13:15], rec['tshade'].reshape(33, 16)[5, 11:13]
    with pytest.raises(AssertionError, match=r'^T3: slot 5 row 2 word 3: tshade of face'):
        _check(verts, mtl, bad, tree)
    bad = _copy(rec)
    bad['tshade'][5, 3, 3] ^= 1                              # the material id
    with pytest.raises(AssertionError, match=r'^T3: slot 5 row 3 word 3'):
        _check(verts, mtl, bad, tree)


def test_D_with_the_sign_flipped_is_rejected_by_T1():
    verts, mtl, rec, tree = _case(33)
    bad = _copy(rec)
    bad['tgeo'][9, 0, 3] ^= 0x80000000
    with pytest.raises(AssertionError, match=r'^T1: slot 9 row 0 word 3: tgeo of face'):
        _check(verts, mtl, bad, tree)


def test_the_comparison_rules():
    nan_a, nan_b = np.array([0x7fc00000], U), np.array([0xffc00001], U)
    pz, nz = np.array([0x00000000], U), np.array([0x80000000], U)
    assert rc.same_words(nan_a, nan_b).all() and not rc.same_words(nan_a, np.array([0x7f800000], U)).any()
    assert not rc.same_words(pz, nz).any() and rc.same_boxes(pz, nz).all() and rc.same_boxes(nan_a, nan_b).all()
    assert not rc.same_boxes(pz, np.array([1], U)).any()     # (the smallest denormal is not a zero)
    verts, mtl, rec, tree = _case(3)
    verts = verts.copy()
    verts[0:3, 1] = F(0.0)                                   # a triangle in the plane y = 0: u.y = v.y = +0.0
    rec, tree = _build(verts, tree['leaf'])
    rec.update(rc.triangle_records(verts, mtl, tree['leaf']))
    _check(verts, mtl, rec, tree)
    slot = int(np.flatnonzero(tree['leaf'] == 0)[0])
    assert rec['tgeo'][slot, 1, 1] == 0
    bad = _copy(rec)
    bad['tgeo'][slot, 1, 1] = 0x80000000
    with pytest.raises(AssertionError, match=rf'^T1: slot {slot} row 1 word 1'):
        _check(verts, mtl, bad, tree)


# ---------------------------------------------------------------- the restatement against tri_records.h itself
@pytest.fixture(scope='module')
def tri_tool(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('tri_records') / 'tri_records_check')
    subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', os.path.join(ROOT, 'tools', 'tri_records_check.cpp'), '-o', exe],
                   check=True, capture_output=True, text=True)
    return exe


def _scaled(f):
    v, m = _model(33, 33)
    v = v.copy()
    v[:, 0:3] *= F(f)
    return v, m


def _zero_area():
    v, m = _model(7, 7)
    v = v.copy().reshape(7, 3, 8)
    v[2, 1, 0:3] = v[2, 0, 0:3]                              # two vertices in one place
    v[4, 2, 0:3] = v[4, 0, 0:3] + F(2.0) * (v[4, 1, 0:3] - v[4, 0, 0:3])     # three on a line
    v[5, :, 0:3] = v[5, 0, 0:3]                              # a point
    return v.reshape(21, 8), m


TOOL_MODELS = {'n2': lambda: _model(2, 2), 'n3': lambda: _model(3, 3), 'n33': lambda: _model(33, 33),
               'duplicates': lambda: _model(33, 33, True), 'times_1e18': lambda: _scaled(1e18), 'times_1e-18': lambda: _scaled(1e-18),
               'zero_area': _zero_area}


@pytest.mark.parametrize('name', list(TOOL_MODELS))
def test_the_numpy_restatement_gives_the_headers_words(tri_tool, tmp_path, name):
    verts, mtl = TOOL_MODELS[name]()
    n = mtl.shape[0]
    with open(tmp_path / 'model.bin', 'wb') as f:
        f.write(np.int32(n).tobytes() + np.ascontiguousarray(verts, F).tobytes() + np.ascontiguousarray(mtl, np.int32).tobytes())
    subprocess.run([tri_tool, str(tmp_path / 'model.bin'), str(tmp_path / 'records.bin')], check=True, capture_output=True)
    words = np.fromfile(tmp_path / 'records.bin', U)
    assert words.size == n * 44
    got = dict(tgeo=words[:n * 16].reshape(n, 4, 4), tfast=words[n * 16:n * 28].reshape(n, 3, 4), tshade=words[n * 28:].reshape(n, 4, 4))
    want = rc.triangle_records(verts, mtl, np.arange(n))
    rc.check_t1(got['tgeo'], want, np.arange(n))
    rc.check_t2(np.concatenate([got['tfast'], want['tfast'][n:]]), want, np.arange(n))
    rc.check_t3(got['tshade'], want, np.arange(n))
    nans = int(np.isnan(got['tfast'].view(F)).sum()) + int(np.isnan(got['tgeo'].view(F)).sum())
    if name in ('times_1e18', 'times_1e-18', 'zero_area'):
        assert nans > 0, 'the model was to reach inf - inf (overflow) or 0 / 0 (underflow, no area)'
    else:
        assert nans == 0 and np.isfinite(got['tfast'].view(F)).all()
    if name == 'times_1e18':
        assert np.isnan(got['tgeo'][:, 0, 3].view(F)).all()  # D = inf - inf for every triangle

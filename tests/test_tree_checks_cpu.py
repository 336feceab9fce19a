'''
tests/tree_checks.py rejects wrong trees (no GPU).

Valid records come from a small generator that belongs to this file: a median split over 46 triangles, its 4-wide
collapse, exact boxes, a quantisation done in f64 and rounded outwards.  It is a fixture, not the product's pass: other
splits, another collapse rule, other arithmetic.  check_all must accept it; then one record field is changed at a time
and the property named for that change must be the one check_all reports -- and, checked one by one, the only property
that fails, except where a second one follows from the change by necessity (said at the mutation).
'''

import numpy as np
import pytest

import tree_checks as tc

F = np.float32
Q_LO = ((1, 2), (2, 0), (2, 2))        # (row, column) of the qlo / qhi / scale word of an axis in a quantised record
Q_HI = ((1, 3), (2, 1), (2, 3))
Q_SCALE = ((0, 3), (1, 0), (1, 1))


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


def _model():
    rng = np.random.default_rng(46)
    cen = rng.uniform(-1.0, 1.0, size=(40, 1, 3))
    pos = (cen + rng.normal(size=(40, 3, 3)) * 0.2).astype(F)
    pos[7] = pos[5]                                             # an exact duplicate
    flat = (np.array([10.0, 0.0, 0.0]) + rng.uniform(-1.0, 1.0, size=(6, 3, 3))).astype(F)
    flat[:, :, 2] = F(3.0)                                      # six triangles in the plane z = 3, away from the rest
    return np.concatenate([pos, flat])


def _build(pos):
    '''-> leaf [n], wnode [nw][8][4], qnode [nw][4][4] (uint32)'''
    n = len(pos)
    tlo, thi = pos.min(axis=1), pos.max(axis=1)
    ctr = pos.astype(np.float64).mean(axis=1)
    leaf, nodes = [], []                 # binary nodes: [left, right, count]; a child >= 0 is a node, < 0 is ~slot

    def split(faces):
        if len(faces) == 1:
            leaf.append(int(faces[0]))
            return ~(len(leaf) - 1)
        c = ctr[faces]
        axis = int(np.argmax(c.max(axis=0) - c.min(axis=0)))
        faces = faces[np.argsort(c[:, axis], kind='stable')]
        me = len(nodes)
        nodes.append([0, 0, len(faces)])
        nodes[me][0] = split(faces[:len(faces) // 2])
        nodes[me][1] = split(faces[len(faces) // 2:])
        return me
    split(np.arange(n))
    leaf = np.array(leaf)

    def box(ch):
        if ch < 0:
            return tlo[leaf[~ch]], thi[leaf[~ch]]
        (l0, h0), (l1, h1) = box(nodes[ch][0]), box(nodes[ch][1])
        return np.minimum(l0, l1), np.maximum(h0, h1)

    grown_from, recs = [0], []
    w = 0
    while w < len(grown_from):           # breadth first: children come after their parents
        ch = nodes[grown_from[w]][:2]
        while len(ch) < 4 and any(c >= 0 for c in ch):
            big = max((c for c in ch if c >= 0), key=lambda c: nodes[c][2])      # the child with the most triangles
            at = ch.index(big)
            ch[at] = nodes[big][0]
            ch.append(nodes[big][1])
        ids, boxes = [], []
        for c in ch:
            boxes.append(box(c))
            if c < 0:
                ids.append(c)
            else:
                ids.append(len(grown_from))
                grown_from.append(c)
        recs.append((ids, boxes))
        w += 1
    nw = len(recs)
    wn = np.zeros((nw, 8, 4), np.uint32)
    qn = np.zeros((nw, 4, 4), np.uint32)
    for w, (ids, boxes) in enumerate(recs):
        k = len(ids)
        idv = np.array(ids + [~n] * (4 - k), np.int32)
        lo = np.full((3, 4), 1e30, F)
        hi = np.full((3, 4), 1e30, F)
        for j, (l, h) in enumerate(boxes):
            lo[:, j], hi[:, j] = l, h
        wn[w, 0:6:2] = _bits(lo)
        wn[w, 1:6:2] = _bits(hi)
        wn[w, 6] = idv.view(np.uint32)
        qn[w, 3] = idv.view(np.uint32)
        for a in range(3):
            o, top = lo[a, :k].min(), hi[a, :k].max()
            e = float(top) - float(o)
            if e == 0.0:
                s = max(F(abs(o)) * F(1e-6), F(1e-30))
            else:
                s = F(e / 255.0)
                if float(s) * 255.0 < e:
                    s = np.nextafter(s, F(np.inf))
                while F(o + F(255) * s) < top:
                    s = np.nextafter(s, F(np.inf))
            ql = np.full(4, 255, np.int64)
            qh = np.zeros(4, np.int64)
            ql[:k] = np.clip(np.floor((lo[a, :k].astype(np.float64) - float(o)) / float(s) - 0.25), 0, 255)
            qh[:k] = np.clip(np.ceil((hi[a, :k].astype(np.float64) - float(o)) / float(s) + 0.25), 0, 255)
            qn[w, 0, a] = _bits(o)
            qn[w][Q_SCALE[a]] = _bits(s)
            qn[w][Q_LO[a]] = sum(int(ql[j]) << (8 * j) for j in range(4))
            qn[w][Q_HI[a]] = sum(int(qh[j]) << (8 * j) for j in range(4))
    return leaf, wn, qn


@pytest.fixture(scope='module')
def valid():
    pos = _model()
    leaf, wn, qn = _build(pos)
    for a in (pos, leaf, wn, qn):
        a.setflags(write=False)
    return pos, leaf, wn, qn, len(pos)


def _mutated(valid, change):
    pos, leaf, wn, qn, n = valid
    wn, qn = wn.copy(), qn.copy()
    change(tc.Tree(pos, leaf, wn, qn, n), wn, qn)
    return pos, leaf, wn, qn, n


def _expect(rec, first, everything=None):
    with pytest.raises(AssertionError) as err:
        tc.check_all(*rec)
    assert str(err.value).startswith(first + ':'), str(err.value)
    assert 'node' in str(err.value)
    assert tc.failing(*rec) == sorted(everything or [first]), str(err.value)
    return str(err.value)


def _step(wn, at, up):
    '''move the f32 at wn[at] by one ulp'''
    x = np.array([wn[at]], np.uint32).view(F)
    wn[at] = np.nextafter(x, F(np.inf) if up else F(-np.inf)).view(np.uint32)[0]


def _set_byte(qn, node, word, slot, value):
    assert 0 <= value <= 255
    v = int(qn[node][word])
    qn[node][word] = (v & ~(255 << (8 * slot))) | (int(value) << (8 * slot))


def test_the_fixture_is_accepted_and_has_what_the_mutations_need(valid):
    pos, leaf, wn, qn, n = valid
    t = tc.check_all(*valid)
    assert tc.failing(*valid) == []
    used = t.used.sum(axis=1)
    assert (used == 2).any() and (used == 3).any() and (used == 4).any(), 'nodes with unused slots, and full ones'
    e = t.node_hi - t.origin
    assert (e[:, 2] == 0).any() and (e > 0).all(axis=1).any(), 'a node that is flat along z, and ordinary ones'
    assert sorted(leaf) == list(range(n)) and not np.array_equal(leaf, np.arange(n))
    m = tc.q_margins(t)
    assert 0.25 <= m['q4_min_steps'] and m['q5_max_steps'] <= 1.25
    assert tc.levels(t.ids, n) >= 3 and tc.stack_need(t.ids, n) >= 5


def _inner_child_below_the_node_top(t):
    '''an internal child whose hi is not its node's on some axis: moving it changes no other box'''
    for w, k in np.argwhere(t.inner):
        for a in range(3):
            if t.hi[w, a, k] < t.node_hi[w, a]:
                return int(w), int(a), int(k)
    raise AssertionError('no such child')


@pytest.mark.parametrize('up', [False, True], ids=['one_ulp_short', 'one_ulp_large'])
def test_an_internal_box_one_ulp_off_is_E2(valid, up):
    def change(t, wn, qn):
        w, a, k = _inner_child_below_the_node_top(t)
        _step(wn, (w, 2 * a + 1, k), up)
    msg = _expect(_mutated(valid, change), 'E2')
    assert 'child' in msg and 'axis' in msg


def test_two_leaf_ids_swapped_between_nodes_is_E1(valid):
    def change(t, wn, qn):
        at = [(int(w), int(k)) for w, k in np.argwhere(t.leafc) if t.leaf[~t.ids[w, k]] not in (5, 7)]
        (w0, k0), (w1, k1) = at[0], next(x for x in at if x[0] != at[0][0])
        for r, row in ((wn, 6), (qn, 3)):
            r[w0, row, k0], r[w1, row, k1] = r[w1, row, k1], r[w0, row, k0]
    _expect(_mutated(valid, change), 'E1')


def test_a_triangle_named_twice_is_E4(valid):
    '''faces 5 and 7 are the same triangle, so the slot that should name 7 and names 5 still holds the right box'''
    def change(t, wn, qn):
        s5, s7 = int(np.flatnonzero(t.leaf == 5)[0]), int(np.flatnonzero(t.leaf == 7)[0])
        w, k = np.argwhere(t.ids == ~s7)[0]
        wn[w, 6, k] = qn[w, 3, k] = np.array(~s5, np.int32).view(np.uint32)
    assert 'triangle slot' in _expect(_mutated(valid, change), 'E4')


def test_id_0_in_an_unused_slot_is_E3(valid):
    def change(t, wn, qn):
        w, k = np.argwhere(t.empty)[0]
        wn[w, 6, k] = qn[w, 3, k] = 0
    _expect(_mutated(valid, change), 'E3')


def test_a_changed_quantised_id_is_Q1(valid):
    def change(t, wn, qn):
        w, k = np.argwhere(t.leafc)[0]
        w2, k2 = np.argwhere(t.leafc)[-1]
        qn[w, 3, k] = qn[w2, 3, k2]
    _expect(_mutated(valid, change), 'Q1')


def test_origin_one_ulp_up_is_Q2(valid):
    '''... and Q4 by necessity: the child that sets the node's lo holds byte 0, and Q4 asks origin <= lo of it exactly'''
    def change(t, wn, qn):
        w = int(np.flatnonzero((t.node_hi - t.origin > 0).all(axis=1))[0])
        _step(qn, (w, 0, 1), True)
    _expect(_mutated(valid, change), 'Q2', ['Q2', 'Q4'])


@pytest.mark.parametrize('factor', [2.0, 0.5], ids=['doubled', 'halved'])
def test_a_wrong_scale_is_Q3(valid, factor):
    '''on a flat axis (every child at bytes 0 and 1, which stay outward and within 1.26 of any positive step) nothing but Q3
    can notice; on an ordinary axis the planes move with the step, so Q4 or Q5 fail behind Q3'''
    def flat(t, wn, qn):
        w = int(np.flatnonzero(t.node_hi[:, 2] - t.origin[:, 2] == 0)[0])
        qn[w][Q_SCALE[2]] = _bits(t.scale[w, 2] * F(factor))
    _expect(_mutated(valid, flat), 'Q3')

    def ordinary(t, wn, qn):
        qn[0][Q_SCALE[0]] = _bits(t.scale[0, 0] * F(factor))
    rec = _mutated(valid, ordinary)
    with pytest.raises(AssertionError, match='^Q3: node 0 axis x'):
        tc.check_all(*rec)
    assert set(tc.failing(*rec)) in ({'Q3', 'Q4'}, {'Q3', 'Q5'}, {'Q3', 'Q4', 'Q5'})


def _plane_with_margin_under_a_step(t, high):
    o, s = t.origin.astype(np.float64)[:, :, None], t.scale.astype(np.float64)[:, :, None]
    if high:
        margin = (o + t.qhi * s - t.hi) / s
        ok = (t.qhi < 255) & (t.qhi > 0)
    else:
        margin = (t.lo - (o + t.qlo * s)) / s
        ok = (t.qlo > 0) & (t.qlo < 255)
    w, a, k = np.argwhere(np.broadcast_to(t.used[:, None, :], ok.shape) & ok & (margin < 1.0))[0]
    return int(w), int(a), int(k)


def test_a_high_plane_one_byte_inwards_is_Q4(valid):
    def change(t, wn, qn):
        w, a, k = _plane_with_margin_under_a_step(t, True)
        _set_byte(qn, w, Q_HI[a], k, t.qhi[w, a, k] - 1)
    assert 'high plane' in _expect(_mutated(valid, change), 'Q4')


def test_a_low_plane_one_byte_inwards_is_Q4(valid):
    def change(t, wn, qn):
        w, a, k = _plane_with_margin_under_a_step(t, False)
        _set_byte(qn, w, Q_LO[a], k, t.qlo[w, a, k] + 1)
    assert 'low plane' in _expect(_mutated(valid, change), 'Q4')


def test_a_high_plane_three_bytes_outwards_is_Q5(valid):
    def change(t, wn, qn):
        u = np.broadcast_to(t.used[:, None, :], t.qhi.shape)
        w, a, k = np.argwhere(u & (t.qhi > 0) & (t.qhi + 3 < 255))[0]
        _set_byte(qn, w, Q_HI[a], k, t.qhi[w, a, k] + 3)
    _expect(_mutated(valid, change), 'Q5')


def test_an_unused_slot_with_qlo_0_is_Q6(valid):
    def change(t, wn, qn):
        w, k = np.argwhere(t.empty)[0]
        _set_byte(qn, w, Q_LO[1], k, 0)
    _expect(_mutated(valid, change), 'Q6')


def _ids(rows, n):
    return np.array([r + [~n] * (4 - len(r)) for r in rows], np.int32)


def test_stack_need_and_levels_on_hand_worked_trees():
    # a chain over 4 leaves: each node one leaf and the next node, the last one two leaves.
    #   need(2) = 2 - 1 = 1;  need(1) = (2 - 1) + need(2) = 2;  need(0) = (2 - 1) + need(1) = 3;  stack = 1 + 3 + 1
    chain = _ids([[~0, 1], [2, ~1], [~2, ~3]], 4)
    assert tc.levels(chain, 4) == 3 and tc.stack_need(chain, 4) == 5
    # a full 4-ary tree of two levels over 16 leaves: need(child) = 4 - 1 = 3;  need(0) = (4 - 1) + 3 = 6;  stack = 1 + 6 + 1
    full = _ids([[1, 2, 3, 4]] + [[~(4 * j + i) for i in range(4)] for j in range(4)], 16)
    assert tc.levels(full, 16) == 2 and tc.stack_need(full, 16) == 8
    # the deepest need decides, not the deepest level: node 1 (three leaves, need 2) against the chain 2 -> 3 (need 1 + 1)
    #   need(0) = (3 - 1) + max(2, 2) = 4 with three used slots;  stack = 6;  levels = 3
    mixed = _ids([[1, 2, ~0], [~1, ~2, ~3], [~4, 3], [~5, ~6]], 7)
    assert tc.levels(mixed, 7) == 3 and tc.stack_need(mixed, 7) == 6
    # one node, two leaves: the smallest tree there is
    assert tc.levels(_ids([[~0, ~1]], 2), 2) == 1 and tc.stack_need(_ids([[~0, ~1]], 2), 2) == 3


def _lbvh():
    '''four leaves by hand: root 0 = (node 1, node 2), node 1 = slots 0 1, node 2 = slots 2 3; faces 1 and 3 are one triangle'''
    n = 4
    pos = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0.5]],
                    [[2, 2, 2], [3, 2, 2], [2, 3, 2.25]],
                    [[-1, -1, -1], [-0.5, -1, -1], [-1, -0.5, -1]],
                    [[2, 2, 2], [3, 2, 2], [2, 3, 2.25]]], F) * F(1.1)
    leaf = np.array([2, 0, 3, 1], np.int32)
    lo, hi = pos.min(axis=1), pos.max(axis=1)
    bmin = np.array([np.minimum(lo[[2, 0]].min(axis=0), lo[[3, 1]].min(axis=0)), lo[[2, 0]].min(axis=0), lo[[3, 1]].min(axis=0)], F)
    bmax = np.array([np.maximum(hi[[2, 0]].max(axis=0), hi[[3, 1]].max(axis=0)), hi[[2, 0]].max(axis=0), hi[[3, 1]].max(axis=0)], F)
    tree = dict(child=np.array([[n + 1, n + 2], [0, 1], [2, 3]], np.int32), leaf=leaf, bmin=bmin, bmax=bmax,
                mc=np.array([1, 5, 5, 9], np.int32), depth=2)
    return pos, tree, n


def test_lbvh_checks_on_a_hand_made_tree():
    pos, tree, n = _lbvh()
    tc.check_lbvh(pos, tree, n)
    assert tc.failing_lbvh(pos, tree, n) == []

    short = dict(tree, bmax=tree['bmax'].copy())
    short['bmax'][2, 1] = np.nextafter(short['bmax'][2, 1], F(-np.inf))
    assert tc.failing_lbvh(pos, short, n) == ['L4']
    with pytest.raises(AssertionError, match='^L4: internal node 2 axis y'):
        tc.check_lbvh(pos, short, n)

    twice = dict(tree, leaf=np.array([2, 0, 3, 3], np.int32))       # (face 3 is face 1's twin: the boxes stay right)
    assert tc.failing_lbvh(pos, twice, n) == ['L1']

    unordered = dict(tree, mc=np.array([1, 5, 4, 9], np.int32))
    assert tc.failing_lbvh(pos, unordered, n) == ['L2']

    assert tc.failing_lbvh(pos, dict(tree, child=np.array([[n + 1, n + 2], [0, 1], [2, 2]], np.int32)), n) == ['L3']
    assert tc.failing_lbvh(pos, dict(tree, depth=3), n) == ['L5']

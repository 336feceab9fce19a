'''
An independent checker for the records the kernels fetch and tests/tree_checks.py never sees: the binary node records
(`fnode`, `snode`) and the triangle records (`tgeo`, `tfast`, `tshade`), as BVHTree().records() downloads them.  Plain numpy
over the downloaded words and the model's vertices, nothing imported from the package under test.  No comparison carries a
tolerance: every one is == on 32-bit words, with the two exceptions stated under `Comparison rules`.

The records (uint32 words; `leaf[slot]` is the face of the model a leaf slot holds, n the number of faces)
--------------------------------------------------------------------------------------------------------
  fnode  [n-1][4][4]  rows a = 0..2 {lo0[a], lo1[a], hi0[a], hi1[a]}: the boxes of the node's two children; row 3 {id0, id1, -, -}:
                      id >= 0 names a node, id < 0 leaf slot ~id.  Words 2 and 3 of the id row are unspecified (the device SAH
                      pass never writes them) and are never looked at
  snode  [n-1][2][4]  {bmin.xyz, child0} {bmax.xyz, child1}: the reference LBVH, a child < n is a leaf slot, a child >= n node child - n
  tgeo   [n][4][4]    by leaf slot: {v0, D} {u, uu} {v, uv} {n, vv}
  tfast  [n+1][3][4]  by leaf slot: {n, v0.x} {a, v0.y} {c, v0.z}; record n: every word 0xffffffff
  tshade [n][4][4]    by leaf slot: {n0.xyz, n1.x} {n1.yz, n2.xy} {n2.z, uv0.xy, uv1.x} {uv1.y, uv2.xy, material id}

Binary nodes
  B1  topology: every id is in range (-n <= id <= n - 2); node 0 is nobody's child; every node 1 .. n-2 has exactly one parent;
      every leaf slot 0 .. n-1 appears exactly once
  B2  a leaf child's box is the f32 min / max of the three vertices of face leaf[slot]
  B3  an internal child's box is the union (f32 min / max) of the two child boxes in the record it names.  With B2 this gives, by
      induction from the leaves, that every box encloses its subtree and is no larger
  B4  numbering.  SAH tree (option tree = 1): DFS pre-order -- an internal left child is me + 1, an internal right child is
      me + (leaves under the left child).  LBVH (tree = 0): the id row is the reference tree's `child` translated (ch < n: ~ch,
      else ch - n), and an internal child's box is that node's bmin / bmax
  B5  levels(ids), the number of levels of internal nodes with the root's being 1 (0 for a tree without nodes), equals the option
      the kernels size their stacks by: fast_depth for fnode, tree_depth for snode.  (tree_build.cpp counts the same thing: the
      host SAH pass starts the root at depth 1 and takes the maximum over the nodes, the LBVH passes likewise.)
  B6  cost: the sum over both children of every record of trunc(clamp(area(child) / area(root), 0, 1) * 2^40), as integers, where
      area = dx * dy + dy * dz + dz * dx in f32, left to right, over extents max(hi - lo, 0); area(root) is that of the union of
      record 0's two boxes, the ratio is taken in f64, and a root area that is not > 0 makes every share 0.  The figures
      refit_stats() reports are this integer over 2^40, exact in a double while the sum is below 2^53 (asserted first)
  N1  snode's rows are the reference tree's arrays bit for bit: {bmin, child0} {bmax, child1}

Triangle records (restated in numpy float32, one rounded operation per line, nothing fused)
  T1  tgeo: u = v1 - v0, v = v2 - v0, n = u x v, uu, uv, vv dot products summed left to right, D = uv * uv - uu * vv
  T2  tfast: {n, v0.x} {a, v0.y} {c, v0.z} with a = (uv v - vv u) / D, c = (uv u - uu v) / D; record n all ones
  T3  tshade: the three normals, the three uv pairs and the material id's integer bits

Comparison rules
  words    equal as uint32, except a position where both sides are NaN (inf - inf of a model scaled by 1e18, D = 0 of a degenerate
           triangle: the payload of a NaN an operation makes is not specified).  -0.0 and +0.0 are different words and must match.
           Used for T1 - T3, N1 and the ids
  boxes    as `words`, except that a zero equals a zero of the other sign: the records' boxes are made by min and max alone, and
           IEEE min / max do not say which of -0.0 and +0.0 they return.  Used for B2, B3 and the boxes of B4

Every check raises AssertionError with a message that starts with the property's name and names the node, the child, the axis
and the two values that disagree, in hex.
'''

import numpy as np

F = np.float32
U = np.uint32
AXES = 'xyz'
ONES = 0xffffffff

BINARY = ('B1', 'B2', 'B3', 'B4', 'B5', 'B6')
TRIANGLE = ('T1', 'T2', 'T3')


def _hex(x):
    x = np.asarray(x)
    if x.dtype == np.float32:
        return f'0x{int(x.view(U)):08x} ({float(x)!r})'
    if x.dtype == np.uint32:
        return f'0x{int(x):08x} ({float(x.view(F))!r})'
    return f'{int(x)}'


def _u(a):
    return np.ascontiguousarray(a).view(U)


def same_words(got, want):
    '''the rule `words`: -> bool array, True where the two agree'''
    g, w = _u(got), _u(want)
    return (g == w) | (np.isnan(g.view(F)) & np.isnan(w.view(F)))


def same_boxes(got, want):
    '''the rule `boxes`'''
    g, w = _u(got).view(F), _u(want).view(F)
    return same_words(g, w) | ((g == 0) & (w == 0))


def _fail(prop, bad, what, got, want, names):
    '''raise for the first True of `bad`; names: one label per axis of bad ('node', 'child', 'axis', 'slot', 'row', 'word')'''
    at = tuple(int(i) for i in np.argwhere(bad)[0])
    where = ' '.join(f'{k} {AXES[i] if k == "axis" else i}' for k, i in zip(names, at))
    g = np.broadcast_to(got, bad.shape)[at]
    w = np.broadcast_to(want, bad.shape)[at]
    raise AssertionError(f'{prop}: {where}: {what}: {_hex(g)} != {_hex(w)}  ({int(bad.sum())} such)')


class Binary:
    '''fnode taken apart once: ids [node][child], lo / hi [node][axis][child] (f32)'''

    def __init__(self, fnode, n):
        self.n = n = int(n)
        self.ni = ni = max(n - 1, 0)
        r = _u(fnode).reshape(-1, 4, 4)
        assert r.shape[0] == ni, f'{r.shape[0]} fnode records for {n} faces'
        self.ids = np.ascontiguousarray(r[:, 3, 0:2]).view(np.int32).astype(np.int64)
        self.lo = np.ascontiguousarray(r[:, 0:3, 0:2]).view(F)
        self.hi = np.ascontiguousarray(r[:, 0:3, 2:4]).view(F)
        self.inner = self.ids >= 0
        self.slot = np.where(self.inner, 0, ~self.ids)


def positions(verts):
    '''[3n][8] vertices -> [n][3][3] positions'''
    return np.ascontiguousarray(np.asarray(verts, F).reshape(-1, 3, 8)[:, :, :3])


# ---------------------------------------------------------------- binary nodes
def check_b1(b):
    n, ni, ids = b.n, b.ni, b.ids
    if ni == 0:
        return
    bad = (ids < -n) | (ids > ni - 1)
    if bad.any():
        _fail('B1', bad, f'id out of range for {n} faces', ids, np.where(ids < 0, -n, ni - 1), ('node', 'child'))
    parents = np.bincount(ids[b.inner], minlength=ni)
    if parents[0] != 0:
        _fail('B1', (ids == 0), 'node 0 is named as a child', ids, -1, ('node', 'child'))
    bad = parents[1:] != 1
    if bad.any():
        k = int(np.flatnonzero(bad)[0]) + 1
        raise AssertionError(f'B1: node {k}: has {int(parents[k])} parents, not 1  ({int(bad.sum())} such)')
    seen = np.bincount(b.slot[~b.inner], minlength=n)
    bad = seen != 1
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        at = np.argwhere(~b.inner & (b.slot == k))
        raise AssertionError(f'B1: slot {k}: appears {int(seen[k])} times, not once; in (node, child) {at.tolist()}  ({int(bad.sum())} such)')
    # (n - 1 records with 2n - 2 children, n of them the slots once each, n - 2 the nodes 1 .. n-2 once each: one tree if connected)
    reach = _order(b)
    assert reach.size == ni, f'B1: {ni - reach.size} nodes cannot be reached from node 0: a cycle apart from the tree'


def _order(b):
    '''the nodes reachable from node 0, parents before children'''
    out = [np.zeros(1, np.int64)] if b.ni else []
    seen = 1
    while out and out[-1].size and seen <= b.ni:
        level = out[-1]
        nxt = b.ids[level][b.inner[level]]
        out.append(nxt)
        seen += nxt.size
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def leaf_boxes(pos, leaf):
    '''[slot][axis] lo and hi of the triangle in every leaf slot: f32 min / max of its three vertices'''
    p = np.asarray(pos, F).reshape(-1, 3, 3)[np.asarray(leaf).astype(np.int64)]
    return p.min(axis=1), p.max(axis=1)


def check_b2(b, pos, leaf):
    if b.ni == 0:
        return
    llo, lhi = leaf_boxes(pos, leaf)
    want_lo = np.moveaxis(llo[b.slot], 2, 1)                 # [node][axis][child]
    want_hi = np.moveaxis(lhi[b.slot], 2, 1)
    isleaf = ~b.inner[:, None, :]
    for got, want, side in ((b.lo, want_lo, 'lo'), (b.hi, want_hi, 'hi')):
        bad = isleaf & ~same_boxes(got, want)
        if bad.any():
            at = np.argwhere(bad)[0]
            slot = int(b.slot[at[0], at[2]])
            _fail('B2', bad, f'{side} of leaf slot {slot} (face {int(np.asarray(leaf)[slot])}) is not its triangle\'s', got, want,
                  ('node', 'axis', 'child'))


def check_b3(b):
    if b.ni == 0:
        return
    k = np.where(b.inner, b.ids, 0)                          # the record an internal child names
    want_lo = np.moveaxis(np.minimum(b.lo[:, :, 0], b.lo[:, :, 1])[k], 2, 1)
    want_hi = np.moveaxis(np.maximum(b.hi[:, :, 0], b.hi[:, :, 1])[k], 2, 1)
    isin = b.inner[:, None, :]
    for got, want, side in ((b.lo, want_lo, 'lo'), (b.hi, want_hi, 'hi')):
        bad = isin & ~same_boxes(got, want)
        if bad.any():
            at = np.argwhere(bad)[0]
            _fail('B3', bad, f'{side} is not the union of the two boxes in node {int(b.ids[at[0], at[2]])}', got, want, ('node', 'axis', 'child'))


def leaves_under(b):
    '''[node][child]: the leaves below each child (needs B1)'''
    cnt = np.ones((b.ni, 2), np.int64)
    for i in _order(b)[::-1]:
        for k in range(2):
            if b.inner[i, k]:
                cnt[i, k] = cnt[b.ids[i, k]].sum()
    return cnt


def check_b4_preorder(b):
    if b.ni == 0:
        return
    cnt = leaves_under(b)
    me = np.arange(b.ni)[:, None]
    want = np.stack([me[:, 0] + 1, me[:, 0] + cnt[:, 0]], axis=1)
    bad = b.inner & (b.ids != want)
    if bad.any():
        _fail('B4', bad, 'not the DFS pre-order number (left: me + 1, right: me + leaves under the left child)', b.ids, want, ('node', 'child'))


def check_b4_lbvh(b, tree):
    '''tree: the reference arrays (child, bmin, bmax) of BVHTree().to_numpy()'''
    if b.ni == 0:
        return
    n = b.n
    ch = np.asarray(tree['child']).astype(np.int64).reshape(-1, 2)
    want = np.where(ch < n, ~ch, ch - n)
    bad = b.ids != want
    if bad.any():
        _fail('B4', bad, 'the id is not the reference tree\'s child, translated', b.ids, want, ('node', 'child'))
    k = np.where(b.inner, b.ids, 0)
    for got, own, side in ((b.lo, tree['bmin'], 'lo'), (b.hi, tree['bmax'], 'hi')):
        want = np.moveaxis(np.asarray(own, F).reshape(-1, 3)[k], 2, 1)
        bad = b.inner[:, None, :] & ~same_boxes(got, want)
        if bad.any():
            _fail('B4', bad, f'{side} is not the reference tree\'s b{"min" if side == "lo" else "max"} of the node it names', got, want,
                  ('node', 'axis', 'child'))


def levels(ids):
    '''levels of internal nodes below (and with) node 0, the root's level being 1; ids [node][2], id >= 0 internal'''
    ids = np.asarray(ids).astype(np.int64).reshape(-1, 2)
    if ids.shape[0] == 0:
        return 0
    level, depth = np.zeros(1, np.int64), 0
    while level.size:
        depth += 1
        assert depth <= ids.shape[0], 'B5: the ids hold a cycle'
        nxt = ids[level]
        level = nxt[nxt >= 0]
    return depth


def check_b5(ids, option, what='fast_depth'):
    got = levels(ids)
    assert got == int(option), f'B5: the records have {got} levels, option {what} says {int(option)}'


def snode_ids(snode, n):
    '''snode's children in fnode's convention'''
    ch = np.ascontiguousarray(_u(snode).reshape(-1, 2, 4)[:, :, 3]).view(np.int32).astype(np.int64)
    return np.where(ch < n, ~ch, ch - n)


def area(lo, hi):
    '''tree_rules.h wb_area in f32: lo, hi [...][3]'''
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(all='ignore'):
        d = np.fmax(hi - lo, F(0))
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        t = dx * dy
        t = t + dy * dz
        t = t + dz * dx
    assert t.dtype == np.float32
    return t


def cost(fnode, n):
    '''B6: the integer rf_cost_kernel sums over the records'''
    b = Binary(fnode, n)
    if b.ni == 0:
        return 0
    root_lo = np.fmin(b.lo[0, :, 0], b.lo[0, :, 1])
    root_hi = np.fmax(b.hi[0, :, 0], b.hi[0, :, 1])
    ra = float(area(root_lo, root_hi))
    if not ra > 0.0:
        return 0
    a = area(np.moveaxis(b.lo, 1, 2), np.moveaxis(b.hi, 1, 2)).astype(np.float64)       # [node][child]
    with np.errstate(all='ignore'):
        r = np.fmin(np.fmax(a / ra, 0.0), 1.0)
    shares = np.trunc(r * 1099511627776.0)
    return sum(int(s) for s in shares.reshape(-1))


def check_b6(fnode, n, reported, what='cost'):
    '''reported: the figure of refit_stats(), the integer over 2^40 as a double'''
    want = cost(fnode, n)
    assert want < 2 ** 53, f'B6: the sum {want} is not exact in a double'
    got = float(reported) * 1099511627776.0
    assert got == float(int(got)) and int(got) == want, f'B6: {what} is {got!r} / 2^40, the records give {want} / 2^40 (off by {got - want!r})'


def check_n1(snode, tree, n):
    ni = max(int(n) - 1, 0)
    s = _u(snode).reshape(-1, 2, 4)
    assert s.shape[0] == ni, f'N1: {s.shape[0]} snode records for {n} faces'
    if ni == 0:
        return
    want = np.zeros((ni, 2, 4), U)
    want[:, 0, 0:3] = _u(np.asarray(tree['bmin'], F).reshape(ni, 3))
    want[:, 1, 0:3] = _u(np.asarray(tree['bmax'], F).reshape(ni, 3))
    want[:, :, 3] = np.asarray(tree['child']).astype(np.int32).reshape(ni, 2).view(U)
    bad = ~same_words(s, want)
    if bad.any():
        _fail('N1', bad, 'snode is not the reference tree\'s array', s, want, ('node', 'row', 'word'))


def check_binary(pos, leaf, fnode, n, sah, tree=None, fast_depth=None):
    '''B1 - B5 over fnode.  sah: True for the SAH tree (pre-order), False for the LBVH (tree: the reference arrays)'''
    b = Binary(fnode, n)
    check_b1(b)
    check_b2(b, pos, leaf)
    check_b3(b)
    if sah:
        check_b4_preorder(b)
    else:
        check_b4_lbvh(b, tree)
    if fast_depth is not None:
        check_b5(b.ids, fast_depth, 'fast_depth')
    return b


# ---------------------------------------------------------------- triangle records
def make_tgeo(p0, p1, p2):
    '''tri_records.h tri_make_tgeo over [m][3] f32 positions -> [m][4][4] f32'''
    p0, p1, p2 = (np.asarray(p, F) for p in (p0, p1, p2))
    with np.errstate(all='ignore'):
        u = p1 - p0
        v = p2 - p0
        nn = np.zeros_like(u)
        for a, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
            s = u[:, i] * v[:, j]
            t = u[:, j] * v[:, i]
            nn[:, a] = s - t

        def dot(x, y):
            d = x[:, 0] * y[:, 0]
            t = x[:, 1] * y[:, 1]
            d = d + t
            t = x[:, 2] * y[:, 2]
            return d + t
        uu, uv, vv = dot(u, u), dot(u, v), dot(v, v)
        s = uv * uv
        t = uu * vv
        D = s - t
    g = np.zeros((p0.shape[0], 4, 4), F)
    for row, (vec, w) in enumerate(((p0, D), (u, uu), (v, uv), (nn, vv))):
        g[:, row, 0:3] = vec
        g[:, row, 3] = w
    return g


def make_tfast(g):
    '''tri_records.h tri_make_tfast over tgeo [m][4][4] f32 -> [m][3][4] f32'''
    g = np.asarray(g, F)
    D, uu, uv, vv = (g[:, r, 3][:, None] for r in range(4))
    u, v = g[:, 1, 0:3], g[:, 2, 0:3]
    with np.errstate(all='ignore'):
        s = uv * v
        t = vv * u
        a = (s - t) / D
        s = uv * u
        t = uu * v
        c = (s - t) / D
    f = np.zeros((g.shape[0], 3, 4), F)
    f[:, 0, 0:3], f[:, 1, 0:3], f[:, 2, 0:3] = g[:, 3, 0:3], a, c
    f[:, :, 3] = g[:, 0, 0:3]
    assert a.dtype == np.float32
    return f


def make_tshade(verts, mtlids):
    '''tri_records.h tri_make_tshade over [m][3][8] vertices (pos3 nrm3 uv2) and [m] material ids -> [m][4][4] uint32'''
    v = _u(np.asarray(verts, F).reshape(-1, 3, 8))
    s = np.zeros((v.shape[0], 16), U)
    s[:, 0:9] = v[:, :, 3:6].reshape(-1, 9)
    s[:, 9:15] = v[:, :, 6:8].reshape(-1, 6)
    s[:, 15] = np.asarray(mtlids).astype(np.int32).view(U)
    return s.reshape(-1, 4, 4)


def triangle_records(verts, mtlids, leaf):
    '''the three arrays as uint32, in leaf-slot order, tfast with its record n'''
    leaf = np.asarray(leaf).astype(np.int64).reshape(-1)
    v = np.asarray(verts, F).reshape(-1, 3, 8)[leaf]
    g = make_tgeo(v[:, 0, 0:3], v[:, 1, 0:3], v[:, 2, 0:3])
    f = np.concatenate([_u(make_tfast(g)), np.full((1, 3, 4), ONES, U)])
    return dict(tgeo=_u(g), tfast=f, tshade=make_tshade(v, np.asarray(mtlids).reshape(-1)[leaf]))


def _check_rows(prop, name, got, want, leaf):
    got = _u(got)
    assert got.shape == want.shape, f'{prop}: {name} has shape {got.shape}, not {want.shape}'
    bad = ~same_words(got, want)
    if bad.any():
        slot = int(np.argwhere(bad)[0][0])
        face = int(np.asarray(leaf)[slot]) if slot < len(leaf) else -1
        _fail(prop, bad, f'{name} of face {face}', got, want, ('slot', 'row', 'word'))


def check_t1(tgeo, want, leaf):
    _check_rows('T1', 'tgeo', tgeo, want['tgeo'], leaf)


def check_t2(tfast, want, leaf):
    tfast = _u(tfast)
    n = want['tfast'].shape[0] - 1
    assert tfast.shape == (n + 1, 3, 4), f'T2: tfast has shape {tfast.shape}, not {(n + 1, 3, 4)}'
    bad = tfast[n:] != ONES                                  # (both sides NaN would not do here: the words are specified)
    if bad.any():
        _fail('T2', bad, f'the sentinel record {n} is not all ones', tfast[n:], U(ONES), ('sentinel', 'row', 'word'))
    _check_rows('T2', 'tfast', tfast[:n], want['tfast'][:n], leaf)


def check_t3(tshade, want, leaf):
    _check_rows('T3', 'tshade', tshade, want['tshade'], leaf)


def check_triangles(verts, mtlids, leaf, rec):
    want = triangle_records(verts, mtlids, leaf)
    check_t1(rec['tgeo'], want, leaf)
    check_t2(rec['tfast'], want, leaf)
    check_t3(rec['tshade'], want, leaf)


# ---------------------------------------------------------------- everything
def check_all(verts, mtlids, rec, tree, n, sah, fast_depth=None):
    '''rec: BVHTree().records(); tree: BVHTree().to_numpy() (leaf order, the reference arrays, depth).  -> Binary(fnode)'''
    n = int(n)
    leaf = np.asarray(tree['leaf']).astype(np.int64).reshape(-1)[:n]
    assert np.array_equal(np.sort(leaf), np.arange(n)), 'the leaf order is no permutation of the faces'
    pos = positions(verts)
    b = check_binary(pos, leaf, rec['fnode'], n, sah, tree, fast_depth)
    check_n1(rec['snode'], tree, n)
    check_b5(snode_ids(rec['snode'], n), tree['depth'], 'tree_depth')
    check_triangles(verts, mtlids, leaf, rec)
    return b

'''
An independent checker for the trees the renderer walks: plain numpy over downloaded records and the model's
vertices, nothing imported from the package under test.

What is checked, and against what
---------------------------------
The 4-wide collapse is two parallel arrays of records, node w at index w, the root at 0, children after their parents:

  wnode [nw][8][4] uint32   rows {lo.x[4]} {hi.x[4]} {lo.y[4]} {hi.y[4]} {lo.z[4]} {hi.z[4]} {id[4]} {-}: exact f32 boxes
  qnode [nw][4][4] uint32   rows {origin.xyz, scale.x} {scale.y, scale.z, qlo.x, qhi.x} {qlo.y, qhi.y, qlo.z, qhi.z} {id[4]},
                            one byte per child in each q word (child k in bits 8k .. 8k+7)

A child id >= 1 names a wide node, an id < 0 names leaf slot ~id, `leaf[slot]` is the face of the model; an unused slot
holds ~n.  The root is nobody's child, so id 0 never marks a used slot: E3 reports it, every other property treats such a
slot as unused.

Exact records (f32 values compared with ==, no tolerance: min and max do not round; -0.0 == +0.0)
  E1  a leaf child's box is the f32 min / max of its triangle's three vertices
  E2  an internal child's box is the union of the used child boxes of the node it names.  E1 and E2 together give, by
      induction from the leaves, that every box encloses every triangle below it -- and that none is larger than that
  E3  an unused slot: id ~n and lo = hi = 1e30f on every axis; no slot names id 0
  E4  topology: ids in range; every node but the root has exactly one parent; every triangle sits in exactly one slot;
      a used slot's box is finite with lo <= hi; an internal child's id is greater than its parent's number

Quantised records, decoded in f64 as plane = origin + q * scale.  ulp(x) is the f32 spacing at |x|, `node lo / hi` the
union of the used children's exact boxes, e = node hi - origin (f64), M = max(|origin|, |node hi|) on the axis.
  Q1  the id row is wnode's id row
  Q2  origin[a] is the f32 min of the used children's lo[a]
  Q3  scale[a] is finite and positive.  A flat axis (e == 0): scale == max(|origin| * 1e-6f, 1e-30f) in f32.  Otherwise
        lower bound, in f32:  float32(origin + float32(255) * scale) >= node hi
        upper bound, in f64:  255 * scale <= e + ulp(e) / 2 + 255 * ulp(scale)
      The builder starts from s0 = fl(fl(node hi - origin) / 255) and raises the step one ulp at a time until the lower
      bound holds.  If s0 holds at once: fl(hi - origin) <= e + ulp(e) / 2 and the quotient adds at most ulp(scale) / 2,
      so 255 * scale <= e + ulp(e) / 2 + 255 * ulp(scale) / 2.  Otherwise the step before, p = scale - ulp, failed:
      fl(origin + fl(255 p)) < hi, and because rounding is monotone and hi is an f32 value the unrounded sum is below
      hi too, so fl(255 p) < e, so 255 p < e + ulp(e) / 2 (the product lies below e, its rounding error is at most
      half the spacing there); one more ulp of the step adds 255 * ulp(scale).
      (The bound first written for this check, e + ulp(M), charged the rounding of the SUM, which the argument above
      shows costs nothing on this side, and left out what the step's own granularity costs: 255 * ulp(scale) is
      between one and two ulp(e), so near the origin, where ulp(e) ~ ulp(M), a right builder exceeds it.)
  Q4  outward rounding, for every used child:
        qlo == 0   : origin <= lo                                  (exact, f32)
        qlo  > 0   : origin + qlo * scale <= lo - 0.24 * scale
        qhi  < 255 : origin + qhi * scale >= hi + 0.24 * scale
        qhi == 255 : origin + 255 * scale >= hi - ulp(M) / 2 - ulp(255 * scale) / 2
      Why 0.24: the builder pads by 0.25 of a step, q = floor(x - 0.25) resp. ceil(x + 0.25) with x the f32 quotient
      (lo - origin) / scale.  The difference and the quotient carry a relative error of 2^-24 each, on a value of at most
      255: 255 * 2^-23 steps; subtracting 0.25f rounds once more, by at most ulp(255) / 2 = 2^-17.  Together below
      4e-5 steps, so a right builder's planes lie at least 0.2499 steps outside and 0.24 leaves room for that and
      nothing more.
      Why the two terms at qhi == 255: Q3's lower bound is a statement about ROUNDED f32 arithmetic; the f64 plane may
      fall short of hi by what those two roundings hide -- ulp(M) / 2 for the sum (the sum is at most M in magnitude)
      and half the spacing of the f32 product 255 * scale.  (The product's term was missing from the bound first written
      for this check; it matters wherever e is of the size of M.)
  Q5  not loose: a low plane with qlo > 0 lies within 1.26 * scale of lo, a high plane with qhi < 255 within
      1.26 * scale of hi, because floor(x - 0.25) > x - 1.25 (and ceil(x + 0.25) < x + 1.25), plus the 4e-5 above
  Q6  an unused slot: qlo byte 255 and qhi byte 0 on all three axes

Stack and depth
  S1  stack_need(ids, n): the LDS stack levels a traversal can ask for.  A step at a node with k used children leaves
      k - 1 entries behind and goes on with one child: need(w) = k - 1 + max need over w's internal children; the answer
      is 1 + need(root) + 1 (the sentinel below, the level the step's last plain store lands on above).
      levels(ids): the number of levels of the wide tree, the root's being 1.

Reference LBVH (the arrays of BVHTree().to_numpy(): child [n-1][2], leaf [n], bmin / bmax [n-1][3], mc [n], depth; a child
id < n is leaf slot id, an id >= n internal node id - n, node 0 is the root)
  L1  leaf is a permutation of 0 .. n-1
  L2  mc is non-decreasing
  L3  child forms one tree over n leaves and n - 1 internal nodes
  L4  every internal node's bmin / bmax is the union of its subtree's triangle bounds (== on f32 values)
  L5  depth is the number of levels of internal nodes, the root's being 1

Every check raises AssertionError with a message that starts with the property's name and names the node, the child
slot, the axis and the two values that disagree.
'''

import numpy as np

F = np.float32
AXES = 'xyz'
EMPTY = F(1e30)

EXACT = ('E1', 'E2', 'E3', 'E4')
QUANT = ('Q1', 'Q2', 'Q3', 'Q4', 'Q5', 'Q6')
LBVH = ('L1', 'L2', 'L3', 'L4', 'L5')


def ulp(x):
    '''the f32 spacing at |x|'''
    return np.spacing(np.abs(np.asarray(x)).astype(F))


def _val(x):
    x = np.asarray(x)
    if x.dtype == np.float32:
        return f'{float(x)!r} (0x{int(x.view(np.uint32)):08x})'
    if x.dtype.kind == 'f':
        return f'{float(x)!r}'
    return f'{int(x)}'


def _fail(prop, bad, what, got, want, rel='!='):
    '''raise for the first True of `bad`, whose axes are (node, axis, slot), (node, slot) or (node, axis) like got / want'''
    at = tuple(np.argwhere(bad)[0])
    where = f'node {at[0]}'
    if bad.ndim == 3:
        where += f' child {at[2]} axis {AXES[at[1]]}'
    elif bad.shape[1] == 4:
        where += f' child {at[1]}'
    else:
        where += f' axis {AXES[at[1]]}'
    g = np.broadcast_to(got, bad.shape)[at]
    w = np.broadcast_to(want, bad.shape)[at]
    raise AssertionError(f'{prop}: {where}: {what}: {_val(g)} {rel} {_val(w)}  ({int(bad.sum())} such)')


class Tree:
    '''the records, taken apart once'''

    def __init__(self, pos, leaf, wnode, qnode, n):
        n = int(n)
        self.n = n
        self.pos = np.ascontiguousarray(pos, F).reshape(n, 3, 3)
        self.leaf = np.asarray(leaf).astype(np.int64).reshape(-1)
        w = np.ascontiguousarray(wnode).view(np.uint32).reshape(-1, 8, 4)
        q = np.ascontiguousarray(qnode).view(np.uint32).reshape(-1, 4, 4)
        assert w.shape[0] == q.shape[0] and w.shape[0] > 0, f'{w.shape[0]} exact records, {q.shape[0]} quantised ones'
        self.nw = nw = w.shape[0]
        self.ids = np.ascontiguousarray(w[:, 6, :]).view(np.int32)                       # [node][slot]
        self.lo = np.ascontiguousarray(w[:, 0:6:2, :]).view(F)                           # [node][axis][slot]
        self.hi = np.ascontiguousarray(w[:, 1:6:2, :]).view(F)
        self.empty = self.ids == ~n
        self.used = ~self.empty & (self.ids != 0)
        self.inner = self.used & (self.ids > 0) & (self.ids < nw)
        self.leafc = self.used & (self.ids < 0) & (self.ids > ~n)
        u = self.used[:, None, :]
        self.node_lo = np.where(u, self.lo, F(np.inf)).min(axis=2)                       # [node][axis]
        self.node_hi = np.where(u, self.hi, F(-np.inf)).max(axis=2)
        self.qids = np.ascontiguousarray(q[:, 3, :]).view(np.int32)
        self.origin = np.ascontiguousarray(q[:, 0, 0:3]).view(F)                         # [node][axis]
        self.scale = np.stack([q[:, 0, 3], q[:, 1, 0], q[:, 1, 1]], axis=1).view(F)
        wl = np.stack([q[:, 1, 2], q[:, 2, 0], q[:, 2, 2]], axis=1)
        wh = np.stack([q[:, 1, 3], q[:, 2, 1], q[:, 2, 3]], axis=1)
        sh = (8 * np.arange(4, dtype=np.uint32))[None, None, :]
        self.qlo = ((wl[:, :, None] >> sh) & 255).astype(np.int64)                       # [node][axis][slot]
        self.qhi = ((wh[:, :, None] >> sh) & 255).astype(np.int64)


# ---------------------------------------------------------------------------------------------- exact records

def check_E1(t):
    at = np.argwhere(t.leafc)
    if not len(at):
        return
    w, k = at[:, 0], at[:, 1]
    slot = ~t.ids[w, k].astype(np.int64)
    ok = slot < len(t.leaf)
    face = np.where(ok, t.leaf[np.minimum(slot, len(t.leaf) - 1)], 0)
    ok &= (face >= 0) & (face < t.n)
    face = np.where(ok, face, 0)
    for name, rec, tri in (('lo', t.lo, t.pos.min(axis=1)), ('hi', t.hi, t.pos.max(axis=1))):
        want = np.zeros_like(rec)
        bad = np.zeros(rec.shape, bool)
        want[w, :, k] = tri[face]
        bad[w, :, k] = (rec[w, :, k] != tri[face]) | ~ok[:, None]
        if bad.any():
            _fail('E1', bad, f'leaf child\'s {name} is not its triangle\'s', rec, want)


def check_E2(t):
    at = np.argwhere(t.inner & (t.ids >= 1))
    if not len(at):
        return
    w, k = at[:, 0], at[:, 1]
    c = t.ids[w, k]
    for name, rec, node in (('lo', t.lo, t.node_lo), ('hi', t.hi, t.node_hi)):
        want = np.zeros_like(rec)
        bad = np.zeros(rec.shape, bool)
        want[w, :, k] = node[c]
        bad[w, :, k] = rec[w, :, k] != node[c]
        if bad.any():
            _fail('E2', bad, f'internal child\'s {name} is not the union of the boxes of the node it names', rec, want)


def check_E3(t):
    if (t.ids == 0).any():
        _fail('E3', t.ids == 0, 'a slot names the root', t.ids, np.int32(~t.n))
    e = np.broadcast_to(t.empty[:, None, :], t.lo.shape)
    for name, rec in (('lo', t.lo), ('hi', t.hi)):
        bad = e & (rec != EMPTY)
        if bad.any():
            _fail('E3', bad, f'unused slot\'s {name} is not 1e30f', rec, EMPTY)


def check_E4(t):
    n, nw, ids = t.n, t.nw, t.ids
    bad = (ids >= nw) | (ids < ~n)
    if bad.any():
        _fail('E4', bad, f'id out of range [{~n}, {nw})', ids, np.int32(nw), rel='outside, limit')
    parents = np.bincount(ids[ids > 0], minlength=nw)[:nw]
    wrong = np.flatnonzero(parents[1:] != 1) + 1
    if len(wrong):
        who = np.argwhere(ids == wrong[0])
        raise AssertionError(f'E4: node {wrong[0]} has {parents[wrong[0]]} parents, not 1 (named by node / child '
                             f'{[tuple(int(x) for x in r) for r in who[:4]]}); {len(wrong)} such nodes')
    slots = ~ids[(ids < 0) & (ids != ~n)].astype(np.int64)
    named = np.bincount(slots, minlength=n)
    wrong = np.flatnonzero(named != 1)
    if len(wrong):
        who = np.argwhere(ids == ~int(wrong[0]))
        raise AssertionError(f'E4: triangle slot {wrong[0]} sits in {named[wrong[0]]} slots, not 1 (node / child '
                             f'{[tuple(int(x) for x in r) for r in who[:4]]}); {len(wrong)} such triangles')
    u = np.broadcast_to(t.used[:, None, :], t.lo.shape)
    for name, rec in (('lo', t.lo), ('hi', t.hi)):
        bad = u & ~np.isfinite(rec)
        if bad.any():
            _fail('E4', bad, f'used slot\'s {name} is not finite', rec, F(0), rel='not finite, e.g. not')
    bad = u & ~(t.lo <= t.hi)
    if bad.any():
        _fail('E4', bad, 'used slot\'s lo > hi', t.lo, t.hi, rel='>')
    own = np.arange(nw, dtype=np.int64)[:, None]
    bad = (ids > 0) & (ids <= own)
    if bad.any():
        _fail('E4', bad, 'internal child does not come after its parent', ids, np.broadcast_to(own, ids.shape), rel='<= own number')


# ---------------------------------------------------------------------------------------------- quantised records

def check_Q1(t):
    bad = t.qids != t.ids
    if bad.any():
        _fail('Q1', bad, 'quantised record\'s id is not the exact record\'s', t.qids, t.ids)


def check_Q2(t):
    bad = t.origin != t.node_lo
    if bad.any():
        _fail('Q2', bad, 'origin is not the min of the used children\'s lo', t.origin, t.node_lo)


def check_Q3(t):
    o, s, hi = t.origin, t.scale, t.node_hi
    bad = ~(np.isfinite(s) & (s > 0))
    if bad.any():
        _fail('Q3', bad, 'scale is not finite and positive', s, F(0), rel='not >')
    e = hi.astype(np.float64) - o.astype(np.float64)
    flat = e == 0
    with np.errstate(over='ignore', invalid='ignore'):
        want = np.maximum(np.abs(o) * F(1e-6), F(1e-30)).astype(F)
        bad = flat & (s != want)
        if bad.any():
            _fail('Q3', bad, 'flat axis: scale is not max(|origin| * 1e-6f, 1e-30f)', s, want)
        far = (o + F(255) * s).astype(F)                                              # f32 arithmetic, as the kernels' bound
        bad = ~flat & ~(far >= hi)
        if bad.any():
            _fail('Q3', bad, '255 steps do not reach the far side in f32', far, hi, rel='<')
        reach = 255.0 * s.astype(np.float64)
        limit = e + 0.5 * ulp(e).astype(np.float64) + 255.0 * ulp(s).astype(np.float64)
        bad = ~flat & ~(reach <= limit)
        if bad.any():
            _fail('Q3', bad, '255 * scale is larger than e + ulp(e) / 2 + 255 ulp(scale)', reach, limit, rel='>')


def _planes(t):
    o = t.origin.astype(np.float64)[:, :, None]
    s = t.scale.astype(np.float64)[:, :, None]
    u = np.broadcast_to(t.used[:, None, :], t.lo.shape)
    return o, s, u, o + t.qlo * s, o + t.qhi * s


def check_Q4(t):
    o, s, u, plo, phi = _planes(t)
    lo, hi = t.lo.astype(np.float64), t.hi.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        bad = u & (t.qlo == 0) & ~(t.origin[:, :, None] <= t.lo)
        if bad.any():
            _fail('Q4', bad, 'low plane at byte 0 lies inside the child: origin > lo', t.origin[:, :, None], t.lo, rel='>')
        limit = lo - 0.24 * s
        bad = u & (t.qlo > 0) & ~(plo <= limit)
        if bad.any():
            _fail('Q4', bad, 'low plane is not 0.24 steps outside: origin + qlo * scale > lo - 0.24 scale', plo, limit, rel='>')
        limit = hi + 0.24 * s
        bad = u & (t.qhi < 255) & ~(phi >= limit)
        if bad.any():
            _fail('Q4', bad, 'high plane is not 0.24 steps outside: origin + qhi * scale < hi + 0.24 scale', phi, limit, rel='<')
        m = np.maximum(np.abs(t.origin), np.abs(t.node_hi))
        slack = 0.5 * ulp(m).astype(np.float64) + 0.5 * ulp((F(255) * t.scale).astype(F)).astype(np.float64)
        limit = hi - slack[:, :, None]
        bad = u & (t.qhi == 255) & ~(phi >= limit)
        if bad.any():
            _fail('Q4', bad, 'high plane at byte 255 falls short: origin + 255 scale < hi - ulp(M) / 2 - ulp(255 scale) / 2', phi, limit, rel='<')


def check_Q5(t):
    o, s, u, plo, phi = _planes(t)
    lo, hi = t.lo.astype(np.float64), t.hi.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        limit = lo - 1.26 * s
        bad = u & (t.qlo > 0) & ~(plo >= limit)
        if bad.any():
            _fail('Q5', bad, 'low plane is loose: origin + qlo * scale < lo - 1.26 scale', plo, limit, rel='<')
        limit = hi + 1.26 * s
        bad = u & (t.qhi < 255) & ~(phi <= limit)
        if bad.any():
            _fail('Q5', bad, 'high plane is loose: origin + qhi * scale > hi + 1.26 scale', phi, limit, rel='>')


def check_Q6(t):
    e = np.broadcast_to(t.empty[:, None, :], t.qlo.shape)
    bad = e & (t.qlo != 255)
    if bad.any():
        _fail('Q6', bad, 'unused slot\'s qlo byte is not 255', t.qlo, np.int64(255))
    bad = e & (t.qhi != 0)
    if bad.any():
        _fail('Q6', bad, 'unused slot\'s qhi byte is not 0', t.qhi, np.int64(0))


def q_margins(t):
    '''for the record, not a bound: the smallest outward margin of a plane that is not clamped (Q4 asks for 0.24) and the
    largest distance of such a plane from its child (Q5 allows 1.26), both in steps of the node's scale'''
    o, s, u, plo, phi = _planes(t)
    lo, hi = t.lo.astype(np.float64), t.hi.astype(np.float64)
    with np.errstate(all='ignore'):
        d = np.concatenate([((lo - plo) / s)[u & (t.qlo > 0)], ((phi - hi) / s)[u & (t.qhi < 255)]])
    if not len(d):
        return dict(q4_min_steps=None, q5_max_steps=None)
    return dict(q4_min_steps=float(d.min()), q5_max_steps=float(d.max()))


# ---------------------------------------------------------------------------------------------- stack and depth

def _wide_levels(ids, n):
    '''level of every wide node reached from the root (root 1, not reached 0), by generations'''
    ids = np.asarray(ids).view(np.int32).reshape(-1, 4)
    nw = ids.shape[0]
    level = np.zeros(nw, np.int64)
    front = np.zeros(1, np.int64)
    d = 0
    while len(front):
        d += 1
        assert d <= nw, 'S1: the id vectors do not form a tree (a cycle)'
        assert not level[front].any(), 'S1: the id vectors do not form a tree (a node reached twice)'
        level[front] = d
        ch = ids[front]
        front = np.unique(ch[(ch > 0) & (ch < nw)].astype(np.int64))
    return level


def levels(ids, n=None):
    '''S1: the number of levels of the wide tree (the root's is 1)'''
    return int(_wide_levels(ids, n).max())


def stack_need(ids, n):
    '''S1: the stack levels a traversal of the wide tree can ask for, 1 + need(root) + 1'''
    ids = np.asarray(ids).view(np.int32).reshape(-1, 4)
    nw = ids.shape[0]
    level = _wide_levels(ids, n)
    k = (ids != ~int(n)).sum(axis=1)
    inner = (ids > 0) & (ids < nw)
    need = np.zeros(nw, np.int64)
    for d in range(int(level.max()), 0, -1):
        at = np.flatnonzero(level == d)
        c = ids[at]
        deep = np.where(inner[at], need[np.clip(c, 0, nw - 1)], 0).max(axis=1)
        need[at] = np.maximum(k[at] - 1, 0) + deep
    return int(1 + need[0] + 1)


# ---------------------------------------------------------------------------------------------- reference LBVH

def _lbvh_levels(child, n):
    '''L3: level of every internal node (root 1); raises unless child is one tree over n leaves and n - 1 internal nodes'''
    child = np.asarray(child).astype(np.int64).reshape(-1, 2)
    assert child.shape[0] == n - 1, f'L3: {child.shape[0]} internal nodes for {n} leaves, not {n - 1}'
    bad = (child < 0) | (child >= 2 * n - 1)
    assert not bad.any(), f'L3: node {np.argwhere(bad)[0][0]} child {np.argwhere(bad)[0][1]}: id {child[bad][0]} outside [0, {2 * n - 1})'
    seen = np.bincount(child.reshape(-1), minlength=2 * n - 1)
    assert seen[n] == 0, f'L3: the root is named as a child {seen[n]} times'
    wrong = np.flatnonzero(np.delete(seen, n) != 1)
    if len(wrong):
        x = int(wrong[0]) + (wrong[0] >= n)
        what = f'leaf slot {x}' if x < n else f'internal node {x - n}'
        raise AssertionError(f'L3: {what} has {seen[x]} parents, not 1; {len(wrong)} such')
    level = np.zeros(n - 1, np.int64)
    front = np.zeros(1, np.int64)
    d = 0
    while len(front):
        d += 1
        level[front] = d
        c = child[front].reshape(-1)
        front = c[c >= n] - n
    assert level.all(), f'L3: internal node {np.flatnonzero(level == 0)[0]} is not reached from the root'
    return level


def check_L1(pos, tree, n):
    leaf = np.asarray(tree['leaf']).astype(np.int64)
    assert len(leaf) == n, f'L1: {len(leaf)} leaf slots for {n} triangles'
    bad = (leaf < 0) | (leaf >= n)
    assert not bad.any(), f'L1: slot {np.flatnonzero(bad)[0]} names face {leaf[bad][0]}, outside [0, {n})'
    c = np.bincount(leaf, minlength=n)
    wrong = np.flatnonzero(c != 1)
    assert not len(wrong), f'L1: face {wrong[0]} sits in {c[wrong[0]]} leaf slots (slots {np.flatnonzero(leaf == wrong[0])[:4]}), not 1'


def check_L2(pos, tree, n):
    mc = np.asarray(tree['mc']).astype(np.int64)
    assert len(mc) == n, f'L2: {len(mc)} Morton codes for {n} triangles'
    down = np.flatnonzero(np.diff(mc) < 0)
    assert not len(down), f'L2: mc falls at slot {down[0]}: {mc[down[0]]} > {mc[down[0] + 1]}'


def check_L3(pos, tree, n):
    _lbvh_levels(tree['child'], n)


def check_L4(pos, tree, n):
    pos = np.ascontiguousarray(pos, F).reshape(n, 3, 3)
    child = np.asarray(tree['child']).astype(np.int64).reshape(-1, 2)
    leaf = np.asarray(tree['leaf']).astype(np.int64)
    level = _lbvh_levels(child, n)
    for name, stored, tri, join in (('bmin', tree['bmin'], pos.min(axis=1), np.minimum), ('bmax', tree['bmax'], pos.max(axis=1), np.maximum)):
        stored = np.asarray(stored, F).reshape(n - 1, 3)
        own = np.zeros((n - 1, 3), F)                       # the union of the subtree's triangle bounds, bottom up
        for d in range(int(level.max()), 0, -1):
            at = np.flatnonzero(level == d)
            side = []
            for k in (0, 1):
                c = child[at, k]
                isleaf = c < n
                side.append(np.where(isleaf[:, None], tri[leaf[np.where(isleaf, c, 0)] % n], own[np.where(isleaf, 0, c - n)]))
            own[at] = join(side[0], side[1])
        bad = stored != own
        if bad.any():
            i, a = np.argwhere(bad)[0]
            raise AssertionError(f'L4: internal node {i} axis {AXES[a]}: {name} {_val(stored[i, a])} != the union of its '
                                 f'subtree\'s triangle bounds {_val(own[i, a])}  ({int(bad.sum())} such)')


def check_L5(pos, tree, n):
    want = int(_lbvh_levels(tree['child'], n).max())
    assert int(tree['depth']) == want, f'L5: depth {int(tree["depth"])} != {want} levels of internal nodes in child'


# ---------------------------------------------------------------------------------------------- groups

_WIDE = dict(E1=check_E1, E2=check_E2, E3=check_E3, E4=check_E4,
             Q1=check_Q1, Q2=check_Q2, Q3=check_Q3, Q4=check_Q4, Q5=check_Q5, Q6=check_Q6)
_LBVH = dict(L1=check_L1, L2=check_L2, L3=check_L3, L4=check_L4, L5=check_L5)


def check_exact(pos, leaf, wnode, qnode, n):
    '''E1-E4.  Topology first: the other three read the tree through it'''
    t = Tree(pos, leaf, wnode, qnode, n)
    for p in ('E4', 'E3', 'E1', 'E2'):
        _WIDE[p](t)
    return t


def check_quantised(pos, leaf, wnode, qnode, n):
    '''Q1-Q6'''
    t = Tree(pos, leaf, wnode, qnode, n)
    for p in QUANT:
        _WIDE[p](t)
    return t


def check_all(pos, leaf, wnode, qnode, n):
    '''E1-E4, Q1-Q6, and that S1's two figures can be computed.  Returns the parsed Tree'''
    t = Tree(pos, leaf, wnode, qnode, n)
    for p in ('E4', 'E3', 'E1', 'E2') + QUANT:
        _WIDE[p](t)
    stack_need(t.ids, n)
    return t


def check_lbvh(pos, tree, n):
    '''L1-L5 on the arrays of BVHTree().to_numpy()'''
    for p in LBVH:
        _LBVH[p](pos, tree, n)


def failing(pos, leaf, wnode, qnode, n):
    '''the names of ALL the E and Q properties the records break, each checked on its own'''
    t = Tree(pos, leaf, wnode, qnode, n)
    out = []
    for p in EXACT + QUANT:
        try:
            _WIDE[p](t)
        except AssertionError as e:
            assert str(e).startswith(p + ':'), str(e)
            out.append(p)
    return out


def failing_lbvh(pos, tree, n):
    '''the names of all the L properties the arrays break (L4 and L5 read the tree through L3 and report L3 where it is broken)'''
    out = []
    for p in LBVH:
        try:
            _LBVH[p](pos, tree, n)
        except AssertionError as e:
            assert str(e)[:2] in LBVH, str(e)
            if str(e)[:2] not in out:
                out.append(str(e)[:2])
    return out

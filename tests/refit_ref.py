'''
What a refit must write, restated in numpy: nothing imported from the package under test.

A refit (BVHTree().refit(), csrc/refit.hip) keeps a built tree's topology -- the reference LBVH's `child` and `leaf`, the id
rows of the 4-wide records -- and recomputes every box from new vertex positions.  refit_ref takes that topology and the new
positions and returns the arrays a refit must leave, byte for byte:

  bmin, bmax  [n-1][3] f32   the LBVH's boxes (BVHTree().to_numpy()): bottom-up unions with np.minimum / np.maximum on f32
  wnode       [nw][8][4] u32 rows {lo.x[4]} {hi.x[4]} {lo.y[4]} {hi.y[4]} {lo.z[4]} {hi.z[4]} {id[4]} {-}: a leaf child's box is the
                             f32 min / max of its triangle's three vertices, an internal child's the union of the used child
                             boxes of the node it names; unused slots (id ~n) and rows 6, 7 are copied from the input
  qnode       [nw][4][4] u32 the 8-bit boxes, re-quantised from the new exact ones with the builder's f32 operations one by one
                             (wide_build.hip wb_expand / tree_rules.h wb_quantise): origin = min of the used children's lo;
                             e = hi - origin; step = e / 255, raised one ulp at a time until origin + 255 * step >= hi in f32,
                             or max(|origin| * 1e-6f, 1e-30f) on a flat axis; bytes floor((lo - origin) / step - 0.25f) and
                             ceil((hi - origin) / step + 0.25f) clamped to 0 .. 255; an unused slot 255 / 0; id row = wnode's

min and max do not round, so the unions do not depend on the order they are formed in; the clamps are fminf / fmaxf (np.fmin /
np.fmax: a NaN quotient clamps to a number, as on the device).
'''

import numpy as np

F = np.float32


def _levels(kids, root=0):
    '''kids [N][k] int64, -1 where a slot names no internal node -> level of every node (root 1), by generations'''
    level = np.zeros(kids.shape[0], np.int64)
    front = np.array([root], np.int64)
    d = 0
    while len(front):
        d += 1
        assert d <= kids.shape[0] and not level[front].any(), 'the ids do not form a tree'
        level[front] = d
        c = kids[front].reshape(-1)
        front = c[c >= 0]
    assert level.all(), 'a node is not reached from the root'
    return level


def _lbvh_boxes(child, leaf, n, tri_lo, tri_hi):
    child = np.asarray(child).astype(np.int64).reshape(n - 1, 2)
    level = _levels(np.where(child >= n, child - n, -1))
    out = []
    for tri, join in ((tri_lo, np.minimum), (tri_hi, np.maximum)):
        own = np.zeros((n - 1, 3), F)
        for d in range(int(level.max()), 0, -1):
            at = np.flatnonzero(level == d)
            side = []
            for k in (0, 1):
                c = child[at, k]
                isleaf = c < n
                side.append(np.where(isleaf[:, None], tri[leaf[np.where(isleaf, c, 0)]], own[np.where(isleaf, 0, c - n)]))
            own[at] = join(side[0], side[1])
        out.append(own)
    return out


def quantise(lo, hi, used, ids):
    '''lo, hi [N][3][4] f32 (axis, slot), used [N][4] bool, ids [N][4] int32 -> qnode [N][4][4] uint32'''
    N = lo.shape[0]
    u = used[:, None, :]
    with np.errstate(all='ignore'):
        plo = np.where(u, lo, F(np.inf)).min(axis=2).astype(F)                      # [N][3]
        phi = np.where(u, hi, F(-np.inf)).max(axis=2).astype(F)
        e = (phi - plo).astype(F)
        sc = np.where(e > 0, (e / F(255)).astype(F), F(0)).astype(F)
        while True:
            short = (e > 0) & ((plo + (F(255) * sc).astype(F)).astype(F) < phi)
            if not short.any():
                break
            sc = np.where(short, np.nextafter(sc, F(np.inf)), sc).astype(F)
        flat = np.maximum((np.abs(plo) * F(1e-6)).astype(F), F(1e-30)).astype(F)
        sc = np.where(sc > 0, sc, flat).astype(F)
        s, o = sc[:, :, None], plo[:, :, None]
        fl = np.floor((((lo - o).astype(F) / s).astype(F) - F(0.25)).astype(F))
        fh = np.ceil((((hi - o).astype(F) / s).astype(F) + F(0.25)).astype(F))
        ql = np.fmin(F(255), np.fmax(F(0), fl)).astype(np.uint32)
        qh = np.fmin(F(255), np.fmax(F(0), fh)).astype(np.uint32)
    ql = np.where(u, ql, np.uint32(255))
    qh = np.where(u, qh, np.uint32(0))
    sh = (8 * np.arange(4, dtype=np.uint32))[None, None, :]
    wl = (ql << sh).sum(axis=2, dtype=np.uint32)                                    # [N][3]: one word per axis
    wh = (qh << sh).sum(axis=2, dtype=np.uint32)
    q = np.zeros((N, 4, 4), np.uint32)
    pu, su = plo.view(np.uint32), sc.view(np.uint32)
    q[:, 0, 0:3] = pu
    q[:, 0, 3] = su[:, 0]
    q[:, 1, 0], q[:, 1, 1], q[:, 1, 2], q[:, 1, 3] = su[:, 1], su[:, 2], wl[:, 0], wh[:, 0]
    q[:, 2, 0], q[:, 2, 1], q[:, 2, 2], q[:, 2, 3] = wl[:, 1], wh[:, 1], wl[:, 2], wh[:, 2]
    q[:, 3, :] = ids.view(np.uint32)
    return q


def refit_ref(child, leaf, wnode, qnode, n, pos):
    '''(child [n-1][2], leaf [n], wnode [nw][8][4], qnode [nw][4][4], n, positions [n][3][3]) -> (bmin, bmax, wnode, qnode)'''
    n = int(n)
    pos = np.ascontiguousarray(pos, F).reshape(n, 3, 3)
    leaf = np.asarray(leaf).astype(np.int64).reshape(-1)
    tri_lo, tri_hi = pos.min(axis=1), pos.max(axis=1)                              # [face][axis]
    if n < 2:
        z = np.zeros((0, 3), F)
        return z, z.copy(), np.zeros((0, 8, 4), np.uint32), np.zeros((0, 4, 4), np.uint32)
    bmin, bmax = _lbvh_boxes(child, leaf, n, tri_lo, tri_hi)

    w = np.ascontiguousarray(wnode).view(np.uint32).reshape(-1, 8, 4).copy()
    nw = w.shape[0]
    assert np.ascontiguousarray(qnode).view(np.uint32).reshape(-1, 4, 4).shape[0] == nw
    ids = np.ascontiguousarray(w[:, 6, :]).view(np.int32)
    used = ids != ~n
    inner = used & (ids > 0)
    leafc = used & (ids < 0)
    lo = np.ascontiguousarray(w[:, 0:6:2, :]).view(F).copy()                       # [node][axis][slot]
    hi = np.ascontiguousarray(w[:, 1:6:2, :]).view(F).copy()
    face = leaf[np.where(leafc, ~ids.astype(np.int64), 0)]                         # [node][slot]
    lo = np.where(leafc[:, None, :], tri_lo[face].transpose(0, 2, 1), lo)
    hi = np.where(leafc[:, None, :], tri_hi[face].transpose(0, 2, 1), hi)
    level = _levels(np.where(inner, ids.astype(np.int64), -1))
    node_lo, node_hi = np.zeros((nw, 3), F), np.zeros((nw, 3), F)
    for d in range(int(level.max()), 0, -1):
        at = np.flatnonzero(level == d)
        c = np.where(inner[at], ids[at].astype(np.int64), 0)
        lo[at] = np.where(inner[at][:, None, :], node_lo[c].transpose(0, 2, 1), lo[at])
        hi[at] = np.where(inner[at][:, None, :], node_hi[c].transpose(0, 2, 1), hi[at])
        u = used[at][:, None, :]
        node_lo[at] = np.where(u, lo[at], F(np.inf)).min(axis=2)
        node_hi[at] = np.where(u, hi[at], F(-np.inf)).max(axis=2)
    w[:, 0:6:2, :] = lo.view(np.uint32)
    w[:, 1:6:2, :] = hi.view(np.uint32)
    return bmin, bmax, w, quantise(lo, hi, used, ids)

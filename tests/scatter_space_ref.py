'''what the spacing tests share (tests/test_scatter_space_cpu.py, tests/test_scatter_space_gpu.py): an independent numpy restatement
of a spaced scatter's elimination as include/miptina.h defines it, written from the definition, not from
scatter_rule.h, and the point sets both tests run.  Everything is f64, one correctly rounded IEEE operation per written operation
in the written order, so mpt_scatter_space_rule and the kernels are held to it exactly.

The definition, in short.  Candidates j and k CONFLICT iff d2 = ((dx dx) + (dy dy)) + (dz dz) < r2 = r r (exactly r apart is
allowed; a coordinate that is not finite makes the comparison false).  In candidate order j is KEPT iff no kept k < j conflicts
with it; the instances are the first `count` kept.  The same set comes out of ROUNDS over a state per candidate -- undecided, kept,
rejected: an undecided j looks at its conflicting lower neighbours; any kept: rejected; else none undecided: kept; else it waits.
In the synchronous form every candidate reads the states the round before left; its number of rounds bounds the device's.'''

import numpy as np

import scatter_ref as sc

UNDECIDED, KEPT, REJECTED = 0, 1, 2


def conflicts(points, r):
    '''[n,n] bool: which pairs conflict'''
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        d = p[:, None, :] - p[None, :, :]
        d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
        return d2 < np.float64(r) * np.float64(r)


def greedy(conflict):
    '''kept [n] bool by the sequential pass'''
    n = conflict.shape[0]
    kept = np.zeros(n, bool)
    for j in range(n):
        kept[j] = not (conflict[j, :j] & kept[:j]).any()
    return kept


def rounds(conflict):
    '''(kept [n] bool, rounds) by the synchronous rounds'''
    n = conflict.shape[0]
    lower = np.tril(conflict, -1)                                          # [j, k]: k < j and they conflict
    state = np.full(n, UNDECIDED)
    count = 0
    while (state == UNDECIDED).any():
        any_kept = (lower & (state == KEPT)[None, :]).any(axis=1)
        any_undecided = (lower & (state == UNDECIDED)[None, :]).any(axis=1)
        new = np.where(any_kept, REJECTED, np.where(any_undecided, UNDECIDED, KEPT))
        state = np.where(state == UNDECIDED, new, state)
        count += 1
        assert count <= n
    return state == KEPT, count


def eliminate(points, r):
    '''(kept [n] bool, rounds of the synchronous form); the two statements of the rule agree on every input'''
    c = conflicts(points, r)
    kept = greedy(c)
    by_rounds, count = rounds(c)
    assert np.array_equal(kept, by_rounds)
    return kept, count


def greedy_of_points(points, r):
    '''kept [n] bool by the sequential pass, a candidate at a time against the kept so far: no n x n table, for the tools' large sets'''
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    r2 = np.float64(r) * np.float64(r)
    kept = np.zeros(p.shape[0], bool)
    held = np.zeros((p.shape[0], 3))
    n = 0
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(p.shape[0]):
            d = p[j] - held[:n]
            if not (((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2]) < r2).any():
                kept[j], held[n] = True, p[j]
                n += 1
    return kept


def positions(P, points):
    '''[n,3]: the placement's point of the records `points` on the faces with world corners P [F,3,3]'''
    f = points['face']
    b1, b2 = points['b1'][:, None], points['b2'][:, None]
    b0 = (1.0 - b1) - b2
    return (b0 * P[f, 0] + b1 * P[f, 1]) + b2 * P[f, 2]


def spaced(P, candidates, r, count):
    '''(kept [M] bool, index [count] -- the candidates that become the instances --, rounds, positions [M,3]) of the candidate
    records over the world corners P'''
    pos = positions(P, candidates)
    kept, count_rounds = eliminate(pos, r)
    index = np.flatnonzero(kept)
    assert index.size >= count, 'precondition: %d of %d candidates kept, %d wanted' % (index.size, kept.size, count)
    return kept, index[:count].astype(np.int64), count_rounds, pos


# ---------------------------------------------------------------- the point sets of the door's tests
def _exact_pair():
    '''two points exactly r apart with d2 == r2 in f64: (3, 4, 12) r / 13 with r = 13 * 2^-4 -- every product and sum is exact'''
    r = 13.0 / 16
    a = np.array([0.25, -0.5, 1.0])
    return np.stack([a, a + np.array([3.0, 4.0, 12.0]) / 16]), r


def _ulp_below_pair():
    '''... and the second moved towards the first along x, an f64 at a time, until d2 < r2: a step moves dx dx by a fifth of an ulp of
    d2, so the first d2 below r2 is the f64 just below it'''
    pts, r = _exact_pair()
    r2 = np.float64(r) * np.float64(r)
    for _ in range(64):
        pts[1, 0] = np.nextafter(pts[1, 0], -np.inf)
        d = pts[1] - pts[0]
        d2 = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
        if d2 < r2:
            assert d2 == np.nextafter(r2, 0.0)
            return pts, r
    raise AssertionError('no such point')


def _borders(r):
    '''pairs r (1 - 2^-40) apart along each axis and along the space diagonal, their midpoints on cell borders 1, 2 and 1000 cell edges
    from the box's corner (the edge is r (1 + 2^-20); the box begins at the first point, the origin); the pairs along an axis stand
    far from each other and from the diagonal's'''
    h = r * (1.0 + 2.0 ** -20)
    gap = r * (1.0 - 2.0 ** -40)
    pts = [np.zeros(3)]
    q = 0
    for cells in (1, 2, 1000):
        for a in range(4):
            d = np.ones(3) / np.sqrt(3.0) if a == 3 else np.eye(3)[a]
            c = np.full(3, cells * h) if a == 3 else np.where(d > 0, cells * h, (2000 + 10 * q) * h)
            pts += [c - (0.5 * gap) * d, c + (0.5 * gap) * d]
            q += 1
    return np.array(pts)


def door_cases():
    '''[(name, points [n,3], r)]: the sizes at which each mechanism of the device can go wrong'''
    rng = np.random.default_rng(31)
    out = []
    out.append(('one point', np.array([[0.5, -1.0, 2.0]]), 0.3))
    pts, r = _exact_pair()
    out.append(('two points exactly r apart', pts, r))
    q, r = _ulp_below_pair()
    out.append(('two points an ulp of d2 below r', q, r))
    out.append(('64 coincident points', np.tile([[0.3, 0.1, -0.7]], (64, 1)), 0.25))
    chain = np.zeros((40, 3))
    chain[:, 0] = 0.6 * np.arange(40)
    out.append(('a chain of 40, 0.6 r apart', chain, 1.0))
    out.append(('the chain in reverse', chain[::-1].copy(), 1.0))
    out.append(('pairs across cell borders', _borders(0.37), 0.37))
    r = 2.0 ** -12
    far = 2.0 ** 30 * r
    out.append(('an extent of 2^30 r', np.array([[0, 0, 0], [0.5 * r, 0, 0], [far, far, far], [far, far - 0.75 * r, far], [0.5 * far, 0, 0]]), r))
    g = np.arange(10) * 1.5
    out.append(('a 10 x 10 x 10 lattice 1.5 r apart', np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3), 1.0))
    pts = rng.random((64, 3))
    pts[17, 1] = np.nan
    out.append(('a NaN coordinate among 63 points', pts, 0.2))
    out.append(('257 uniform points', rng.random((257, 3)), 0.14))
    out.append(('1000 uniform points', rng.random((1000, 3)), 0.09))
    return out

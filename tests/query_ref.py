'''
The yardstick of the batch ray queries (BVHTree.intersect / occluded): for single rays, which triangle of a model is the nearest
hit -- by plain float64 numpy over ALL triangles, no tree, nothing of ptina_amd -- and for which rays that answer cannot
depend on rounding.

A ray is its f32 origin and direction taken as f64, the direction normalised again in f64.  Every triangle gets its
Moller-Trumbore u, v, t, the cosine cos = |det| / |e1 x e2| between the ray and its normal, its bounding sphere (centroid c,
radius R), the sphere's position along the ray ta = (c - o) . d and its distance from the ray, and is one of

  away        the sphere is more than 1.01 R + 1e-9 from the ray or lies behind it (ta + 1.01 R < 0): no rounding makes it a hit
  sure hit    not away, cos >= COS, u >= B, v >= B, u + v <= 1 - B, t >= T_ABS
  sure miss   away, or cos >= COS and (u <= -B or v <= -B or u + v >= 1 + B or t <= -T_ABS)
  doubtful    everything else

with B the triangle's barycentric margin: BARY = 1e-4, and more for a sliver (below).

and the ray is DECIDED when either there is no sure hit and no doubtful triangle (a miss), or the nearest sure hit tn exists,
the second sure hit is beyond tn (1 + DEPTH_GAP) and every doubtful triangle's sphere begins beyond that too
(ta - 1.01 R > tn (1 + DEPTH_GAP)): that face.  On a decided ray hit, index and object must be exactly right.

One more term than a geometric search needs.  The reference's Face.intersect (geometries.py:129) tests a triangle only when
|n . d| >= eps with n = e1 x e2 NOT normalised and eps = 1e-6 (common.py:32): a triangle whose area is of the order of eps --
the 1e-3 fillers of the `deep` case, |n| = 4e-6 -- is by that definition parallel to most rays, and no tree can find what the
reference's own test rejects.  |n . d| is |det| of the solve above: below EPS_REF (1 - EPS_BAND) the triangle is a sure miss,
whatever else holds; within EPS_REF (1 +- EPS_BAND) -- a thousand times the f32 rounding of that dot product -- it is doubtful.

The margins classify rays; they are no tolerance on a kernel.  DEPTH_GAP is visibility_ref.DEPTH_GAP; T_ABS = 1e-3 covers the
reference's absolute epsilons on t.  BARY = 1e-4 is three orders above the f32 rounding of the reference's Face.intersect for a
well-shaped triangle -- and for a well-shaped one only: the reference divides by D = uv^2 - uu vv (geometries.py:134-143), which for
edges at an angle theta is -uu vv sin^2 theta, so its s and t carry a rounding of about 2^-24 uu vv / |D| = 2^-24 / sin^2 theta.
A random model has slivers (face 142 of `flat`: sin theta = 2.4e-3, and the oracle's own Face.intersect puts a point with
u + v = 0.947 at 1.02, outside).  The margin keeps its "three orders above the rounding" per triangle:
B = max(BARY, BARY_ROUNDINGS 2^-24 uu vv / |D|), never below the 1e-4; a degenerate triangle is never sure of anything but "away".
'''

import numpy as np

DEPTH_GAP = 1e-3           # relative (visibility_ref.DEPTH_GAP)
BARY = 1e-4
BARY_ROUNDINGS = 1e3       # a sliver's margin: this many f32 roundings of the reference's barycentric solve
COS = 1e-3
T_ABS = 1e-3
SPHERE = 1.01
EPS_REF = 1e-6             # the reference's eps (common.py:32) in Face.intersect's test abs(b) >= eps (geometries.py:129)
EPS_BAND = 1e-3
RAYS = 2048


def rays(pos, seed, n=RAYS):
    '''n f32 rays for the model pos [T][3][3]: origins uniform in its bounding box grown by a quarter each way (each extent
    floored at a tenth of the largest, so that a flat model is not coplanar with its rays); the first half aimed at a
    Dirichlet(1, 1, 1) point of a random triangle, the second half with uniform directions -> (o, d), f32 [n][3]'''
    rng = np.random.default_rng(seed)
    pos = np.asarray(pos, np.float64)
    lo, hi = pos.reshape(-1, 3).min(axis=0), pos.reshape(-1, 3).max(axis=0)
    cen, ext = (lo + hi) / 2, hi - lo
    ext = np.maximum(ext, 0.1 * ext.max())
    o = cen + (rng.random((n, 3)) - 0.5) * ext * 1.5
    half = n // 2
    tri = rng.integers(0, pos.shape[0], half)
    w = rng.dirichlet([1.0, 1.0, 1.0], half)
    target = (pos[tri] * w[:, :, None]).sum(axis=1)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:half] = target - o[:half]
    return o.astype(np.float32), d.astype(np.float32)


def octant(d):
    """the direction octant of each ray, 0 .. 7: bit k set where component k has its sign bit set (as the walks read 1 / d)"""
    sign = np.signbit(np.asarray(d, np.float32))
    return sign[:, 0] * 1 + sign[:, 1] * 2 + sign[:, 2] * 4


def bounce_rays(pos, o, d, ref, seed):
    """the rays a path would trace next from the decided hits of (o, d): origins the f64 hit points rounded to f32 -- on the
    surface, where a camera ray never starts --, avoid the face hit; the first half aimed at a Dirichlet(1, 1, 1) point of a
    random triangle, the second half with uniform directions -> (o, d, avoid): f32 [m][3], f32 [m][3], int32 [m]"""
    rng = np.random.default_rng(seed)
    pos = np.asarray(pos, np.float64)
    sel = np.flatnonzero(ref['decided'] & ref['hit'])
    d64 = np.asarray(d, np.float32).astype(np.float64)[sel]
    d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
    start = (np.asarray(o, np.float32).astype(np.float64)[sel] + ref['t'][sel, None] * d64).astype(np.float32)
    m = sel.size
    half = m // 2
    tri = rng.integers(0, pos.shape[0], half)
    w = rng.dirichlet([1.0, 1.0, 1.0], half)
    target = (pos[tri] * w[:, :, None]).sum(axis=1)
    nd = rng.normal(size=(m, 3))
    nd /= np.linalg.norm(nd, axis=1, keepdims=True)
    nd[:half] = target - start[:half].astype(np.float64)
    return start, nd.astype(np.float32), ref['index'][sel].astype(np.int32)


AXIS_RAYS = 1024


def axis_rays(pos, seed, n=AXIS_RAYS):
    """n f32 rays along the axes' planes: every direction has one component exactly zero and every other ray a second one
    (1 / d is +-inf there, o / d inf or NaN); half of the zeros are -0.0.  The first half aimed: the origin is a Dirichlet point
    of a random triangle moved back along the ray (- s d); the second half starts as rays() starts -> (o, d)"""
    rng = np.random.default_rng(seed)
    pos = np.asarray(pos, np.float64)
    lo, hi = pos.reshape(-1, 3).min(axis=0), pos.reshape(-1, 3).max(axis=0)
    cen, ext = (lo + hi) / 2, hi - lo
    ext = np.maximum(ext, 0.1 * ext.max())
    d = rng.normal(size=(n, 3))
    first = rng.integers(0, 3, n)
    second = (first + 1 + rng.integers(0, 2, n)) % 3
    rows = np.arange(n)
    d[rows, first] = 0.0
    two = rows[1::2]
    d[two, second[two]] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = cen + (rng.random((n, 3)) - 0.5) * ext * 1.5
    half = n // 2
    tri = rng.integers(0, pos.shape[0], half)
    w = rng.dirichlet([1.0, 1.0, 1.0], half)
    s = (0.05 + rng.random(half)) * ext.max()
    o[:half] = (pos[tri] * w[:, :, None]).sum(axis=1) - s[:, None] * d[:half]
    d = d.astype(np.float32)
    zero = np.argwhere(d == 0)
    minus = zero[rng.permutation(zero.shape[0])[:zero.shape[0] // 2]]
    d[minus[:, 0], minus[:, 1]] = np.float32(-0.0)
    return o.astype(np.float32), d


def far_rays(pos, radii, seed, n=256):
    """n f32 rays aimed at Dirichlet points of random triangles from `radii` bounding radii away from the model's centre"""
    rng = np.random.default_rng(seed)
    pos = np.asarray(pos, np.float64)
    lo, hi = pos.reshape(-1, 3).min(axis=0), pos.reshape(-1, 3).max(axis=0)
    cen, rad = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (cen + radii * rad * u).astype(np.float32)
    tri = rng.integers(0, pos.shape[0], n)
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    target = (pos[tri] * w[:, :, None]).sum(axis=1)
    # every other ray passes the model by: aimed at a point a radius and a half beside it
    target[1::2] += 1.5 * rad * np.cross(u[1::2], rng.normal(size=(n // 2, 3)))
    return o, (target - o.astype(np.float64)).astype(np.float32)


def _terms(pos, o, d):
    '''per (ray, triangle): u, v, t, cos, and the triangle's class -> (u, v, t, sure_hit, doubtful, ta - SPHERE R)'''
    v0, e1, e2 = pos[:, 0], pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    nrm = np.linalg.norm(np.cross(e1, e2), axis=1)
    c = pos.mean(axis=1)
    R = np.linalg.norm(pos - c[:, None, :], axis=2).max(axis=1)
    o_, d_ = o[:, None, :], d[:, None, :]
    uu, vv, uv = (e1 * e1).sum(axis=1), (e2 * e2).sum(axis=1), (e1 * e2).sum(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        B = np.maximum(BARY, BARY_ROUNDINGS * 2.0 ** -24 * uu * vv / np.abs(uv * uv - uu * vv))
    B = np.where(np.isfinite(B), B, np.inf)[None]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        p = np.cross(d_, e2[None])
        det = (e1[None] * p).sum(axis=2)
        s = o_ - v0[None]
        u = (s * p).sum(axis=2) / det
        q = np.cross(s, e1[None])
        v = (d_ * q).sum(axis=2) / det
        t = (e2[None] * q).sum(axis=2) / det
        cos = np.abs(det) / nrm[None]
        oc = c[None] - o_
        ta = (oc * d_).sum(axis=2)
        off = np.linalg.norm(oc - ta[..., None] * d_, axis=2)
        away = (off > SPHERE * R[None] + 1e-9) | (ta + SPHERE * R[None] < 0)
        steep = cos >= COS
        parallel = np.abs(det) < EPS_REF * (1 - EPS_BAND)                      # (to the reference: see the module docstring)
        tested = np.abs(det) > EPS_REF * (1 + EPS_BAND)
        sure_hit = ~away & tested & steep & (u >= B) & (v >= B) & (u + v <= 1 - B) & (t >= T_ABS)
        sure_miss = away | parallel | (steep & ((u <= -B) | (v <= -B) | (u + v >= 1 + B) | (t <= -T_ABS)))
    return u, v, t, sure_hit, ~sure_hit & ~sure_miss, ta - SPHERE * R[None]


def classify(pos, o, d, avoid=None, block=128):
    '''pos [T][3][3], f32 rays o, d [n][3], avoid None or [n] (the face a ray does not see: the model without it) ->
    dict of [n] arrays: decided, hit (the decided verdict), index (the face, -1), t, u, v (f64, of that face)'''
    pos = np.asarray(pos, np.float64)
    o = np.asarray(o, np.float32).astype(np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float32).astype(np.float64).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    n = o.shape[0]
    out = dict(decided=np.zeros(n, bool), hit=np.zeros(n, bool), index=np.full(n, -1, np.int64), t=np.full(n, np.inf),
               u=np.zeros(n), v=np.zeros(n))
    for a in range(0, n, block):
        b = min(n, a + block)
        u, v, t, sure, doubt, begin = _terms(pos, o[a:b], d[a:b])
        if avoid is not None:
            r = np.flatnonzero(np.asarray(avoid[a:b]) >= 0)
            sure[r, np.asarray(avoid[a:b])[r]] = False
            doubt[r, np.asarray(avoid[a:b])[r]] = False
        ts = np.where(sure, t, np.inf)
        k = ts.argmin(axis=1)
        rows = np.arange(b - a)
        tn = ts[rows, k]
        ts[rows, k] = np.inf
        second = ts.min(axis=1)
        any_sure, any_doubt = sure.any(axis=1), doubt.any(axis=1)
        limit = tn * (1 + DEPTH_GAP)
        doubt_near = (doubt & ~(begin > limit[:, None])).any(axis=1)
        is_hit = any_sure & (second > limit) & ~doubt_near
        is_miss = ~any_sure & ~any_doubt
        out['decided'][a:b] = is_hit | is_miss
        out['hit'][a:b] = is_hit
        out['index'][a:b] = np.where(is_hit, k, -1)
        out['t'][a:b] = np.where(is_hit, tn, np.inf)
        out['u'][a:b] = np.where(is_hit, u[rows, k], 0.0)
        out['v'][a:b] = np.where(is_hit, v[rows, k], 0.0)
    return out


def caps(name, ref):
    '''the cap that keeps the tests honest, asserted before any kernel output is looked at -> (decided, hits, misses) shares'''
    dec = float(ref['decided'].mean())
    hits = float((ref['decided'] & ref['hit']).mean())
    misses = float((ref['decided'] & ~ref['hit']).mean())
    print(f'{name}: decided {dec:.3f}, decided hits {hits:.3f}, decided misses {misses:.3f} of {ref["decided"].size} rays')
    assert dec >= (0.60 if name == 'flat' else 0.90), (name, dec)
    assert hits >= 0.20 and misses >= 0.20, (name, hits, misses)
    return dec, hits, misses


def caps_of_set(name, which, ref):
    """the caps of the bounce (B) and axis (C) ray sets, asserted before any kernel output is looked at: decided >= 0.90, decided
    hits and decided misses >= 0.20 each; set C of the coplanar `flat`: decided >= 0.60, hits >= 0.10"""
    dec = float(ref['decided'].mean())
    hits = float((ref['decided'] & ref['hit']).mean())
    misses = float((ref['decided'] & ~ref['hit']).mean())
    print(f'{name} set {which}: decided {dec:.3f}, decided hits {hits:.3f}, decided misses {misses:.3f} of {ref["decided"].size} rays')
    if name == 'flat':
        assert which == 'C', 'set B is not used on flat: a coplanar model has no bounce hits'
        assert dec >= 0.60 and hits >= 0.10, (name, which, dec, hits)
    else:
        assert dec >= 0.90 and hits >= 0.20 and misses >= 0.20, (name, which, dec, hits, misses)
    return dec, hits, misses


def errors(ref, got, what, first=None, tol_depth=None, tol_uv=None):
    '''messages for every decided ray whose answer is not the reference's: hit and index exactly, object exactly where `first`
    (the objects' first faces; None: every object must be -1) is given, depth / u / v within the tolerances where given'''
    dec = ref['decided']
    hit, index = np.asarray(got['hit']).astype(bool), np.asarray(got['index'])
    bad = []
    for r in np.flatnonzero(dec & ((hit != ref['hit']) | (index != ref['index'])))[:8]:
        bad.append(f'{what}: ray {r} gives hit {bool(hit[r])} face {int(index[r])}, the reference hit {bool(ref["hit"][r])} face {int(ref["index"][r])} at t {ref["t"][r]:.6g}')
    if 'object' in got:
        want = np.full(dec.size, -1) if first is None else np.where(ref['hit'], np.searchsorted(np.asarray(first), ref['index'], side='right') - 1, -1)
        for r in np.flatnonzero(dec & (np.asarray(got['object']) != want))[:8]:
            bad.append(f'{what}: ray {r} gives object {int(got["object"][r])}, face {int(ref["index"][r])} belongs to {int(want[r])}')
    ok = dec & ref['hit'] & hit & (index == ref['index'])
    if tol_depth is not None:
        dev = np.abs(np.asarray(got['depth'], np.float64) - np.where(ok, ref['t'], 0.0))
        for r in np.flatnonzero(ok & ~(dev <= tol_depth))[:8]:
            bad.append(f'{what}: ray {r} depth {float(got["depth"][r])!r} against {ref["t"][r]!r}: off by {dev[r]:.3g} > {tol_depth:.3g}')
    if tol_uv is not None:
        for key in ('u', 'v'):
            dev = np.abs(np.asarray(got[key], np.float64) - ref[key])
            for r in np.flatnonzero(ok & ~(dev <= tol_uv))[:8]:
                bad.append(f'{what}: ray {r} {key} {float(got[key][r])!r} against {ref[key][r]!r}: off by {dev[r]:.3g} > {tol_uv:.3g}')
    return bad


def deviation(ref, got):
    '''largest |depth - t| and largest |u - u64|, |v - v64| over the decided hits -> (depth, uv)'''
    ok = ref['decided'] & ref['hit']
    dd = np.abs(np.asarray(got['depth'], np.float64) - ref['t'])[ok]
    du = np.abs(np.asarray(got['u'], np.float64) - ref['u'])[ok]
    dv = np.abs(np.asarray(got['v'], np.float64) - ref['v'])[ok]
    return float(dd.max()), float(max(du.max(), dv.max()))


def normalized32(d):
    '''the f32 direction a kernel traces: d / |d| in f32'''
    d = np.asarray(d, np.float32)
    return (d / np.sqrt((d * d).sum(axis=1, dtype=np.float32))[:, None]).astype(np.float32)


def oracle_answers(o_, o, d, avoid=None):
    '''the CPU oracle's own f32 LinearBVH.intersect (oracle.Oracle.intersect) of every ray, its direction normalised in f32 ->
    the dict BVHTree.intersect returns (without object)'''
    dn = normalized32(d)
    n = dn.shape[0]
    out = dict(hit=np.zeros(n, bool), depth=np.zeros(n, np.float32), index=np.zeros(n, np.int32), u=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    for r in range(n):
        h, depth, index, u, v = o_.intersect(o[r], dn[r], -1 if avoid is None else int(avoid[r]))
        out['hit'][r], out['depth'][r], out['index'][r], out['u'][r], out['v'][r] = h != 0, depth, index, u, v
    return out

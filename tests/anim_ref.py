'''what the animation tests share (tests/test_anim_cpu.py, tests/test_anim_gpu.py): a restatement of the rule of
ptina_amd/csrc/anim_rule.h, scalar by scalar in f64 in exactly the written order -- Python floats are IEEE
doubles and + - * / sqrt floor are correctly rounded on both sides, so host and device are held to it BIT FOR BIT wherever the slerp's
theta branch is not taken.  That branch calls acos and sin, each side its own library's: there the two are held to error_bound, a
first-order bound of their difference.

The same code runs over two kinds of number: float, and Err -- a value with a bound of how far the other evaluation's may lie from it.
Every Err operation adds the roundings of both evaluations (2 U |result|: each rounds its own operands once, half an ulp) to what
its operands carry, propagated to first order (products of two errors are dropped, as compose_ref.error_bound drops them); acos and
sin add (ulp_a + ulp_b) units in the last place of their result, the library errors of the two sides, carried on through the
division by sin theta (theta >= acos 0.9995: at most x 32), the quaternion-to-matrix expressions and the products down the chain.
Branches follow the values: everything a branch depends on (key search, d against 0 and 0.9995) is computed without a library
function and is the same bits on both sides.'''

import math

import numpy as np

from ptina_amd.tools.anim import Track, track, pack_clip      # noqa: F401  (the tests build their clips with these)

U = 2.0 ** -53
# Units in the last place by which a library's f64 acos and sin may miss the exact value: twice the largest error measured against
# np.longdouble over the arguments the tests use, rounded up to an integer (DESIGN.md section 3.17.1 has the measurements; the tests
# test_host_trig_stays_within_its_measured_error and test_device_trig_stays_within_its_measured_error assert the margin).
# Measured over the 296 acos and 888 sin arguments of cases(): glibc's libm 0.4966 and 0.5005; the device library on an MI355X
# (through mpt_anim_trig) 0.6235 and 0.6958.
ULP_TRIG_HOST = 2              # ceil(2 * 0.5005)
ULP_TRIG_DEVICE = 2            # ceil(2 * 0.6958)
CAP = 1e-9                     # the asserted bound may not exceed this, relative to the palette's largest entry: else the derivation is wrong
THETA_D = 0.9995

_state = {'theta': 0, 'ulps': 0.0, 'args': None}


class Err:
    '''a value v and a first-order bound e of |the other evaluation's value - v|'''
    __slots__ = ('v', 'e')

    def __init__(self, v, e=0.0):
        self.v, self.e = float(v), float(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def __add__(self, o):
        o = Err.of(o)
        v = self.v + o.v
        return Err(v, self.e + o.e + 2 * U * abs(v))
    __radd__ = __add__

    def __sub__(self, o):
        o = Err.of(o)
        v = self.v - o.v
        return Err(v, self.e + o.e + 2 * U * abs(v))

    def __rsub__(self, o):
        return Err.of(o) - self

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, o):
        o = Err.of(o)
        v = self.v * o.v
        return Err(v, abs(self.v) * o.e + abs(o.v) * self.e + 2 * U * abs(v))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o)
        v = self.v / o.v
        return Err(v, self.e / abs(o.v) + abs(v) * o.e / abs(o.v) + 2 * U * abs(v))

    def __lt__(self, o):
        return self.v < Err.of(o).v

    def __gt__(self, o):
        return self.v > Err.of(o).v


def _val(x):
    return x.v if isinstance(x, Err) else x


def _sqrt(x):
    if isinstance(x, Err):
        v = math.sqrt(x.v)
        return Err(v, x.e / (2 * v) + 2 * U * v)
    return math.sqrt(x)


def _lib(name, fn, x, slope):
    '''a library function: the host's value; under Err its two sides' library errors and what the argument carries, by |slope|'''
    if _state['args'] is not None:
        _state['args'][name].append(_val(x))
    if isinstance(x, Err):
        v = fn(x.v)
        return Err(v, abs(slope(x.v)) * x.e + _state['ulps'] * float(np.spacing(abs(v))))
    return fn(x)


def _acos(x):
    return _lib('acos', math.acos, x, lambda v: 1.0 / math.sqrt(max(1.0 - v * v, 1e-300)))


def _sin(x):
    return _lib('sin', math.sin, x, math.cos)


# ---------------------------------------------------------------- the rule
def components(path, ntargets):
    return 4 if path == 1 else ntargets if path == 3 else 3


def span(tracks):
    '''[t0, t1] of a clip: the least first key to the greatest last key (0, 0 without tracks)'''
    if not tracks:
        return 0.0, 0.0
    return min(float(t.times[0]) for t in tracks), max(float(t.times[-1]) for t in tracks)


def local_time(t, offset, speed, loop, t0, t1):
    tau = (t - offset) * speed
    if loop and t1 > t0:
        x, d = tau - t0, t1 - t0
        with np.errstate(invalid='ignore'):
            tau = t0 + (x - float(np.floor(np.float64(x / d))) * d)
    return tau


def key(T, tau):
    '''(k, None) at key k itself, or (k, (dt, u)) between keys k and k + 1'''
    n = len(T)
    if n == 1 or not tau > T[0]:
        return 0, None
    if tau >= T[n - 1]:
        return n - 1, None
    lo, hi = 0, n - 1
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if T[mid] <= tau:
            lo = mid
        else:
            hi = mid
    dt = T[lo + 1] - T[lo]
    return lo, (dt, (tau - T[lo]) / dt)


def normalise4(q):
    ln = _sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [c / ln for c in q]


def slerp(a, b, u):
    d = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]
    if d < 0.0:
        b, d = [-c for c in b], -d
    if d > THETA_D:
        return normalise4([a[c] + u * (b[c] - a[c]) for c in range(4)])
    _state['theta'] += 1
    theta = _acos(d)
    sa, sb, s = _sin((1.0 - u) * theta), _sin(u * theta), _sin(theta)
    return [(sa * a[c] + sb * b[c]) / s for c in range(4)]


def sample(tr, ntargets, tau, N=float):
    '''the values of Track tr at tau, as numbers of kind N'''
    C = components(tr.path, ntargets)
    T = [float(x) for x in tr.times]
    V = np.asarray(tr.values, np.float32).reshape(len(T), -1)
    cubic = tr.interpolation == 2
    val = (lambda k: [N(float(x)) for x in V[k, C:2 * C]]) if cubic else (lambda k: [N(float(x)) for x in V[k, :C]])
    k, between = key(T, tau)
    v0 = val(k)
    if between is None or tr.interpolation == 0:
        return v0
    dt, u = between
    v1 = val(k + 1)
    if not cubic:
        if tr.path != 1:
            return [v0[c] + u * (v1[c] - v0[c]) for c in range(C)]
        return slerp(v0, v1, u)
    b0 = [N(float(x)) for x in V[k, 2 * C:3 * C]]
    a1 = [N(float(x)) for x in V[k + 1, 0:C]]
    u2 = u * u
    u3 = u2 * u
    h00, h10, h01, h11 = (2.0 * u3 - 3.0 * u2) + 1.0, (u3 - 2.0 * u2) + u, 3.0 * u2 - 2.0 * u3, u3 - u2
    g10, g11 = h10 * dt, h11 * dt
    p = [((h00 * v0[c] + g10 * b0[c]) + h01 * v1[c]) + g11 * a1[c] for c in range(C)]
    return normalise4(p) if tr.path == 1 else p


def local(trs):
    '''[R(q) diag(s) | t] as 12 numbers of trs = t3 q4 (x y z w) s3'''
    x, y, z, w = trs[3:7]
    R = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
         2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
         2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]
    M = []
    for r in range(3):
        M += [R[3 * r + c] * trs[7 + c] for c in range(3)] + [trs[r]]
    return M


def mul(A, B):
    out = []
    for r in range(3):
        out += [(A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c] for c in range(3)]
        out.append(((A[4 * r] * B[3] + A[4 * r + 1] * B[7]) + A[4 * r + 2] * B[11]) + A[4 * r + 3])
    return out


def _locals(skel, ntargets, tracks, binding, t, N):
    '''(weights, the joints' local matrices as 12 numbers each, parents, inverse binds [nj,12])'''
    parents, rest, ib = skel if skel is not None else (np.zeros(0, np.int64), np.zeros((0, 10)), np.zeros((0, 3, 4)))
    nj = len(parents)
    rest, ib = np.asarray(rest, np.float64).reshape(nj, 10), np.asarray(ib, np.float64).reshape(nj, 12)
    offset, speed, loop = binding
    tau = local_time(float(t), float(offset), float(speed), bool(loop), *span(tracks))
    trs = [[N(float(x)) for x in rest[j]] for j in range(nj)]
    w = [N(0.0)] * ntargets
    for tr in tracks:
        v = sample(tr, ntargets, tau, N)
        if tr.path == 3:
            w = v
        else:
            at = (0, 3, 7)[tr.path]
            trs[tr.target][at:at + len(v)] = v
    return w, [local(x) for x in trs], parents, ib


def pose(skel, ntargets, tracks, binding, t):
    '''(weights [ntargets], palette [nj,3,4], theta) f64 of an object at scene time t: skel = (parents [nj], rest [nj,10],
    inverse_bind [nj,3,4]) or None, tracks a list of Tracks, binding = (offset, speed, loop); theta: how often the slerp's theta
    branch was taken (0: the pose is reproducible bit for bit)'''
    _state['theta'] = 0
    w, loc, parents, ib = _locals(skel, ntargets, tracks, binding, t, float)
    glob, pal = [], []
    for j, G in enumerate(loc):
        if parents[j] >= 0:
            G = mul(glob[int(parents[j])], G)
        glob.append(G)
        pal.append(mul(G, [float(x) for x in ib[j]]))
    return np.array(w, np.float64).reshape(ntargets), np.array(pal, np.float64).reshape(len(pal), 3, 4), _state['theta']


def _product_bound(A, eA, B, eB):
    '''(e3, et) of C = A . B for affine A = (A3 | a) and B = (B3 | b) [3,4] whose two evaluations lie within eA = (Frobenius norm of
    the 3x3 parts' difference, norm of the translations') and eB of one another.  In norms, because a chain of 256 rotations keeps
    its 2-norm where entrywise bounds through |A| |B| grow with every level:
        |dC3|_F <= |dA3|_F |B3|_2 + |A3|_2 |dB3|_F + 6 U |A3|_F |B3|_F                 three terms summed, both sides' roundings
        |dc|    <= |dA3|_F |b| + |A3|_2 |db| + |da| + 8 U (|A3|_F |b| + |a|)           four terms'''
    A3, a, B3, b = A[:, :3], A[:, 3], B[:, :3], B[:, 3]
    n2, fro = (lambda M: float(np.linalg.norm(M, 2))), (lambda M: float(np.linalg.norm(M)))
    e3 = eA[0] * n2(B3) + n2(A3) * eB[0] + 6 * U * fro(A3) * fro(B3)
    et = eA[0] * fro(b) + n2(A3) * eB[1] + eA[1] + 8 * U * (fro(A3) * fro(b) + fro(a))
    return e3, et


def error_bound(skel, ntargets, tracks, binding, t, ulp_a, ulp_b):
    '''(weights' bounds [ntargets], palette's [nj,3,4]): how far two evaluations whose acos and sin miss by ulp_a and ulp_b units in
    the last place may lie apart, to first order (the head of the file): entry by entry up to the joints' local matrices, in norms
    down the chain (_product_bound), so that every entry of a palette matrix's 3x3 part carries the bound of its Frobenius norm'''
    _state['ulps'] = float(ulp_a + ulp_b)
    w, loc, parents, ib = _locals(skel, ntargets, tracks, binding, t, Err)
    nj = len(loc)
    out = np.zeros((nj, 3, 4))
    glob = []
    for j in range(nj):
        G = np.array([x.v for x in loc[j]]).reshape(3, 4)
        e = np.array([x.e for x in loc[j]]).reshape(3, 4)
        eG = (float(np.linalg.norm(e[:, :3])), float(np.linalg.norm(e[:, 3])))
        if parents[j] >= 0:
            P, eP = glob[int(parents[j])]
            eG = _product_bound(P, eP, G, eG)
            G = np.array(mul(list(P.reshape(-1)), list(G.reshape(-1)))).reshape(3, 4)
        glob.append((G, eG))
        out[j, :, :3], out[j, :, 3] = _product_bound(G, eG, ib[j].reshape(3, 4), (0.0, 0.0))
    return np.array([x.e for x in w], np.float64).reshape(ntargets), out


def record_trig(fn):
    '''run fn() and return the arguments the restatement handed to acos and sin meanwhile: {'acos': [...], 'sin': [...]}'''
    _state['args'] = {'acos': [], 'sin': []}
    try:
        fn()
        return {k: np.array(v, np.float64) for k, v in _state['args'].items()}
    finally:
        _state['args'] = None


def trig_ulps(x, got, name):
    '''the errors of got = acos(x) / sin(x) in units of the last place of the exact value, taken with np.longdouble (64 bits of
    mantissa: its own error is 2^-11 of such a unit)'''
    x, got = np.asarray(x, np.float64), np.asarray(got, np.float64)
    exact = getattr(np, 'arccos' if name == 'acos' else 'sin')(x.astype(np.longdouble))
    ulp = np.spacing(np.abs(exact.astype(np.float64))).astype(np.longdouble)
    return np.abs(got.astype(np.longdouble) - exact) / ulp


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_pose(got, skel, ntargets, tracks, binding, t, ulp_got, what=''):
    '''holds got = (weights, palette) to the restatement: bit for bit off the theta branch, within error_bound (capped) on it.
    Returns (theta, the largest |got - restatement| / bound, or 0.0)'''
    w, pal, theta = pose(skel, ntargets, tracks, binding, t)
    if theta == 0:
        assert same_bits(got[0], w) and same_bits(got[1], pal), (what, 'not the restatement\'s bits', np.abs(got[1] - pal).max() if pal.size else 0,
                                                                 np.abs(got[0] - w).max() if w.size else 0)
        return 0, 0.0
    ew, ep = error_bound(skel, ntargets, tracks, binding, t, ulp_got, ULP_TRIG_HOST)
    assert same_bits(got[0], w), (what, 'weights do not pass the slerp')
    scale = float(np.abs(pal).max())
    assert ep.max() <= CAP * scale, (what, 'the bound exceeds the cap: the derivation is wrong', float(ep.max()), scale)
    diff = np.abs(got[1] - pal)
    ratio = float((diff[ep > 0] / ep[ep > 0]).max()) if (ep > 0).any() else 0.0
    print('%s: theta branch x%d, bound <= %.3g (%.3g of the largest entry), largest |got - restatement| / bound %.4f' % (what, theta, ep.max(), ep.max() / scale, ratio))
    assert np.all(diff <= ep), (what, ratio, float(diff.max()))
    return theta, ratio


# ---------------------------------------------------------------- skeletons and clips (fixed seeds)
def skeleton(g, nj, shape='tree', scales=(0.95, 1.05)):
    '''(parents [nj], rest [nj,10], inverse_bind [nj,3,4]): shape 'chain' (nj deep), 'star' (all under joint 0), 'tworoots' (two
    chains side by side) or 'tree' (random parents).  Rest rotations are unit to f64 rounding, scales near 1, shifts small enough
    that a chain of 256 stays finite and tame'''
    if shape == 'chain':
        parents = np.arange(nj) - 1
    elif shape == 'star':
        parents = np.where(np.arange(nj) == 0, -1, 0)
    elif shape == 'tworoots':
        parents = np.arange(nj) - 2
        parents[:2] = -1
    else:
        parents = np.array([-1] + [int(g.integers(0, j)) for j in range(1, nj)])
    q = g.normal(size=(nj, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rest = np.concatenate([g.uniform(-0.2, 0.2, (nj, 3)), q, g.uniform(*scales, (nj, 3))], axis=1)
    ib = np.zeros((nj, 3, 4))
    for j in range(nj):
        a = g.normal(size=4)
        a /= np.linalg.norm(a)
        ib[j] = np.array(local([g.uniform(-0.5, 0.5), g.uniform(-0.5, 0.5), g.uniform(-0.5, 0.5), *a, 1.0, 1.0, 1.0])).reshape(3, 4)
    return parents.astype(np.int64), rest, ib


def rotation_keys(g, n, mode):
    '''[n,4] f32 rotations, about unit: mode 'far' -- independent, so that neighbours take the theta branch (d < 0.9995 almost
    surely); 'near' -- each within 0.02 rad of the one before on the 3-sphere (d > 0.9995: nlerp); 'flip' -- near, with every other
    key negated (d < 0: the shorter arc)'''
    q = g.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if mode != 'far':
        for k in range(1, n):
            step = g.normal(size=4)
            q[k] = q[k - 1] + 0.02 * g.uniform(0.2, 1.0) * step / np.linalg.norm(step)
            q[k] /= np.linalg.norm(q[k])
        if mode == 'flip':
            q[1::2] *= -1
    return q.astype(np.float32)


def random_track(g, target, path, interp, nkeys, ntargets=0, rot='far', t_first=0.0, t_last=2.0):
    C = components(path, ntargets)
    times = np.sort(g.uniform(t_first, t_last, nkeys)).astype(np.float32)
    times[0], times[-1] = (t_first, t_last) if nkeys > 1 else (t_first, t_first)
    times = np.unique(times)
    while times.size < nkeys:                                                # (f32 ties: vanishingly rare)
        times = np.unique(np.append(times, g.uniform(t_first, t_last)).astype(np.float32))
    if path == 1:
        v = rotation_keys(g, nkeys, rot)
    elif path == 2:
        v = g.uniform(0.8, 1.25, (nkeys, C)).astype(np.float32)
    elif path == 0:
        v = g.uniform(-0.3, 0.3, (nkeys, C)).astype(np.float32)
    else:
        v = g.uniform(-1.0, 1.5, (nkeys, C)).astype(np.float32)
    if interp == 2:
        tan = g.normal(scale=0.3, size=(2, nkeys, C)).astype(np.float32)
        v = np.stack([tan[0], v, tan[1]], axis=1)
    return Track(int(target), int(path), int(interp), times, v)


def random_clip(g, nj, T, rot='far', nkeys=(1, 2, 33), interps=(0, 1, 2), density=0.7, t_last=2.0, paths=(0, 1, 2)):
    '''tracks over nj joints and T morph targets: each (joint, path) has a track with probability `density`, of a random
    interpolation and key count from the given ones; all start at 0, and the first ends at t_last (the clip's span).  rot: what
    LINEAR rotation tracks do ('far': the theta branch; 'near' / 'flip': nlerp)'''
    tracks = []
    for j in range(nj):
        for path in paths:
            if g.random() < density:
                interp = int(g.choice(interps))
                tracks.append(random_track(g, j, path, interp, int(g.choice(nkeys)), rot=rot, t_last=t_last))
    if T and (g.random() < density or not tracks):
        tracks.append(random_track(g, -1, 3, int(g.choice(interps)), int(g.choice(nkeys)), ntargets=T, t_last=t_last))
    if tracks and tracks[0].times.size == 1:
        tr = tracks[0]
        tracks[0] = random_track(g, tr.target, tr.path, tr.interpolation, 2, ntargets=T, rot=rot, t_last=t_last)
    return tracks


# ---------------------------------------------------------------- the cases both test files walk
TIMES = (1.0, 1.71)            # the scene times the cases are evaluated at; every clip spans [0, 2]


def bindings(tracks, n=None):
    '''(offset, speed, loop) of the objects of a case, chosen for scene time 1.0: local time inside the span; exactly on t1 = 2 (a
    loop wraps it to t0) and exactly on t0; exactly on an inner key, looped and clamped; before the first key and behind the last,
    clamped; speed 0; negative speed; a local time of -1 that the loop wraps to 1; offset and speed together'''
    many = [t for t in tracks if t.times.size > 2]
    k = float(many[0].times[many[0].times.size // 2]) if many else 0.5
    out = [(0.0, 1.0, True), (-1.0, 1.0, True), (1.0, 1.0, True), (1.0 - k, 1.0, True), (1.0 - k, 1.0, False), (3.0, 1.0, False), (-4.0, 1.0, False),
           (0.25, 0.0, True), (0.5, -1.5, True), (2.0, 1.0, True), (-0.375, 2.0, False)]
    return out if n is None else [out[i] for i in (0, 3, 8, 1, 5)[:n]]


def _pair(a, b, interp=1):
    return np.array([a, b], np.float32) if interp != 2 else None


def cases():
    '''[(name, skel or None, ntargets, tracks, bindings, exact)]: exact -- no object of the case takes the slerp's theta branch at
    TIMES (the tests check that this is so)'''
    g = np.random.default_rng(1721)
    out = []
    # one joint, every path animated: LINEAR translation of 2 keys, a LINEAR rotation of 33 keys that takes the theta branch, CUBICSPLINE scale
    tr = [random_track(g, 0, 0, 1, 2), random_track(g, 0, 1, 1, 33, rot='far'), random_track(g, 0, 2, 2, 2)]
    out.append(('one joint, theta', skeleton(g, 1), 0, tr, bindings(tr), False))
    # five joints under two roots: none, only T (STEP), only R (CUBICSPLINE), only S (LINEAR, one key), STEP R + CUBICSPLINE T; 3 targets LINEAR
    tr = [random_track(g, 1, 0, 0, 33), random_track(g, 2, 1, 2, 33), random_track(g, 3, 2, 1, 1), random_track(g, 4, 1, 0, 2), random_track(g, 4, 0, 2, 33),
          random_track(g, -1, 3, 1, 33, ntargets=3)]
    out.append(('five joints, two roots', skeleton(g, 5, 'tworoots'), 3, tr, bindings(tr), True))
    # the same rig with LINEAR on T and R (nlerp, and nlerp along the shorter arc) and STEP on S and W
    tr = [random_track(g, 0, 0, 1, 33), random_track(g, 1, 1, 1, 33, rot='near'), random_track(g, 2, 1, 1, 2, rot='flip'), random_track(g, 3, 2, 0, 33),
          random_track(g, 4, 2, 2, 33), random_track(g, -1, 3, 0, 2, ntargets=3)]
    out.append(('five joints, nlerp', skeleton(g, 5, 'tworoots'), 3, tr, bindings(tr), True))
    # 64 joints as a star, one target, CUBICSPLINE weights
    tr = random_clip(g, 64, 0, rot='near') + [random_track(g, -1, 3, 2, 33, ntargets=1)]
    out.append(('star of 64', skeleton(g, 64, 'star'), 1, tr, bindings(tr, 5), True))
    tr = random_clip(g, 64, 0, rot='far', density=0.5)
    out.append(('tree of 64, theta', skeleton(g, 64, 'tree'), 0, tr, bindings(tr, 3), False))
    # a chain 256 deep
    tr = random_clip(g, 256, 0, rot='flip', density=0.5)
    out.append(('chain of 256', skeleton(g, 256, 'chain'), 0, tr, bindings(tr, 3), True))
    # ... and one that takes the theta branch.  Its scales are 1 and only T and R are animated: down a chain the bound multiplies what a
    # joint carries by the 2-norm of every matrix below it, and only rotations keep that at 1 (the chain above has the scales, bit for bit)
    tr = random_clip(g, 256, 0, rot='far', density=0.2, interps=(1,), paths=(0, 1))
    out.append(('chain of 256, theta', skeleton(g, 256, 'chain', scales=(1.0, 1.0)), 0, tr, bindings(tr, 2), False))
    # morph targets and no skin: weight tracks only
    tr = [random_track(g, -1, 3, 2, 33, ntargets=3)]
    out.append(('morph only, 3 targets', None, 3, tr, bindings(tr), True))
    tr = [random_track(g, -1, 3, 1, 2, ntargets=1)]
    out.append(('morph only, 1 target', None, 1, tr, bindings(tr), True))
    # the slerp's corners, a joint each, two keys at 0 and 2 from the identity: a far rotation negated (d < 0 and nlerp behind the flip), identical
    # keys (d = 1), and d = the f32 next above the double 0.9995 -- nlerp all; then d < 0 with theta, d = the f32 next below 0.9995, a half turn
    lo = np.float32(0.9995)
    lo, hi = (np.nextafter(lo, np.float32(0)), lo) if float(lo) > THETA_D else (lo, np.nextafter(lo, np.float32(1)))
    assert float(lo) <= THETA_D < float(hi)
    one = [0.0, 0.0, 0.0, 1.0]
    R = lambda j, b: Track(j, 1, 1, np.float32([0, 2]), np.float32([one, b]))     # noqa: E731
    nb = (-rotation_keys(g, 2, 'near')).tolist()
    tr = [Track(0, 1, 1, np.float32([0, 2]), np.float32([[-c for c in nb[0]], nb[1]])), R(1, one), R(2, [math.sqrt(1 - float(hi) ** 2), 0, 0, float(hi)])]
    out.append(('slerp corners, nlerp', skeleton(g, 3, 'star'), 0, tr, bindings(tr), True))
    tr = [R(0, [-0.6, 0.0, 0.64, -0.48]), R(1, [0, math.sqrt(1 - float(lo) ** 2), 0, float(lo)]), R(2, [1.0, 0, 0, 0])]
    out.append(('slerp corners, theta', skeleton(g, 3, 'star'), 0, tr, bindings(tr), False))
    # a clip without tracks: the rest pose
    out.append(('rest pose', skeleton(g, 5, 'tree'), 0, [], bindings([], 2), True))
    return out

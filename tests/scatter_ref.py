'''what the scatter tests share (tests/test_scatter_cpu.py, tests/test_scatter_gpu.py): an independent numpy restatement of a scatter
as include/miptina.h defines it, written from the definition, not from scatter_rule.h.  Every value is
computed in f64 with one correctly rounded IEEE + - * / sqrt floor per written operation, in the written order, so the kernels
and mpt_scatter_rule are held to it bit for bit.  64-bit products are taken modulo 2^64 -- by numpy's uint64 arrays, which wrap,
and in mix_int by Python integers, which the CPU test holds the arrays to.

The definition, in short.  draw(i, k) = mix(mix(seed) + 16 i + k), mix SplitMix64's finaliser; unit = ((draw >> 11) + 0.5) 2^-53.
A face's weight is its world area times its density (1, or the image's channel at the mean of its corner uvs, clamped to [0, 1]);
q = floor(w / wmax 2^24); cdf the exclusive scan; instance i takes the largest face with cdf[g] <= draw(i, 0) mod T, the point
b1 = su (1 - v), b2 = su v with su = sqrt(unit 1), v = unit 2, a scale from unit 3 and a yaw from the first of eight pairs of
draws inside the unit disc.  Its matrix has the columns scale Tn, scale N, scale Bn, P, the frame made from N by the
construction of Duff et al.'''

import numpy as np

import displace_ref as dr

M64 = (1 << 64) - 1
NORMAL, UP = 0, 1
POINT = np.dtype([('face', np.int32), ('pad', np.int32), ('b1', np.float64), ('b2', np.float64), ('scale', np.float64), ('cy', np.float64),
                  ('sy', np.float64)])
SEED = 20           # (chosen on the CPU: the distribution checks of test_scatter_cpu.py pass with it; as compose_ref.GRID_SEED)
# A world matrix for the surfaces of the tests: non-uniform, sheared and -- its bottom row -- not affine.  Under an affine matrix the
# opposite faces of a centrally symmetric mesh (the octahedron) have equal areas, and w / wmax * 2^24 of the second lands within an
# ulp of 2^24: under this one no share of the tests' surfaces but the largest's own lies near an integer (test_scatter_cpu.py).
BENT = np.array([[1.7, 0.4, -0.2, 0.3], [0.1, 0.6, 0.5, -1.0], [-0.3, 0.2, 2.2, 0.5], [0.02, -0.03, 0.05, 1.0]])


# ---------------------------------------------------------------- draws
def mix_int(z):
    '''SplitMix64's finaliser on a Python integer'''
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix(z):
    '''the same on a uint64 array (its sums and products wrap)'''
    z = np.asarray(z, np.uint64)
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw(seed, i, k):
    '''draw k of the instances i (an array): uint64'''
    key = np.uint64(mix_int(int(seed) & M64))
    return mix(key + np.uint64(16) * np.asarray(i, np.uint64) + np.uint64(k))


def unit(d):
    return ((np.asarray(d, np.uint64) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


# ---------------------------------------------------------------- the surface
def world_corners(rec, world):
    '''[F,3,3] f64: the corners of the records rec [3F,8] f32 placed by the 4x4 matrix `world`, by the composition's expressions for a
    position, unrounded'''
    rec, W = np.asarray(rec), np.asarray(world, np.float64)
    assert rec.dtype == np.float32 and rec.ndim == 2 and rec.shape[1] == 8 and W.shape == (4, 4)
    p = rec[:, :3].astype(np.float64)
    ph = [((p[:, 0] * W[j, 0] + p[:, 1] * W[j, 1]) + p[:, 2] * W[j, 2]) + W[j, 3] for j in range(4)]
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.stack([ph[0] / ph[3], ph[1] / ph[3], ph[2] / ph[3]], axis=1).reshape(-1, 3, 3)


def cross(P):
    a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def length(c):
    return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def density(rec, image, channel):
    '''[F] f64: the image's channel at the mean of every face's corner uvs, clamped to [0, 1], NaN as 0'''
    uv = np.asarray(rec)[:, 6:8].astype(np.float64).reshape(-1, 3, 2)
    u = ((uv[:, 0, 0] + uv[:, 1, 0]) + uv[:, 2, 0]) / 3.0
    v = ((uv[:, 0, 1] + uv[:, 1, 1]) + uv[:, 2, 1]) / 3.0
    d = dr.height(dr.sample(image, u, v), channel)
    d = np.where(np.isnan(d), 0.0, d)
    return np.minimum(np.maximum(d, 0.0), 1.0)


def weights(P, dens=None):
    with np.errstate(invalid='ignore', over='ignore'):
        w = (0.5 * length(cross(P))) * (1.0 if dens is None else dens)
    return np.where(np.isfinite(w), w, 0.0)


def shares(w):
    '''q [F] uint32 and the values w / wmax * 2^24 they are the floors of'''
    wmax = float(np.max(w))
    assert wmax > 0
    x = w / wmax * 16777216.0
    return np.floor(x).astype(np.uint32), x


def near_boundary(x, ulps=4):
    '''which of the values w / wmax * 2^24 lie within `ulps` f64 ulps of an integer (where another order of evaluation could floor
    to the neighbour)'''
    return np.abs(x - np.rint(x)) <= ulps * np.spacing(np.maximum(np.abs(x), 1.0))


def scan(q):
    '''cdf [F + 1] uint64: the exclusive scan of q with the total behind it'''
    return np.concatenate([[0], np.cumsum(np.asarray(q, np.uint64), dtype=np.uint64)]).astype(np.uint64)


# ---------------------------------------------------------------- selection and placement
def select(cdf, seed, count, smin=1.0, smax=1.0, random_yaw=True, first=0):
    '''the sticky records [count] of instances first .. first + count - 1'''
    cdf = np.asarray(cdf, np.uint64)
    F, T = cdf.size - 1, cdf[-1]
    assert T > 0
    i = np.arange(first, first + count, dtype=np.uint64)
    out = np.zeros(count, POINT)
    t = draw(seed, i, 0) % T
    out['face'] = np.searchsorted(cdf[:F], t, side='right') - 1       # the largest g with cdf[g] <= t
    su, v = np.sqrt(unit(draw(seed, i, 1))), unit(draw(seed, i, 2))
    out['b1'] = su * (1.0 - v)
    out['b2'] = su * v
    out['scale'] = float(smin) + (float(smax) - float(smin)) * unit(draw(seed, i, 3))
    out['cy'], out['sy'] = 1.0, 0.0
    if random_yaw:
        open_ = np.ones(count, bool)
        for j in range(8):
            x, y = 2.0 * unit(draw(seed, i, 4 + 2 * j)) - 1.0, 2.0 * unit(draw(seed, i, 5 + 2 * j)) - 1.0
            r2 = x * x + y * y
            take = open_ & (r2 > 2.0 ** -20) & (r2 <= 1.0)
            ln = np.sqrt(r2[take])
            out['cy'][take], out['sy'][take] = x[take] / ln, y[take] / ln
            open_ &= ~take
    return out


def basis(N):
    '''(T0, B0) [n,3] of the unit vectors N [n,3]: Duff et al., "Building an Orthonormal Basis, Revisited"'''
    s = np.copysign(1.0, N[:, 2])
    with np.errstate(invalid='ignore', divide='ignore'):
        a = -1.0 / (s + N[:, 2])
        b = (N[:, 0] * N[:, 1]) * a
        B0 = np.stack([1.0 + (s * (N[:, 0] * N[:, 0])) * a, s * b, -(s * N[:, 0])], axis=1)
        T0 = np.stack([b, s + (N[:, 1] * N[:, 1]) * a, -N[:, 1]], axis=1)
    return T0, B0


def unit_vector(c):
    c = np.asarray(c, np.float64).reshape(-1, 3)
    with np.errstate(invalid='ignore', divide='ignore'):
        return c / length(c)[:, None]


def place(P, points, align=NORMAL, up=(0, 1, 0)):
    '''the world matrices [n,4,4] of the records `points` on the faces with world corners P [F,3,3] as they are now'''
    f = points['face']
    P0, P1, P2 = P[f, 0], P[f, 1], P[f, 2]
    b1, b2 = points['b1'][:, None], points['b2'][:, None]
    b0 = (1.0 - b1) - b2
    N = unit_vector(cross(P[f])) if align == NORMAL else np.repeat(unit_vector(up), f.size, axis=0)
    T0, B0 = basis(N)
    cy, sy, sc = points['cy'][:, None], points['sy'][:, None], points['scale'][:, None]
    with np.errstate(invalid='ignore'):
        Tn, Bn = cy * T0 + sy * B0, cy * B0 - sy * T0
        W = np.zeros((f.size, 4, 4))
        W[:, :3, 0], W[:, :3, 1], W[:, :3, 2] = sc * Tn, sc * N, sc * Bn
        W[:, :3, 3] = (b0 * P0 + b1 * P1) + b2 * P2
    W[:, 3, 3] = 1.0
    return W


def scatter(rec, world, seed, count, scale=(1.0, 1.0), align=NORMAL, up=(0, 1, 0), random_yaw=True, image=None, channel=dr.MEAN, q=None):
    '''(records, matrices, q) of a scatter over the surface records rec [3F,8] f32 placed by `world`.  q given: the selection is held
    to those shares (the device's) instead of the restatement's own'''
    P = world_corners(rec, world)
    if q is None:
        q, _ = shares(weights(P, None if image is None else density(rec, image, channel)))
    points = select(scan(q), seed, count, scale[0], scale[1], random_yaw)
    return points, place(P, points, align, up), q


def instance_primitives(mesh_rec, worlds, mtlid):
    '''the (p, n, t, w, m) tuples of the instances for multimesh.compose_multiple_meshes: the instance mesh by each matrix'''
    import deform_ref
    p, n, t = deform_ref.split(mesh_rec)
    return [(p, n, t, w, mtlid) for w in worlds]

'''
numpy restatement of the variance-guided mode of the A-Trous filter behind FilmTable.get_denoised(variance=...) (include/miptina.h,
mpt_denoise_set_variance), in the manner of tests/denoise_ref.py: one body for both precisions,
dtype=np.float64 the yardstick, dtype=np.float32 rounding after every operation in the order the HIP kernels use
(ptina_amd/csrc/denoise.hip: v_0 as ((dr dr + dg dg) + db db) (nA / nB); the prefilter's and the stencil's taps dx outer / dy
inner, both ascending; kc = 1 / (sigma_variance^2 g + 1e-10); the variance sum over (w w) v, divided by (sum w) (sum w)).
tests/test_denoise_var_cpu.py holds this file to independent statements of its properties; tests/test_denoise_var_gpu.py holds the
GPU to it.  Also here: the synthetic films both use.
'''

import numpy as np

from denoise_ref import H, MARKER, _dist2, _ratio

B = (1.0 / 4, 1.0 / 2, 1.0 / 4)


def variance0(F0, M, m, valid, T):
    '''v_0 [nx][ny]: the squared standard error of the mean of F0 from the two groups the mark M splits its samples into, over
    the demodulator m; 0 where the pixel is not valid or lacks a group'''
    nA, n = M[..., 3], F0[..., 3]
    nB = n - nA
    has = valid & (nA > 0) & (nB > 0)
    with np.errstate(all='ignore'):
        d = (F0[..., :3] / n[..., None] - M[..., :3] / nA[..., None]) / m
        v = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * (nA / nB)
        v = np.fmin(np.fmax(v, T(0)), T(np.float32(3.0e38)))
    return np.where(has, v, T(0)).astype(T)


def denoise_var_ref(F0, F1, F2, M, nx, ny, sigma_variance, iterations=5, sigma_color=1.0, sigma_albedo=0.1, sigma_normal=0.3,
                    demodulate=True, dtype=np.float64):
    '''F0, F1, F2, M: the raw accumulators of passes 0, 1, 2 and of the mark ([nx*ny][4], element x*ny + y).  Returns (the image
    [nx][ny][4], v_final [nx][ny]) of `dtype`; iterations = 0 gives the resolved image and v_0.  The sigmas are taken as the f32
    values the C ABI receives; sigma_color is not used.'''
    T = np.dtype(dtype).type
    F0, F1, F2, M = (np.asarray(F).reshape(nx, ny, 4).astype(T) for F in (F0, F1, F2, M))
    c, valid = _ratio(F0, T)
    a, _ = _ratio(F1, T)
    n, _ = _ratio(F2, T)
    out = np.empty((nx, ny, 4), T)
    out[...] = np.array(MARKER, np.float32).astype(T)
    m = np.maximum(a, T(np.float32(1e-2))) if demodulate else np.ones_like(a)
    v = variance0(F0, M, m, valid, T)
    if iterations == 0:
        out[valid, :3] = c[valid]
        out[valid, 3] = 1
        return out, v
    e = np.zeros_like(c)
    e[valid] = (c / m)[valid] if demodulate else c[valid]
    sv, sa, sn = (T(np.float32(s)) for s in (sigma_variance, sigma_albedo, sigma_normal))
    sv2, ka, kn = sv * sv, T(1) / (sa * sa), T(1) / (sn * sn)
    h, b = [T(x) for x in H], [T(x) for x in B]
    for i in range(iterations):
        s = 1 << i
        R = 2 * s

        def pad(x, r):
            return np.pad(x, ((r, r), (r, r)) + ((0, 0),) * (x.ndim - 2))
        # the colour tolerance of every pixel from the variance around it
        v1, ok1 = pad(v, 1), pad(valid, 1)
        num, den = np.zeros((nx, ny), T), np.zeros((nx, ny), T)
        for dx in range(3):
            for dy in range(3):
                sl = (slice(dx, dx + nx), slice(dy, dy + ny))
                num += np.where(ok1[sl], (b[dx] * b[dy]) * v1[sl], T(0))
                den += np.where(ok1[sl], b[dx] * b[dy], T(0))
        with np.errstate(all='ignore'):
            kc = np.where(valid, T(1) / (sv2 * (num / den) + T(np.float32(1e-10))), T(0)).astype(T)
        ep, ap, np_, okp, vp = pad(e, R), pad(a, R), pad(n, R), pad(valid, R), pad(v, R)
        sw, sv_ = np.zeros((nx, ny), T), np.zeros((nx, ny), T)
        se = np.zeros((nx, ny, 3), T)
        for dx in range(5):
            for dy in range(5):
                ox, oy = R + (dx - 2) * s, R + (dy - 2) * s
                sl = (slice(ox, ox + nx), slice(oy, oy + ny))
                eq, aq, nq, ok = ep[sl], ap[sl], np_[sl], okp[sl]
                with np.errstate(all='ignore'):
                    arg = (_dist2(e, eq) * kc + _dist2(a, aq) * ka) + _dist2(n, nq) * kn
                    w = np.where(ok & valid, (h[dx] * h[dy]) * np.exp(-arg), T(0)).astype(T)
                    sw += w
                    se += w[..., None] * eq
                    sv_ += (w * w) * vp[sl]
        nxt, nv = np.zeros_like(e), np.zeros_like(v)
        nxt[valid] = se[valid] / sw[valid][:, None]
        nv[valid] = sv_[valid] / (sw[valid] * sw[valid])
        e, v = nxt, nv
    out[valid, :3] = (e * m)[valid] if demodulate else e[valid]
    out[valid, 3] = 1
    return out, v


# ---------------------------------------------------------------- synthetic films
def random_film(seed, nx, ny, broken=0.2):
    '''(F0, F1, F2, M) f32 [nx*ny][4] for the parity tests: a smooth colour field with a step the guides do not see, gamma noise of
    a relative size that varies over the film in two groups of nA and nB in {1, 2, 4, 8, 3} samples, smooth albedo with one edge,
    normals of two orientations; of a share `broken` of the pixels a quarter each is not valid (F0.w = 0), has nA = 0, has nB = 0,
    or has an empty guide pass'''
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    L = (0.5 + 0.4 * np.sin(0.37 * x + 0.2) * np.cos(0.23 * y)) * np.where(x + 2 * y > (nx + 2 * ny) * 0.55, 0.3, 1.0)
    truth = L[..., None] * np.array([1.0, 0.8, 0.6])
    rel = np.exp(rng.uniform(np.log(0.02), np.log(1.5), (nx, ny, 1)))
    k = 1.0 / rel ** 2
    nA = rng.choice([1.0, 2.0, 4.0, 8.0, 3.0], (nx, ny))
    nB = rng.choice([1.0, 2.0, 4.0, 8.0, 3.0], (nx, ny))
    A = truth * rng.gamma(nA[..., None] * k * np.ones(3)) / k
    Bs = truth * rng.gamma(nB[..., None] * k * np.ones(3)) / k
    kind = np.where(rng.random((nx, ny)) < broken, rng.integers(1, 5, (nx, ny)), 0)
    alb = np.where((y > ny * 0.4)[..., None], [0.7, 0.6, 0.5], [0.2, 0.5, 0.004]) * (1 + 0.05 * np.sin(0.5 * x))[..., None]
    nrm = np.where((x > nx * 0.6)[..., None], [0.0, 0.6, 0.8], [0.0, 0.0, 1.0])
    F0, F1, F2, M = (np.zeros((nx, ny, 4), np.float32) for _ in range(4))
    nA = np.where(kind == 2, 0.0, nA)
    nB = np.where(kind == 3, 0.0, nB)
    M[..., :3], M[..., 3] = A * (nA > 0)[..., None], nA
    F0[..., :3] = M[..., :3].astype(np.float64) + Bs * (nB > 0)[..., None]
    F0[..., 3] = nA + nB
    F0[kind == 1] = [3.0, 2.0, 1.0, 0.0]                 # (not valid whatever the sums hold; the mark keeps its samples)
    F1[..., :3], F1[..., 3] = alb * 2, 2
    F2[..., :3], F2[..., 3] = nrm * 2, 2
    F1[kind == 4] = 0
    F2[kind == 4] = 0
    return tuple(F.reshape(-1, 4) for F in (F0, F1, F2, M))


QUALITY_N = 96


def quality_film(seed):
    '''The film of the quality claim: 96x96, two groups of 16 samples with gamma-distributed noise of
    exact mean, flat albedo and normal.  A smooth field, cut by a shadow edge the guides cannot see (y > x / 2 + 30 is in shadow);
    relative noise per sample 1.5 in the left half and 0.5 in the right one; in the right half a band (x in 56..87, y in 8..23) of
    illumination stripes 2 pixels wide at relative noise 0.05.  Returns (F0, F1, F2, M, truth [96][96][3], regions: name -> mask)'''
    N = QUALITY_N
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    L = 0.45 + 0.15 * np.sin(2 * np.pi * x / N) * np.cos(2 * np.pi * y / N)
    edge = y - (0.5 * x + 30)
    L = L * np.where(edge > 0, 0.35, 1.0)
    band = (x >= 56) & (x < 88) & (y >= 8) & (y < 24)
    L = np.where(band, 0.34 * np.where((x // 2) % 2 == 0, 1.2, 0.8), L)
    truth = L[..., None] * np.array([1.0, 0.9, 0.8])
    rel = np.where(band, 0.05, np.where(x < N // 2, 1.5, 0.5))[..., None]
    k = 1.0 / rel ** 2
    A = truth * rng.gamma(16 * k * np.ones(3)) / k
    Bs = truth * rng.gamma(16 * k * np.ones(3)) / k
    F0, F1, F2, M = (np.zeros((N, N, 4), np.float32) for _ in range(4))
    M[..., :3], M[..., 3] = A, 16
    F0[..., :3], F0[..., 3] = A + Bs, 32
    F1[...] = [0.5, 0.5, 0.5, 1.0]
    F2[...] = [0.0, 0.0, 1.0, 1.0]
    regions = {'whole': np.ones((N, N), bool), 'stripes': band, 'noisiest': (x < N // 2) & (np.abs(edge) > 2),
               'edge': (np.abs(edge) <= 2) & ~band}
    return tuple(F.reshape(-1, 4) for F in (F0, F1, F2, M)) + (truth, regions)

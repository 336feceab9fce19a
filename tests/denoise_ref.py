'''
numpy restatement of the edge-avoiding A-Trous filter behind FilmTable.get_denoised (include/miptina.h, mpt_get_denoised;
DESIGN.md section 3.9), vectorised over the 25 shifted slices of the film.  One body for both precisions: dtype=np.float64 is the
yardstick, dtype=np.float32 rounds after every operation in the order the HIP kernels use (ptina_amd/csrc/denoise.hip: taps
dx outer / dy inner, both ascending; |d|^2 = (dx dx + dy dy) + dz dz; the exponent (colour + albedo) + normal), so that
|ref32 - ref64| is what f32 arithmetic alone does to this filter on a given film.  tests/test_denoise_cpu.py holds this file to
independent statements of its properties.
'''

import numpy as np

H = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
MARKER = (0.9, 0.4, 0.9, 0.0)             # FilmTable.get_image's empty pixel
DEFAULTS = dict(iterations=5, sigma_color=1.0, sigma_albedo=0.1, sigma_normal=0.3, demodulate=True)


def _dist2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _ratio(F, T):
    '''rgb / w where w != 0, else 0'''
    w = F[..., 3]
    ok = w != 0
    out = np.zeros(F.shape[:-1] + (3,), T)
    out[ok] = F[ok][:, :3] / F[ok][:, 3:4]
    return out, ok


def denoise_ref(F0, F1, F2, nx, ny, iterations=5, sigma_color=1.0, sigma_albedo=0.1, sigma_normal=0.3, demodulate=True,
                dtype=np.float64):
    '''F0, F1, F2: the raw accumulators of passes 0, 1, 2 ([nx*ny][4], element x*ny + y).  Returns [nx][ny][4] of `dtype`.
    The sigmas are taken as the f32 values the C ABI receives.'''
    T = np.dtype(dtype).type
    F0, F1, F2 = (np.asarray(F).reshape(nx, ny, 4).astype(T) for F in (F0, F1, F2))
    c, valid = _ratio(F0, T)
    a, _ = _ratio(F1, T)
    n, _ = _ratio(F2, T)
    out = np.empty((nx, ny, 4), T)
    out[...] = np.array(MARKER, np.float32).astype(T)
    if iterations == 0:
        out[valid, :3] = c[valid]
        out[valid, 3] = 1
        return out
    m = np.maximum(a, T(np.float32(1e-2))) if demodulate else np.ones_like(a)
    e = np.zeros_like(c)
    e[valid] = (c / m)[valid] if demodulate else c[valid]
    sc, sa, sn = (T(np.float32(s)) for s in (sigma_color, sigma_albedo, sigma_normal))
    ka, kn = T(1) / (sa * sa), T(1) / (sn * sn)
    h = [T(x) for x in H]
    for i in range(iterations):
        s = 1 << i
        R = 2 * s
        sci = sc * T(2.0 ** -i)
        kc = T(1) / (sci * sci)

        def pad(v):
            return np.pad(v, ((R, R), (R, R)) + ((0, 0),) * (v.ndim - 2))
        ep, ap, np_, vp = pad(e), pad(a), pad(n), pad(valid)
        sw = np.zeros((nx, ny), T)
        se = np.zeros((nx, ny, 3), T)
        for dx in range(5):
            for dy in range(5):
                ox, oy = R + (dx - 2) * s, R + (dy - 2) * s
                sl = (slice(ox, ox + nx), slice(oy, oy + ny))
                eq, aq, nq, ok = ep[sl], ap[sl], np_[sl], vp[sl]
                arg = (_dist2(e, eq) * kc + _dist2(a, aq) * ka) + _dist2(n, nq) * kn
                with np.errstate(over='ignore', under='ignore'):
                    w = np.where(ok, (h[dx] * h[dy]) * np.exp(-arg), T(0)).astype(T)
                sw += w
                se += w[..., None] * eq
        nxt = np.zeros_like(e)
        nxt[valid] = se[valid] / sw[valid][:, None]
        e = nxt
    out[valid, :3] = (e * m)[valid] if demodulate else e[valid]
    out[valid, 3] = 1
    return out

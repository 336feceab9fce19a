'''
numpy restatement of FilmTable.get_display (include/miptina.h, mpt_get_display): sanitise, meter, expose,
tone-map, transfer, dither, quantise.  One body for both precisions: dtype=np.float64 is the yardstick, dtype=np.float32 rounds
after every operation as the HIP code does (ptina_amd/csrc/display.hip), except where the definition itself says f64 -- the metering's
logarithms, their sum and the exposure's last steps.  tests/test_display_cpu.py holds this file to closed forms, and
tests/test_display_gpu.py holds the GPU to it by the byte rule below.
'''

import numpy as np

MARKER8 = (230, 102, 230, 0)                # get_image's empty pixel (0.9, 0.4, 0.9, 0) at 8 bits
OPS = ('linear', 'ptina', 'reinhard', 'aces')
TRANSFERS = ('srgb', 'gamma')
DEFAULTS = dict(op='aces', transfer='srgb', dither=True, exposure=None, key=0.18, white=4.0, gamma=2.2)
V_MAX = 1e18


def bayer(x, y):
    '''the 8x8 Bayer index of (x & 7, y & 7), as the header spells it'''
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    m = np.zeros(np.broadcast(x, y).shape, np.int64)
    for i in range(3):
        m |= ((((x ^ y) >> i) & 1) << (2 * (2 - i) + 1)) | (((y >> i) & 1) << (2 * (2 - i)))
    return m


def sanitise(c, T=np.float64):
    '''fminf(fmaxf(c, 0), 3e38): NaN -> 0, negative -> 0, +inf -> 3e38 (np.fmax / np.fmin return the argument that is not NaN)'''
    return np.fmin(np.fmax(np.asarray(c, T), T(0)), T(3.0e38))


def luminance(c, T=np.float64):
    return (T(0.2126) * c[..., 0] + T(0.7152) * c[..., 1]) + T(0.0722) * c[..., 2]


def exposure_of(c, valid, key=0.18, T=np.float64):
    '''key / exp(mean log(1e-4 + Y)) over the valid pixels, 1 without any: 1e-4 + Y in T, the rest in f64, rounded to T once'''
    n = int(valid.sum())
    if n == 0:
        return T(1)
    with np.errstate(over='ignore'):
        terms = np.log((T(1e-4) + luminance(c[valid], T)).astype(np.float64))
    lavg = np.exp(terms.sum() / n)
    return T(np.float64(np.float32(key)) / lavg)


def tone(v, op, white=4.0, T=np.float64):
    '''the operator and its clamp to 0..1; v already exposed'''
    v = np.asarray(v, T)
    with np.errstate(over='ignore', invalid='ignore'):
        if op == 'linear':
            t = v
        elif op == 'ptina':
            t = v / (v + T(0.155)) * T(1.019)
        elif op == 'reinhard':
            w = T(np.float32(white))
            t = v * (T(1) + v / (w * w)) / (T(1) + v)
        elif op == 'aces':
            t = v * (T(2.51) * v + T(0.03)) / (v * (T(2.43) * v + T(0.59)) + T(0.14))
        else:
            raise ValueError(op)
    return np.fmin(np.fmax(t, T(0)), T(1))


def transfer_curve(t, transfer, gamma=2.2, T=np.float64):
    t = np.asarray(t, T)
    if transfer == 'srgb':
        return np.where(t <= T(0.0031308), T(12.92) * t, T(1.055) * np.power(t, T(1) / T(2.4)) - T(0.055)).astype(T)
    if transfer == 'gamma':
        return np.power(t, T(1) / T(np.float32(gamma)))
    raise ValueError(transfer)


def display_ref(raw, nx, ny, op='aces', transfer='srgb', dither=True, exposure=None, key=0.18, white=4.0, gamma=2.2, dtype=np.float64):
    '''raw: accumulators [nx*ny][4] (element x*ny + y).  Returns (u, bytes, valid, E): u [nx][ny][3] of `dtype` = 255 s + B, the
    value in front of the floor; bytes [nx][ny][4] uint8 in the FILM layout; valid [nx][ny]; E the exposure used (of `dtype`).
    The parameters are taken as the f32 values the C ABI receives.'''
    T = np.dtype(dtype).type
    F = np.asarray(raw, np.float32).reshape(nx, ny, 4).astype(T)
    valid = F[..., 3] != 0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        c = sanitise(F[..., :3] / F[..., 3:4], T)
    E = exposure_of(c, valid, key, T) if not exposure else T(np.float32(exposure))
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.fmin(E * c, T(V_MAX))
    s = transfer_curve(tone(v, op, white, T), transfer, gamma, T)
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    B = ((bayer(xs, ys).astype(T) + T(0.5)) / T(64)) if dither else np.full((nx, ny), T(0.5))
    u = (T(255) * s + B[..., None]).astype(T)
    out = np.empty((nx, ny, 4), np.uint8)
    out[...] = MARKER8
    q = np.clip(np.floor(u), 0, 255).astype(np.uint8)
    out[valid, :3] = q[valid]
    out[valid, 3] = 255
    return u, out, valid, E


def display_layout(film_layout):
    '''[nx][ny][4] -> [ny][nx][4], rows top-down: what ti.imwrite builds'''
    return np.ascontiguousarray(np.swapaxes(film_layout, 0, 1)[::-1])


def byte_rule(got, raw, nx, ny, **kw):
    '''The byte rule: with u64 the f64 restatement's value in front of the floor, a byte must be floor(u64) (clamped); where u64
    lies within tau of an integer either neighbour passes, never more than 1 off.  tau = 8 d, d = max |u32 - u64| of the f32
    restatement on the same film, in byte units (two independent f32 roundings, pow / log / exp implementations an ulp or two
    apart, the reduction's order).  `got`: [nx][ny][4] uint8, FILM layout.
    Returns dict(d, tau, excused, colour_bytes, bad, worst): excused = bytes that differ from floor(u64) and pass by the rule;
    bad = bytes outside the rule; invalid pixels must be the marker and valid alpha 255 (counted in bad).'''
    u64, b64, valid, E64 = display_ref(raw, nx, ny, dtype=np.float64, **kw)
    u32, b32, _, E32 = display_ref(raw, nx, ny, dtype=np.float32, **kw)
    got = np.asarray(got)
    assert got.shape == (nx, ny, 4) and got.dtype == np.uint8
    nvalid = int(valid.sum())
    d = float(np.abs(u32[valid].astype(np.float64) - u64[valid]).max()) if nvalid else 0.0
    tau = 8 * d
    lo = np.clip(np.floor(u64 - tau), 0, 255).astype(np.int64)
    hi = np.clip(np.floor(u64 + tau), 0, 255).astype(np.int64)
    g = got[..., :3].astype(np.int64)
    want = b64[..., :3].astype(np.int64)
    inside = ((g == lo) | (g == hi)) & (np.abs(g - want) <= 1)
    bad = int((~inside[valid]).sum())
    bad += int((got[~valid] != np.uint8(MARKER8)).any(axis=-1).sum()) + int((got[valid][:, 3] != 255).sum())
    excused = int(((g != want) & inside)[valid].sum())
    return dict(d=d, tau=tau, excused=excused, colour_bytes=3 * nvalid, bad=bad, E64=float(E64), E32=float(E32),
                worst=int(np.abs(g - want)[valid].max()) if nvalid else 0)


def synthetic_film(seed, nx, ny, invalid=0.25):
    '''accumulators with colours log-uniform over 1e-6 .. 1e4 and mixed weights: w in {1, 2, 3, 4, 0.5, 7} and, for a share
    `invalid` of the pixels, 0'''
    rng = np.random.default_rng(seed)
    n = nx * ny
    w = rng.choice(np.float32([1, 2, 3, 4, 0.5, 7]), n)
    c = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), (n, 3)))
    F = np.empty((n, 4), np.float32)
    F[:, :3] = c * w[:, None]
    F[:, 3] = w
    F[rng.random(n) < invalid] = 0
    return F

'''
CPU tests of tests/denoise_var_ref.py, the numpy restatement of the variance-guided A-Trous filter that
tests/test_denoise_var_gpu.py holds FilmTable.get_denoised(variance=...) to: each property of the definition (include/miptina.h,
mpt_denoise_set_variance) is checked against a statement of it that shares no code with the restatement; then the claim the mode
is built on -- that it filters better than the fixed sigma_color -- on a synthetic film whose truth is known; then the header's
prototypes against the ctypes table.
'''

import os
import re

import numpy as np
import pytest

import noise_ref
from denoise_ref import denoise_ref, MARKER, H
from denoise_var_ref import denoise_var_ref, quality_film, random_film, QUALITY_N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat(nx, ny, rgbw):
    return np.tile(np.float32(rgbw), (nx * ny, 1))


def _noisy(rng, nx, ny, nA=4, nB=4, lo=0.1, hi=1.0):
    '''(F0, M): two groups of samples scattered around a random colour in [lo, hi)'''
    c = rng.uniform(lo, hi, (nx * ny, 3))
    M = np.empty((nx * ny, 4), np.float32)
    M[:, :3], M[:, 3] = c * rng.uniform(0.5, 1.5, (nx * ny, 3)) * nA, nA
    F0 = np.empty_like(M)
    F0[:, :3], F0[:, 3] = M[:, :3] + c * rng.uniform(0.5, 1.5, (nx * ny, 3)) * nB, nA + nB
    return F0, M


# ---------------------------------------------------------------- 1. the variance is the noise estimate's
def test_v0_is_the_noise_estimates_standard_error_squared():
    '''m = 1 (no demodulation): v_0 = sum over the channels of noise_ref's d^2, d = |m - a| sqrt(nA / nB); the two differ by the
    rounding of the square root and of four more operations: a few f32 ulp'''
    nx, ny = 31, 17
    F, M = noise_ref.synthetic_pair(11, nx, ny)
    _, v0 = denoise_var_ref(F, _flat(nx, ny, [1, 1, 1, 1]), _flat(nx, ny, [0, 0, 1, 1]), M, nx, ny, 4.0, iterations=0, demodulate=False,
                            dtype=np.float32)
    assert v0.dtype == np.float32 and v0.shape == (nx, ny)
    nA, n = M[:, 3], F[:, 3]
    with np.errstate(all='ignore'):
        d = np.abs(noise_ref.clamp0(F[:, :3] / n[:, None]) - noise_ref.clamp0(M[:, :3] / nA[:, None])) * noise_ref.noise_k(nA, n - nA)[:, None]
    _, valid = noise_ref.noise_map(F, M)
    want = np.where(valid, (d.astype(np.float64) ** 2).sum(axis=1), 0.0)
    assert valid.sum() > 0.7 * nx * ny and (~valid).sum() > 20
    assert np.allclose(v0.reshape(-1), want, rtol=2e-6, atol=0)
    assert np.all(v0.reshape(-1)[~valid] == 0)


def test_pixels_without_two_groups_carry_no_variance_and_stay_valid():
    rng = np.random.default_rng(12)
    nx, ny = 9, 8
    F0, M = _noisy(rng, nx, ny)
    M[5] = [0, 0, 0, 0]                      # nA = 0
    M[6] = F0[6]                             # nB = 0
    M[7, 3] = F0[7, 3] + 1                   # nB < 0
    img, v = denoise_var_ref(F0, _flat(nx, ny, [1, 1, 1, 2]), _flat(nx, ny, [0, 0, 1, 1]), M, nx, ny, 4.0, iterations=0)
    assert np.all(v.reshape(-1)[[5, 6, 7]] == 0) and np.all(np.delete(v.reshape(-1), [5, 6, 7]) > 0)
    assert np.all(img[..., 3] == 1)
    img, v = denoise_var_ref(F0, _flat(nx, ny, [1, 1, 1, 2]), _flat(nx, ny, [0, 0, 1, 1]), M, nx, ny, 4.0, iterations=2)
    assert np.all(img[..., 3] == 1) and np.isfinite(img).all() and np.isfinite(v).all()


# ---------------------------------------------------------------- 2. no evidence of noise, no filtering
@pytest.mark.parametrize('demodulate', [True, False])
def test_a_film_whose_groups_agree_comes_back_unchanged(demodulate):
    '''M = F0 / 2 exactly: both groups have the same mean, v_0 = 0 everywhere, kc = 1e10, and a neighbour whose colour differs by
    more than 1e-4 weighs less than exp(-100): the film's pixels all differ by more (uniform colours; the closest pair of the
    film is checked), so every pixel keeps its value'''
    rng = np.random.default_rng(13)
    nx, ny = 23, 19
    F0 = np.empty((nx * ny, 4), np.float32)
    F0[:, :3], F0[:, 3] = rng.uniform(0.5, 8.0, (nx * ny, 3)), 8
    M = (F0 / 2).astype(np.float32)
    c = F0[:, :3].astype(np.float64) / 8
    F1 = _flat(nx, ny, [0.5, 0.25, 1.0, 1.0])
    closest = min(np.sqrt(((c[i + 1:] - c[i]) ** 2).sum(axis=1)).min() for i in range(nx * ny - 1))
    assert closest > 4e-4                    # demodulated by at most 1: the distances only grow
    img, v = denoise_var_ref(F0, F1, _flat(nx, ny, [0, 0, 1, 1]), M, nx, ny, 4.0, demodulate=demodulate)
    assert np.all(v == 0)
    assert np.abs(img[..., :3].reshape(-1, 3) - c).max() < 1e-12


# ---------------------------------------------------------------- 3. the variance of a weighted mean
def test_constant_film_constant_variance_one_iteration():
    '''every colour weight is 1, so w = h h over the taps inside the film and v' = v sum (h h)^2 / (sum h h)^2, written here as
    loops over the taps of every pixel'''
    nx, ny = 7, 6
    F0 = _flat(nx, ny, [4.0, 2.0, 1.0, 8.0])                     # mean (0.5, 0.25, 0.125)
    M = _flat(nx, ny, [3.0, 1.0, 0.5, 4.0])                      # group A mean (0.75, 0.25, 0.125): d = (-0.25, 0, 0), nA / nB = 1
    img, v = denoise_var_ref(F0, _flat(nx, ny, [1, 1, 1, 1]), _flat(nx, ny, [0, 0, 1, 1]), M, nx, ny, 4.0, iterations=1, demodulate=False)
    assert np.allclose(img[..., :3], [0.5, 0.25, 0.125], rtol=1e-14, atol=0)
    v0 = 0.0625
    for x in range(nx):
        for y in range(ny):
            s1 = s2 = 0.0
            for dx in range(-2, 3):
                for dy in range(-2, 3):
                    if 0 <= x + dx < nx and 0 <= y + dy < ny:
                        s1 += H[dx + 2] * H[dy + 2]
                        s2 += (H[dx + 2] * H[dy + 2]) ** 2
            assert abs(v[x, y] - v0 * s2 / s1 ** 2) < 1e-15
    assert v[3, 3] < 0.08 * v0 and v[0, 0] > v[3, 3]              # an interior pixel averages 25 taps: sum h^4 = (35 / 128)^2


# ---------------------------------------------------------------- 4. what is not valid neither gives nor receives
def test_an_invalid_pixel_neither_gives_nor_receives():
    rng = np.random.default_rng(14)
    nx, ny = 11, 14
    F0, M = _noisy(rng, nx, ny)
    F1, F2 = _flat(nx, ny, [1, 0.5, 0.25, 1]), _flat(nx, ny, [0, 0, 1, 1])
    hole = 5 * ny + 6
    F0[hole] = [3.0, 2.0, 1.0, 0.0]
    G0, N = F0.copy(), M.copy()
    G0[hole, :3] = [-50.0, 1e6, 7.0]
    N[hole] = [1e3, 0.0, 5.0, 0.0]
    for dtype in (np.float64, np.float32):
        a, va = denoise_var_ref(F0, F1, F2, M, nx, ny, 4.0, dtype=dtype)
        b, vb = denoise_var_ref(G0, F1, F2, N, nx, ny, 4.0, dtype=dtype)
        assert a.dtype == dtype and va.dtype == dtype
        assert np.array_equal(a[5, 6], np.array(MARKER, np.float32).astype(dtype)) and va[5, 6] == 0
        assert np.array_equal(a, b) and np.array_equal(va, vb)


def test_invalid_columns_are_as_good_as_the_films_border():
    '''columns [8, 20) of a 28-column film valid, the rest not: the valid part filters exactly as a film of its own -- in the
    stencil and in the prefilter, whose denominator counts valid taps only'''
    nx, ny = 28, 13
    F0, F1, F2, M = (F.reshape(nx, ny, 4).copy() for F in random_film(15, nx, ny, broken=0.0))
    F0[:8, :, 3] = 0
    F0[20:, :, 3] = 0
    whole, vw = denoise_var_ref(*(F.reshape(-1, 4) for F in (F0, F1, F2, M)), nx, ny, 4.0)
    alone, va = denoise_var_ref(*(F[8:20].reshape(-1, 4) for F in (F0, F1, F2, M)), 12, ny, 4.0)
    assert np.array_equal(whole[8:20], alone) and np.array_equal(vw[8:20], va)
    assert np.all(vw[:8] == 0) and np.all(vw[20:] == 0) and np.all(whole[:8] == np.float32(MARKER))


# ---------------------------------------------------------------- 5. the limit is the fixed filter's limit
@pytest.mark.parametrize('demodulate', [True, False])
def test_wide_sigma_variance_is_the_fixed_filter_with_wide_sigma_color(demodulate):
    '''sigma_variance = 1e15 on a film with v_0 > 0 everywhere: kc = 1 / (1e30 g) with g above 1e-8 here, the colour term below
    1e-20: the weights are the fixed filter's at sigma_color = 1e15 (colour term below 1e-26) to far inside 1e-12'''
    rng = np.random.default_rng(16)
    nx, ny = 21, 17
    F0, M = _noisy(rng, nx, ny)
    F1 = np.empty_like(F0)
    F1[:, :3], F1[:, 3] = rng.uniform(0.3, 0.5, (nx * ny, 3)), 1
    F2 = np.empty_like(F0)
    F2[:, :3], F2[:, 3] = rng.uniform(-0.2, 0.2, (nx * ny, 3)), 1
    _, v0 = denoise_var_ref(F0, F1, F2, M, nx, ny, 1e15, iterations=0, demodulate=demodulate)
    assert v0.min() > 1e-8
    kw = dict(iterations=4, sigma_albedo=0.3, sigma_normal=0.5, demodulate=demodulate)
    got, _ = denoise_var_ref(F0, F1, F2, M, nx, ny, 1e15, **kw)
    want = denoise_ref(F0, F1, F2, nx, ny, sigma_color=1e15, **kw)
    assert np.abs(got - want).max() < 1e-12
    narrow = denoise_ref(F0, F1, F2, nx, ny, sigma_color=0.05, **kw)
    assert np.abs(narrow - want).max() > 1e-3                    # (the colour term does matter on this film)


def test_f32_restatement_stays_close_to_f64():
    nx, ny = 21, 17
    film = random_film(17, nx, ny)
    a, va = denoise_var_ref(*film, nx, ny, 4.0, dtype=np.float64)
    b, vb = denoise_var_ref(*film, nx, ny, 4.0, dtype=np.float32)
    assert b.dtype == np.float32 and vb.dtype == np.float32
    assert (np.abs(b - a) / (1 + np.abs(a))).max() < 1e-4
    assert (np.abs(vb - va) / (np.median(va[va > 0]) + np.abs(va))).max() < 1e-3


# ---------------------------------------------------------------- 6. it filters better
@pytest.mark.parametrize('seed', [1, 2, 3, 4, 5, 6])
def test_guided_filter_beats_the_fixed_one_on_the_synthetic_film(seed):
    '''RMSE against the truth, variance-guided at sigma_variance = 4 over the fixed filter at its defaults, f64: the whole film
    <= 0.6, the stripe band <= 0.15, the noisiest region <= 1.0, the shadow-edge band <= 1.0.  Measured with this restatement over
    the six seeds: 0.36-0.40, 0.027-0.038, 0.66-0.73, 0.76-0.85'''
    N = QUALITY_N
    F0, F1, F2, M, truth, regions = quality_film(seed)
    fixed = denoise_ref(F0, F1, F2, N, N)
    guided, _ = denoise_var_ref(F0, F1, F2, M, N, N, 4.0)
    plain = denoise_ref(F0, F1, F2, N, N, iterations=0)

    def rmse(img, mask):
        return float(np.sqrt(((img[..., :3] - truth)[mask] ** 2).mean()))
    ratio = {k: rmse(guided, m) / rmse(fixed, m) for k, m in regions.items()}
    print(f'seed {seed}: guided / fixed RMSE ' + ', '.join(f'{k} {r:.3f}' for k, r in ratio.items()) +
          f'; stripe band: plain {rmse(plain, regions["stripes"]):.4f}, fixed {rmse(fixed, regions["stripes"]):.4f}, '
          f'guided {rmse(guided, regions["stripes"]):.4f}')
    assert all(m.sum() > 300 for m in regions.values())
    assert ratio['whole'] <= 0.6
    assert ratio['stripes'] <= 0.15
    assert ratio['noisiest'] <= 1.0
    assert ratio['edge'] <= 1.0
    # what the mode is for: the fixed filter wipes the stripes out, the guided one keeps them
    assert rmse(fixed, regions['stripes']) > 10 * rmse(plain, regions['stripes'])
    assert rmse(guided, regions['stripes']) < rmse(plain, regions['stripes'])


# ---------------------------------------------------------------- 7. the ABI
def test_header_prototypes_match_the_ctypes_table():
    import ctypes as C
    from ptina_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'miptina.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    ctype = {'mpt_ctx *': C.c_void_p, 'float': C.c_float, 'float *': _lib._fp, 'const float *': _lib._fp, 'int': C.c_int,
             'const mpt_denoise_params *': C.POINTER(_lib.DenoiseParams)}
    for name in ('mpt_denoise_set_variance', 'mpt_denoise_get_variance', 'mpt_denoise_eval'):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, f'{name} is not declared'
        args = []
        for a in m.group(1).split(','):
            t = re.sub(r'\s+', ' ', re.sub(r'\w+\s*$', '', a.strip())).strip()      # drop the parameter's name
            args.append(ctype[t])
        res, want = _lib.SIGNATURES[name]
        assert res is C.c_int and want == args, name
    assert C.sizeof(_lib.DenoiseParams) == 20                    # the mode is context state: the struct did not grow

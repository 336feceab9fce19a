'''
CPU tests of tests/denoise_ref.py, the numpy restatement of the A-Trous filter that tests/test_denoise_gpu.py holds
FilmTable.get_denoised to: each property of the definition (include/miptina.h, mpt_get_denoised) is checked here against a
statement of it that shares no code with the restatement, so that the restatement can be trusted as the GPU's yardstick.
'''

import numpy as np
import pytest

from denoise_ref import denoise_ref, MARKER


def _film(rng, nx, ny, lo=0.0, hi=1.0, spp=4):
    '''raw accumulators [nx*ny][4]: rgb sums of `spp` samples in [lo, hi), w = spp'''
    F = np.empty((nx * ny, 4), np.float32)
    F[:, :3] = rng.uniform(lo, hi, (nx * ny, 3)) * spp
    F[:, 3] = spp
    return F


def _empty(nx, ny):
    return np.zeros((nx * ny, 4), np.float32)


@pytest.mark.parametrize('sigmas', [(1.0, 0.1, 0.3), (1e-3, 1e-3, 1e-3), (1e6, 1e6, 1e6)])
@pytest.mark.parametrize('demodulate', [True, False])
def test_constant_film_stays_constant(sigmas, demodulate):
    nx, ny = 13, 9
    F0 = np.tile(np.float32([2.0, 1.0, 0.5, 4.0]), (nx * ny, 1))
    F1 = np.tile(np.float32([0.5, 0.25, 1.0, 2.0]), (nx * ny, 1))          # albedo (0.25, 0.125, 0.5): exact in f32
    F2 = np.tile(np.float32([0.0, 0.0, 2.0, 2.0]), (nx * ny, 1))
    out = denoise_ref(F0, F1, F2, nx, ny, 5, *sigmas, demodulate=demodulate)
    assert np.allclose(out[..., :3], [0.5, 0.25, 0.125], rtol=1e-14, atol=0) and np.all(out[..., 3] == 1)


def _b3_atrous_separable(img, iterations):
    '''plain B3-spline A-Trous smoothing, written on its own: per iteration a 1-D pass along y, then one along x, every output
    divided by the sum of the taps that fell inside the film (the rectangle's inside mask is separable, so this is the 2-D
    renormalised filter)'''
    h = np.array([1, 4, 6, 4, 1], np.float64) / 16

    def pass_1d(v, axis, s):
        v = np.moveaxis(v, axis, 0)
        n = v.shape[0]
        num, den = np.zeros_like(v), np.zeros(n)
        for k in range(5):
            for j in range(n):
                q = j + (k - 2) * s
                if 0 <= q < n:
                    num[j] += h[k] * v[q]
                    den[j] += h[k]
        return np.moveaxis(num / den.reshape((n,) + (1,) * (v.ndim - 1)), 0, axis)

    for i in range(iterations):
        img = pass_1d(pass_1d(img, 1, 1 << i), 0, 1 << i)
    return img


def test_wide_sigmas_give_the_plain_b3_spline_atrous():
    '''All sigmas 1e6, no demodulation: every edge-stopping weight is 1 up to exp(-|d|^2 / (1e6 2^-i)^2).  The colours span 0.01,
    so that exponent is below 3e-4 / (1e6 / 16)^2 = 8e-14 at the last iteration: far inside the 1e-12 the comparison is held to.'''
    rng = np.random.default_rng(1)
    nx, ny = 37, 29
    F0 = _film(rng, nx, ny, 0.5, 0.51)
    got = denoise_ref(F0, _film(rng, nx, ny), _film(rng, nx, ny), nx, ny, 5, 1e6, 1e6, 1e6, demodulate=False)
    c = (F0[:, :3].astype(np.float64) / F0[:, 3:4]).reshape(nx, ny, 3)
    want = _b3_atrous_separable(c, 5)
    assert np.abs(got[..., :3] - want).max() < 1e-12
    assert np.all(got[..., 3] == 1)


@pytest.mark.parametrize('demodulate', [True, False])
def test_an_albedo_edge_stops_the_filter(demodulate):
    '''two half-planes whose albedo differs by 1 at sigma_albedo = 0.1: a tap across the edge weighs at most exp(-100), so
    changing one half's colours moves the other half by less than 1e-30'''
    rng = np.random.default_rng(2)
    nx, ny = 24, 20
    F0 = _film(rng, nx, ny).reshape(nx, ny, 4)
    F1 = np.zeros((nx, ny, 4), np.float32)
    F1[:12] = [0.2, 0.2, 0.2, 1.0]
    F1[12:] = [1.2, 1.2, 1.2, 1.0]
    F2 = np.tile(np.float32([0, 0, 1, 1]), (nx * ny, 1))
    G0 = F0.copy()
    G0[12:, :, :3] = rng.uniform(0, 8, (12, ny, 3))
    a = denoise_ref(F0.reshape(-1, 4), F1.reshape(-1, 4), F2, nx, ny, demodulate=demodulate)
    b = denoise_ref(G0.reshape(-1, 4), F1.reshape(-1, 4), F2, nx, ny, demodulate=demodulate)
    assert np.abs(a[:12] - b[:12]).max() < 1e-30
    assert np.abs(a[12:] - b[12:]).max() > 0.1                       # (the changed half did change)


def test_an_empty_pixel_gives_the_marker_and_touches_nothing():
    rng = np.random.default_rng(3)
    nx, ny = 11, 14
    F0, F1, F2 = _film(rng, nx, ny), _film(rng, nx, ny), _film(rng, nx, ny)
    hole = 5 * ny + 6
    F0[hole] = [3.0, 2.0, 1.0, 0.0]
    G0 = F0.copy()
    G0[hole, :3] = [-50.0, 1e6, 7.0]
    for dtype in (np.float64, np.float32):
        a = denoise_ref(F0, F1, F2, nx, ny, dtype=dtype)
        b = denoise_ref(G0, F1, F2, nx, ny, dtype=dtype)
        assert a.dtype == dtype
        assert np.array_equal(a[5, 6], np.array(MARKER, np.float32).astype(dtype))
        assert np.array_equal(a, b)
        assert np.all(np.delete(a.reshape(-1, 4), hole, axis=0)[:, 3] == 1)


def test_zero_iterations_is_the_resolved_input():
    rng = np.random.default_rng(4)
    nx, ny = 7, 5
    F0, F1, F2 = _film(rng, nx, ny), _film(rng, nx, ny), _film(rng, nx, ny)
    F0[3] = 0
    out = denoise_ref(F0, F1, F2, nx, ny, iterations=0, dtype=np.float32)
    want = np.empty((nx * ny, 4), np.float32)
    want[:, :3] = F0[:, :3] / np.where(F0[:, 3:4] != 0, F0[:, 3:4], 1)
    want[:, 3] = 1
    want[3] = MARKER
    assert np.array_equal(out.reshape(-1, 4), want)


def test_f32_restatement_stays_close_to_f64():
    '''the f32 body is the same filter: on a random film its distance to the f64 result is rounding, a few 1e-7'''
    rng = np.random.default_rng(5)
    nx, ny = 21, 17
    F0, F1, F2 = _film(rng, nx, ny), _film(rng, nx, ny, 0.2, 0.9), _film(rng, nx, ny, -1, 1)
    a = denoise_ref(F0, F1, F2, nx, ny, dtype=np.float64)
    b = denoise_ref(F0, F1, F2, nx, ny, dtype=np.float32)
    assert b.dtype == np.float32
    assert (np.abs(b - a) / (1 + np.abs(a))).max() < 1e-5

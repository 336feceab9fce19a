'''
numpy restatement of FilmTable.get_noise (include/miptina.h, mpt_get_noise): the estimate in f32, one
numpy operation per operation of the definition, in its order -- numpy's f32 +, -, *, /, sqrt, fmax and fmin are the correctly
rounded IEEE operations ptina_amd/csrc/noise.hip compiles to, so the GPU's map and maximum must equal this file's bit for bit --
and the statistics over the valid pixels, the sum of the f32 values e taken in f64.  tests/test_noise_cpu.py holds this file to
Cycles' form and to what the estimate is for; tests/test_noise_gpu.py holds the GPU to it.
'''

import collections

import numpy as np

f32 = np.float32

# the fixed shape of the device's two-stage sum (noise.hip: NZ_BLOCK, NZ_PER_LANE): the first stage leaves one partial per RUN
# film elements, ONE workgroup of LANES lanes folds them
LANES, PER_LANE = 256, 4
RUN = LANES * PER_LANE

Stats = collections.namedtuple('Stats', 'valid above sum max')


def parts(npix):
    '''partials the first stage emits for a film of npix elements (noise.hip, mpt_noise_parts)'''
    return (int(npix) + RUN - 1) // RUN


def first_film_beyond_one_round():
    '''the smallest film for which the first stage emits more partials than the second stage has lanes: a lane of the fold then
    takes more than one'''
    npix = LANES * RUN + 1
    assert parts(npix) == LANES + 1 and parts(npix - 1) == LANES
    return npix


def clamp0(x):
    '''fminf(fmaxf(x, 0), 3e38): NaN -> 0, negative -> 0, +inf -> 3e38 (np.fmax / np.fmin return the argument that is not NaN)'''
    return np.fmin(np.fmax(np.asarray(x, f32), f32(0)), f32(3.0e38))


def noise_k(nA, nB):
    '''k = sqrtf(nA / nB)'''
    return np.sqrt(np.asarray(nA, f32) / np.asarray(nB, f32))


def noise_map(film_raw, mark_raw):
    '''(e [npix] f32, 0 where not valid; valid [npix] bool) of the accumulators film_raw and mark_raw [npix][4]'''
    F = np.ascontiguousarray(np.asarray(film_raw, f32).reshape(-1, 4))
    M = np.ascontiguousarray(np.asarray(mark_raw, f32).reshape(-1, 4))
    assert F.shape == M.shape
    with np.errstate(all='ignore'):
        nA, n = M[:, 3], F[:, 3]
        nB = n - nA
        valid = (nA > 0) & (nB > 0)
        a = clamp0(M[:, :3] / nA[:, None])
        m = clamp0(F[:, :3] / n[:, None])
        k = noise_k(nA, nB)
        d = np.abs(m - a) * k[:, None]
        num = ((d[:, 0] + d[:, 1]) + d[:, 2]) / f32(3)
        den = f32(1e-4) + np.sqrt(((m[:, 0] + m[:, 1]) + m[:, 2]) / f32(3))
        e = clamp0(num / den)
    assert e.dtype == f32
    return np.where(valid, e, f32(0)).astype(f32), valid


def noise_stats(e, valid, threshold):
    '''over the valid pixels: their count, the count of e > threshold (f32), the f64 sum of the f32 values e, the largest e'''
    ev = e[valid]
    return Stats(int(valid.sum()), int((ev > f32(threshold)).sum()), float(ev.astype(np.float64).sum()),
                 f32(ev.max()) if ev.size else f32(0))


def noise_ref(film_raw, mark_raw, threshold):
    '''(e, valid, Stats)'''
    e, valid = noise_map(film_raw, mark_raw)
    return e, valid, noise_stats(e, valid, threshold)


def synthetic_pair(seed, nx, ny, invalid=0.2):
    '''(film, mark) accumulators [nx*ny][4] of a render caught in the middle: per pixel nA in {1, 2, 4, 16, 3, 0.5} samples in the
    mark and nB in {1, 2, 4, 16, 5, 0.25} added since, the two groups' means scattered around a colour log-uniform over
    1e-5 .. 1e3 by a relative noise log-uniform over 1e-4 .. 1; of a share `invalid` of the pixels a third each has nA = 0, nB = 0
    and both'''
    rng = np.random.default_rng(seed)
    n = nx * ny
    nA = rng.choice(f32([1, 2, 4, 16, 3, 0.5]), n)
    nB = rng.choice(f32([1, 2, 4, 16, 5, 0.25]), n)
    c = np.exp(rng.uniform(np.log(1e-5), np.log(1e3), (n, 3)))
    s = np.exp(rng.uniform(np.log(1e-4), np.log(1.0), (n, 1)))
    a = c * np.abs(1 + s * rng.normal(0, 1, (n, 3)))
    b = c * np.abs(1 + s * rng.normal(0, 1, (n, 3)))
    kind = np.where(rng.random(n) < invalid, rng.integers(1, 4, n), 0)
    nA = np.where((kind == 1) | (kind == 3), f32(0), nA)
    nB = np.where((kind == 2) | (kind == 3), f32(0), nB)
    M = np.empty((n, 4), f32)
    M[:, :3] = a * nA[:, None]
    M[:, 3] = nA
    F = np.empty((n, 4), f32)
    F[:, :3] = M[:, :3].astype(np.float64) + b * nB[:, None]
    F[:, 3] = nA + nB
    return F, M

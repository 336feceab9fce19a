'''
CPU tests of the noise estimate's definition (include/miptina.h, mpt_get_noise): tests/noise_ref.py -- the
numpy restatement tests/test_noise_gpu.py holds the GPU to -- against Cycles' form computed independently, on invalid and poisoned
accumulators, and on the CPU oracle's films, where the estimate must fall as 1 / sqrt(N); the ABI record; and render_until's
schedule against a stub engine and a stub film.
'''

import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import setup_oracle
from noise_ref import (noise_map, noise_ref, noise_stats, noise_k, synthetic_pair, parts, first_film_beyond_one_round, LANES,
                       PER_LANE, RUN)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ULP = 2.0 ** -23            # the spacing of f32 at 1: a correctly rounded operation is within ULP / 2, relative


def _cycles(F, M):
    '''Cycles' criterion from the two halves' means, in f64: mean(|a - b|) / 2 over 1e-4 + sqrt(mean m)'''
    F, M = F.astype(np.float64), M.astype(np.float64)
    nA, nB = M[:, 3:4], F[:, 3:4] - M[:, 3:4]
    a, b, m = M[:, :3] / nA, (F[:, :3] - M[:, :3]) / nB, F[:, :3] / F[:, 3:4]
    return np.abs(a - b).mean(axis=1) / 2 / (1e-4 + np.sqrt(m.mean(axis=1))), a, m


def _dyadic_halves(seed, n):
    '''equal halves of 1, 2, 4 or 8 samples whose sums are integers below 2^12: a, b, m and m - a are exact in f32'''
    rng = np.random.default_rng(seed)
    h = rng.choice(f32([1, 2, 4, 8]), n)
    M = np.empty((n, 4), f32)
    F = np.empty((n, 4), f32)
    M[:, :3] = rng.integers(0, 2048, (n, 3))
    M[:, 3] = h
    F[:, :3] = M[:, :3] + rng.integers(0, 2048, (n, 3))
    F[:, 3] = 2 * h
    return F, M


def test_equal_halves_are_the_cycles_criterion():
    '''Means that are exact in f32: what is left are the estimate's own roundings -- two additions, a division by 3 (numerator), two
    additions, a division, a square root, an addition (denominator) and the last division, half an ulp each, the denominator's
    halved once by the root: under 5 ulp; held to 8'''
    F, M = _dyadic_halves(1, 4096)
    e, valid = noise_map(F, M)
    want, _, _ = _cycles(F, M)
    assert valid.all() and (want > 0).sum() > 4000
    err = np.abs(e.astype(np.float64) - want)
    print('dyadic halves: worst |e - cycles| = %.3f ulp' % float((err / (want * ULP + 1e-300)).max()))
    assert np.all(err <= 8 * ULP * want)


def test_equal_halves_of_rounded_means_stay_within_the_cancellation_bound():
    '''Means that round: a and m each carry half an ulp, and m - a cancels (itself exact or half an ulp), so per channel |m - a| is
    off by at most ULP / 2 (m + a) -- not relative to the difference.  With the 5 ulp of the rest:
    |e - cycles| <= 8 ULP cycles + ULP / 2 mean(m + a) / (1e-4 + sqrt(mean m)), the second term doubled for slack in its own
    roundings'''
    F, M = synthetic_pair(2, 64, 64, invalid=0.0)
    M[:, 3] = f32(4)
    F[:, 3] = f32(8)
    e, valid = noise_map(F, M)
    want, a, m = _cycles(F, M)
    assert valid.all()
    bound = 8 * ULP * want + ULP * (m + a).mean(axis=1) / (1e-4 + np.sqrt(m.mean(axis=1)))
    err = np.abs(e.astype(np.float64) - want)
    print('rounded halves: worst |e - cycles| / bound = %.3f' % float((err / bound).max()))
    assert np.all(err <= bound)


def test_k_is_exactly_one_for_equal_halves_and_the_group_ratio_otherwise():
    for h in (0.25, 0.5, 1, 2, 3, 5, 7, 16, 100, 1000, 12345, 2 ** 20, 2 ** 23):
        assert noise_k(f32(h), f32(2 * h) - f32(h)) == f32(1)
    assert noise_k(f32(16), f32(4)) == f32(2) and noise_k(f32(4), f32(16)) == f32(0.5)
    # unequal groups: |m - a| k is |a - b| sqrt(nA nB) / n, the standard error of m from the two group means
    F, M = synthetic_pair(3, 32, 32, invalid=0.0)
    e, valid = noise_map(F, M)
    F64, M64 = F.astype(np.float64), M.astype(np.float64)
    nA, n = M64[:, 3:4], F64[:, 3:4]
    nB = n - nA
    a, b, m = M64[:, :3] / nA, (F64[:, :3] - M64[:, :3]) / nB, F64[:, :3] / n
    want = (np.abs(a - b) * np.sqrt(nA * nB) / n).mean(axis=1) / (1e-4 + np.sqrt(m.mean(axis=1)))
    k = np.sqrt(nA / nB)[:, 0]
    bound = 10 * ULP * want + k * ULP * (m + a).mean(axis=1) / (1e-4 + np.sqrt(m.mean(axis=1)))      # (as above, the cancellation scaled by k)
    assert valid.all() and np.all(np.abs(e - want) <= bound)


def test_invalid_pixels_give_zero_and_are_not_counted():
    F, M = synthetic_pair(4, 16, 16, invalid=0.0)
    F[0:10, 3] = M[0:10, 3]                       # nB = 0
    M[10:20] = 0                                  # nA = 0
    F[20:30] = 0
    M[20:30] = 0                                  # both
    M[30:35, 3] = F[30:35, 3] + 1                 # nB < 0: a film cleared behind the mark's back
    M[35:40, 3] = -M[35:40, 3]                    # nA < 0
    e, valid, st = noise_ref(F, M, 0.0)
    assert not valid[:40].any() and valid[40:].all() and not e[:40].any() and (e[40:] > 0).all()
    assert st.valid == 256 - 40 and st.above == st.valid and st.max == e.max()
    assert st.sum == e[40:].astype(np.float64).sum()
    # nothing valid: every statistic 0
    e, valid, st = noise_ref(F, F, 0.0)
    assert st == (0, 0, 0.0, 0) and not e.any()
    # > and not >=: a threshold at a value that occurs does not count it
    e, valid = noise_map(*synthetic_pair(5, 16, 16))
    t = np.sort(e[valid])[valid.sum() // 2]
    assert noise_stats(e, valid, t).above == int((e[valid] > t).sum()) < int((e[valid] >= t).sum())
    assert noise_stats(e, valid, e.max()).above == 0


def test_poisoned_accumulators_give_finite_estimates():
    F, M = synthetic_pair(6, 24, 24, invalid=0.0)
    rng = np.random.default_rng(7)
    for bad in (np.nan, np.inf, -np.inf, -2.5, 3e38, -3e38):
        for A in (F, M):
            rows = rng.choice(len(A), 20, replace=False)
            A[rows, rng.integers(0, 3, 20)] = f32(bad)
    F[0, :3] = np.inf                             # every channel saturates: the sums overflow and the last clamp holds e
    F[1, :3] = f32([np.nan, np.inf, -1.0])
    M[2, :3] = np.inf
    F[3, :3] = 0
    M[3, :3] = 0                                  # zero radiance: 0 / 1e-4
    F[4, 3] = np.inf                              # an infinite weight: m = 0, k = 0
    F[5, 3] = np.nan                              # NaN weights are not valid
    M[6, 3] = np.nan
    e, valid, st = noise_ref(F, M, 0.05)
    assert np.isfinite(e).all() and (e >= 0).all() and e.max() <= f32(3e38)
    assert valid[:5].all() and not valid[5] and not valid[6] and e[3] == 0 and e[4] == 0 and e[5] == 0 and e[6] == 0
    assert np.isfinite(st.sum) and np.isfinite(st.max) and 0 < st.above < st.valid == 24 * 24 - 2


def test_the_stats_record_is_32_bytes_and_the_result_divides_safely():
    from ptina_amd._lib import NoiseStats, NoiseResult
    assert C.sizeof(NoiseStats) == 32
    assert [(n, t) for n, t in NoiseStats._fields_] == [('valid', C.c_int64), ('above', C.c_int64), ('sum', C.c_double),
                                                        ('max', C.c_float), ('threshold', C.c_float)]
    r = NoiseResult(NoiseStats(0, 0, 0.0, 0.0, 0.5))
    assert (r.valid, r.above, r.mean, r.max, r.fraction, r.map, r.threshold) == (0, 0, 0.0, 0.0, 0.0, None, 0.5)
    r = NoiseResult(NoiseStats(8, 2, 4.0, 1.5, 0.25), map='m')
    assert (r.mean, r.fraction, r.max, r.map) == (0.5, 0.25, 1.5, 'm')


def test_the_restatement_names_the_kernels_sum_shape():
    '''noise_ref's sizing function is noise.hip's: the GPU test takes the film that sends the fold round twice from it'''
    src = open(os.path.join(ROOT, 'ptina_amd', 'csrc', 'noise.hip')).read()
    got = dict((k, int(v)) for k, v in re.findall(r'\b(NZ_BLOCK|NZ_PER_LANE) = (\d+)', src))
    assert got == {'NZ_BLOCK': LANES, 'NZ_PER_LANE': PER_LANE} and 'NZ_RUN = NZ_BLOCK * NZ_PER_LANE' in src
    assert re.search(r'mpt_noise_parts\(size_t npix\) \{ return \(npix \+ NZ_RUN - 1\) / NZ_RUN; \}', src)
    assert [parts(n) for n in (0, 1, RUN, RUN + 1, 97 * 61)] == [0, 1, 1, 2, 6]
    assert first_film_beyond_one_round() == LANES * RUN + 1


# ---------------------------------------------------------------- render_until's schedule
class StubFilm:
    '''a film whose estimate is what the test says it is at each sample count'''

    def __init__(self, engine, above_at, valid=100):
        self.engine, self.above_at, self.valid, self.marks, self.calls = engine, above_at, valid, [], []

    def mark(self):
        self.marks.append(self.engine.spp)

    def get_noise(self, threshold, map=False, remark=False):
        from ptina_amd._lib import NoiseStats, NoiseResult
        self.calls.append((self.engine.spp, threshold, map, remark))
        return NoiseResult(NoiseStats(self.valid, self.above_at(self.engine.spp), 0.0, 0.0, threshold))


class StubEngine:
    def __init__(self):
        self.spp, self.renders = 0, []

    def render(self, nframes=1):
        assert nframes >= 1
        self.renders.append(nframes)
        self.spp += nframes


def _run(above_at, *args, **kw):
    from ptina_amd.engine import render_until
    eng = StubEngine()
    film = StubFilm(eng, above_at)
    return render_until(eng, *args, film=film, **kw), eng, film


def test_render_until_stops_at_the_first_passing_check():
    r, eng, film = _run(lambda spp: 0 if spp >= 64 else 50, 0.05, 1024, min_spp=4)
    assert (r.spp, r.converged) == (64, True) and [s for s, _ in r.history] == [8, 16, 32, 64]
    assert eng.renders == [4, 4, 8, 16, 32] and film.marks == [4]
    assert film.calls == [(s, 0.05, False, True) for s in (8, 16, 32, 64)]          # one re-marking check per doubling, no map
    assert [st.above for _, st in r.history] == [50, 50, 50, 0]
    # at the very first check
    r, eng, film = _run(lambda spp: 0, 1e9, 64, min_spp=2)
    assert (r.spp, r.converged, len(r.history)) == (4, True, 1) and eng.renders == [2, 2]
    # the default floor is 16 frames
    r, eng, film = _run(lambda spp: 0, 0.1, 64)
    assert eng.renders == [16, 16] and film.marks == [16]


def test_render_until_honours_the_fraction():
    above = {8: 30, 16: 11, 32: 10, 64: 0}
    r, _, _ = _run(lambda spp: above[spp], 0.05, 1024, min_spp=4, fraction=0.1)
    assert (r.spp, r.converged) == (32, True)                                         # 11 > 0.1 x 100 >= 10
    r, _, _ = _run(lambda spp: above[spp], 0.05, 1024, min_spp=4)
    assert (r.spp, r.converged) == (64, True)


def test_render_until_never_exceeds_max_spp_and_spends_it_all():
    r, eng, film = _run(lambda spp: 1, 0.0, 20, min_spp=4)
    assert (r.spp, r.converged) == (20, False) and [s for s, _ in r.history] == [8, 16, 20] and eng.renders == [4, 4, 8, 4]
    for min_spp in (1, 2, 3, 5, 16):
        for max_spp in (2 * min_spp, 2 * min_spp + 1, 37, 64, 100, 1000):
            if max_spp < 2 * min_spp:
                continue
            r, eng, film = _run(lambda spp: 1, 0.01, max_spp, min_spp=min_spp)
            assert r.spp == max_spp == eng.spp == sum(eng.renders) and not r.converged
            assert all(s <= max_spp for s, _ in r.history) and r.history[-1][0] == max_spp
            assert all(b == min(2 * a, max_spp) for a, b in zip([min_spp] + [s for s, _ in r.history], [s for s, _ in r.history]))
    # converging exactly at the cap is converging
    r, _, _ = _run(lambda spp: 0 if spp == 20 else 1, 0.0, 20, min_spp=4)
    assert (r.spp, r.converged) == (20, True)


def test_render_until_refuses_bad_arguments_before_it_renders():
    from ptina_amd.engine import render_until
    for kw in (dict(max_spp=64, min_spp=0), dict(max_spp=64, min_spp=-3), dict(max_spp=31, min_spp=16), dict(max_spp=1, min_spp=1)):
        eng = StubEngine()
        with pytest.raises(ValueError, match='render_until'):
            render_until(eng, 0.05, film=StubFilm(eng, lambda spp: 0), **kw)
        assert eng.renders == []


def test_the_engines_and_the_worker_expose_render_until():
    import inspect
    import ptina_amd.worker as worker
    from ptina_amd.engine.path import PathEngine
    from ptina_amd.engine.brute import BruteEngine
    from ptina_amd.things import FilmTable
    for cls in (PathEngine, BruteEngine):
        assert list(inspect.signature(cls.render_until).parameters) == ['self', 'noise', 'max_spp', 'min_spp', 'fraction']
        assert inspect.signature(cls.render_until).parameters['min_spp'].default == 16
    assert callable(worker.render_until) and callable(worker.get_noise)
    assert 'render_until' not in worker._PASS_THROUGH and 'get_noise' not in worker._PASS_THROUGH
    for name in ('mark', 'get_noise', 'get_mark', 'noise_kernel_time'):
        assert callable(getattr(FilmTable, name))
    ns = {}
    exec('from ptina.engine.path import *', ns)                   # the drop-in alias package re-exports the loop
    assert ns['render_until'] is __import__('ptina_amd.engine', fromlist=['x']).render_until


# ---------------------------------------------------------------- what the estimate is for
@pytest.mark.parametrize('scene,nx,ny', [('s34', 32, 32), ('s978', 24, 24)])
def test_the_estimate_falls_as_the_film_converges(oracle_mod, scene, nx, ny):
    '''On the CPU oracle's films, doubling from a mark at 2 spp: the mean of e over the film falls from the 4-spp check to the
    64-spp check by more than a factor of 2 (1 / sqrt(N) predicts 4; measured 0.1355 -> 0.0333 for s34 at 32 x 32 and
    0.1298 -> 0.0356 for s978 at 24 x 24)'''
    from ptina_amd import scenes
    o = setup_oracle(oracle_mod, scenes.get_scene(scene), nx, ny)
    o.render(2)
    mark, spp, means = o.get_film_raw(0), 2, {}
    while spp < 64:
        o.render(spp)
        spp *= 2
        film = o.get_film_raw(0)
        assert np.all(film[:, 3] == spp) and np.all(mark[:, 3] == spp // 2)
        e, valid, st = noise_ref(film, mark, 0.05)
        assert valid.all() and np.all(noise_k(mark[:, 3], film[:, 3] - mark[:, 3]) == 1)
        means[spp] = st.sum / st.valid
        mark = film
    print(scene, {k: round(v, 4) for k, v in means.items()})
    assert means[4] > 2 * means[64] > 0
    assert means[4] > means[16] > means[64]

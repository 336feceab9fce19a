'''
GPU tests (-m gpu) of the film's noise estimate (FilmTable.mark / get_noise, mpt_noise_eval, render_until; ptina_amd/csrc/noise.hip).

Parity is against tests/noise_ref.py (held to Cycles' form by tests/test_noise_cpu.py) fed with the very accumulators the device
holds.  Every operation of e is one correctly rounded IEEE f32 operation on both sides, so the map and the maximum must be EQUAL,
bit for bit, and the counts equal integers; the f64 sum of the f32 values may differ by the order of the additions only: with
non-negative terms, at most npix 2^-52 of the sum.
'''

import ctypes as C

import numpy as np
import pytest

from helpers import setup_engine, report
from noise_ref import noise_map, noise_stats, synthetic_pair, first_film_beyond_one_round, parts, RUN, LANES

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


def _scene(name):
    from ptina_amd import scenes
    return scenes.get_scene(name)


def _film():
    from ptina_amd.things import FilmTable
    return FilmTable()


def _ctx():
    from ptina_amd.common import ctx
    return ctx()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u32), np.ascontiguousarray(b).view(u32))


def _thresholds(e, valid):
    '''0, and values of e that occur -- the median and the largest -- so that > against >= shows'''
    ev = np.sort(e[valid])
    return [0.0] + ([float(ev[ev.size // 2]), float(ev[-1])] if ev.size else [0.5])


def _held(what, got, F, M, nx, ny, threshold, want_map=True):
    '''a NoiseResult against the restatement on the film F and the mark M'''
    e, valid = noise_map(F, M)
    want = noise_stats(e, valid, threshold)
    npix = nx * ny
    slack = npix * 2.0 ** -52 * want.sum
    report(f'noise {what} {nx}x{ny} threshold {threshold:.9g}: valid {got.valid} / {want.valid}, above {got.above} / {want.above}, max {got.max:.9g} / '
           f'{float(want.max):.9g}, sum {got.sum!r} / {want.sum!r} (off {abs(got.sum - want.sum):.3e}, bound {slack:.3e})'
           + (f', map differs in {int((got.map.reshape(-1).view(u32) != e.view(u32)).sum())} of {npix}' if got.map is not None else ''))
    assert (got.map is not None) == want_map
    if want_map:
        assert got.map.dtype == f32 and got.map.shape == (nx, ny)
        assert _same(got.map.reshape(-1), e), f'{what}: the map is not the restatement bit for bit'
    assert (got.valid, got.above) == (want.valid, want.above), what
    assert f32(got.max).view(u32) == f32(want.max).view(u32), what
    assert abs(got.sum - want.sum) <= slack, what
    assert f32(got.threshold) == f32(threshold)
    assert got.mean == (got.sum / got.valid if got.valid else 0.0) and got.fraction == (got.above / got.valid if got.valid else 0.0)
    return e, valid


# ---------------------------------------------------------------- 1. the door against the restatement
BEYOND = first_film_beyond_one_round()
DOOR = [(1, 1), (3, 5), (16, 16), (32, 32), (257, 1), (1, RUN + 1), (97, 61), (BEYOND, 1)]
# one pixel; less than a wave; a workgroup's run exactly (16 x 16 of display.hip's idiom is a quarter of it, 32 x 32 is it); ragged
# runs; one element into the second workgroup; several workgroups; more partials than the fold has lanes


@pytest.mark.parametrize('nx,ny', DOOR)
def test_door_is_the_restatement_bit_for_bit(fresh, nx, ny):
    from ptina_amd.things import init_things
    init_things()
    F, M = synthetic_pair(1000 * nx + ny, nx, ny)
    if nx * ny == 1:
        F, M = f32([[3.0, 1.5, 0.25, 4]]), f32([[1.0, 1.0, 0.125, 2]])
    assert parts(nx * ny) == (LANES + 1 if nx == BEYOND else (nx * ny + RUN - 1) // RUN)
    e, valid = noise_map(F, M)
    assert valid.any()
    for t in _thresholds(e, valid):
        got, new = _ctx().noise_eval(F, M, nx, ny, t)
        _held('door', got, F, M, nx, ny, t)
        assert _same(new, F), 'the re-marked mark is not the film'
    # without the map, without the new mark: the same statistics
    t = _thresholds(e, valid)[1]
    a, new = _ctx().noise_eval(F, M, nx, ny, t, map=False, remark=False)
    assert new is None
    _held('door, statistics only', a, F, M, nx, ny, t, want_map=False)
    b, _ = _ctx().noise_eval(F, M, nx, ny, t)
    assert (a.valid, a.above, a.sum, a.max) == (b.valid, b.above, b.sum, b.max)


def test_door_on_poisoned_and_degenerate_films(fresh):
    from ptina_amd.things import init_things
    init_things()
    nx, ny = 33, 31
    F, M = synthetic_pair(21, nx, ny)
    rng = np.random.default_rng(22)
    for bad in (np.nan, np.inf, -np.inf, -2.5, 3e38, -3e38):
        for A in (F, M):
            rows = rng.choice(len(A), 12, replace=False)
            A[rows, rng.integers(0, 3, 12)] = f32(bad)
    F[0] = f32([np.inf, np.inf, np.inf, 8])
    M[0] = f32([1, 2, 3, 4])                       # every channel saturates: the sums overflow, the last clamp holds e
    F[1] = f32([np.nan, np.inf, -1.0, 8])
    M[1] = f32([np.inf, np.inf, 0, 4])
    F[2, 3], M[2, 3] = np.inf, 1                   # an infinite weight: valid, m = 0, k = 0
    F[3, 3], M[3, 3] = np.nan, 1                   # NaN weights: not valid
    F[4, 3], M[4, 3] = 4, np.nan
    F[5], M[5] = f32([1e-42, 0, 1e-40, 2]), f32([1e-44, 1e-45, 0, 1])        # denormal sums and means
    e, valid = noise_map(F, M)
    assert np.isfinite(e).all() and valid[:3].all() and not valid[3] and not valid[4] and valid[5] and e[5] > 0
    for t in _thresholds(e, valid):
        got, new = _ctx().noise_eval(F, M, nx, ny, t)
        _held('poisoned', got, F, M, nx, ny, t)
        assert _same(new, F) and np.isfinite(got.map).all() and np.isfinite(got.sum) and np.isfinite(got.max)
    # nothing valid: the mark is the film (no sample since); no mark at all; no film
    F, M = synthetic_pair(23, nx, ny, invalid=0.0)
    for f, m in ((F, F), (F, np.zeros_like(M)), (np.zeros_like(F), np.zeros_like(M))):
        got, new = _ctx().noise_eval(f, m, nx, ny, 0.0)
        _held('nothing valid', got, f, m, nx, ny, 0.0)
        assert (got.valid, got.above, got.sum, got.max, got.mean, got.fraction) == (0, 0, 0.0, 0.0, 0.0, 0.0) and not got.map.any()
        assert _same(new, f)
    # zero radiance, every pixel valid: e = 0 / 1e-4
    f = np.zeros((nx * ny, 4), f32)
    m = np.zeros((nx * ny, 4), f32)
    f[:, 3], m[:, 3] = 8, 4
    got, _ = _ctx().noise_eval(f, m, nx, ny, 0.0)
    _held('black', got, f, m, nx, ny, 0.0)
    assert (got.valid, got.above, got.sum, got.max) == (nx * ny, 0, 0.0, 0.0) and not got.map.any()


def test_door_calls_repeat_bit_for_bit(fresh):
    from ptina_amd.things import init_things
    init_things()
    nx, ny = 97, 61
    F, M = synthetic_pair(31, nx, ny)
    e, valid = noise_map(F, M)
    t = _thresholds(e, valid)[1]
    a, na = _ctx().noise_eval(F, M, nx, ny, t)
    other, _ = _ctx().noise_eval(*synthetic_pair(32, 64, 50), 64, 50, 0.1)        # (another film through the same buffers in between)
    b, nb = _ctx().noise_eval(F, M, nx, ny, t)
    assert a.map is not b.map and a.map.tobytes() == b.map.tobytes() and na.tobytes() == nb.tobytes()
    assert (a.valid, a.above, a.max) == (b.valid, b.above, b.max) and np.float64(a.sum).tobytes() == np.float64(b.sum).tobytes()
    assert other.valid != a.valid


# ---------------------------------------------------------------- 2. rendered films
@pytest.mark.parametrize('scene,nx,ny', [('s34', 32, 32), ('s978', 40, 24)])
def test_rendered_films(fresh, scene, nx, ny):
    eng = setup_engine(_scene(scene), nx, ny)
    film = _film()
    eng.render(4)
    film.mark()
    raw4 = film.get_raw(0).copy()
    assert np.all(raw4[:, 3] == 4) and _same(film.get_mark(), raw4)
    eng.render(4)
    raw8 = film.get_raw(0).copy()
    e, valid = noise_map(raw8, raw4)
    assert valid.all()
    got = {}
    for t in _thresholds(e, valid):
        got[t] = film.get_noise(t, map=True)
        _held(f'{scene} 4+4', got[t], raw8, raw4, nx, ny, t)
        assert _same(film.get_mark(), raw4)                      # without remark the mark stays
    t = _thresholds(e, valid)[1]
    again = film.get_noise(t, map=True)
    assert again.map is not got[t].map and again.map.tobytes() == got[t].map.tobytes()
    assert (again.valid, again.above, again.max, np.float64(again.sum).tobytes()) == \
        (got[t].valid, got[t].above, got[t].max, np.float64(got[t].sum).tobytes())
    _held(f'{scene} 4+4, statistics only', film.get_noise(t), raw8, raw4, nx, ny, t, want_map=False)
    # remark: the same estimate, and the mark is the film as it is now
    _held(f'{scene} 4+4, remark', film.get_noise(t, map=True, remark=True), raw8, raw4, nx, ny, t)
    assert _same(film.get_mark(), raw8) and _same(film.get_raw(0), raw8)
    eng.render(8)
    raw16 = film.get_raw(0).copy()
    assert np.all(raw16[:, 3] == 16)
    e16, v16 = noise_map(raw16, raw8)
    t = _thresholds(e16, v16)[1]
    _held(f'{scene} 8+8', film.get_noise(t, map=True, remark=True), raw16, raw8, nx, ny, t)
    assert _same(film.get_mark(), raw16)
    # nothing rendered since the mark: nothing valid
    r = film.get_noise(0.0, map=True)
    assert (r.valid, r.above, r.sum, r.max) == (0, 0, 0.0, 0.0) and not r.map.any()


# ---------------------------------------------------------------- 3. nothing is disturbed
def test_mark_and_estimate_write_no_film_pass(fresh):
    from ptina_amd.engine.preview import PreviewEngine
    nx, ny = 40, 24
    eng = setup_engine(_scene('s978'), nx, ny)
    film = _film()
    eng.render(4)
    PreviewEngine().render(2)
    before = [film.get_raw(p).copy() for p in range(3)]
    film.mark()
    for p in range(3):
        assert _same(before[p], film.get_raw(p)), f'mark() changed pass {p}'
    eng.render(4)
    before = [film.get_raw(p).copy() for p in range(3)]
    film.get_noise(0.05)
    film.get_noise(0.05, map=True)
    film.get_noise(0.05, map=True, remark=True)
    for p in range(3):
        assert _same(before[p], film.get_raw(p)), f'get_noise() changed pass {p}'


def test_a_film_rendered_around_the_calls_is_the_film_rendered_without_them(fresh):
    from ptina_amd import common
    nx, ny = 32, 32
    eng = setup_engine(_scene('s34'), nx, ny)
    eng.render(16)
    want = _film().get_raw(0).copy()
    common.reset_all()
    eng = setup_engine(_scene('s34'), nx, ny)
    film = _film()
    eng.render(4)
    film.mark()
    eng.render(4)
    film.get_noise(0.05, remark=True)
    eng.render(8)
    assert np.all(want[:, 3] == 16) and _same(film.get_raw(0), want)


def test_get_noise_leaves_the_image_hint_intact(fresh):
    '''render(); mark() / get_noise(); get_image() returns the image of a context that never called them, bit for bit:
    PathEngine.render() hints the array of the next get_image(0), and the calls run between the hint and the call that spends it'''
    from ptina_amd import common
    nx, ny = 48, 40
    eng = setup_engine(_scene('s978'), nx, ny)
    eng.render(3)
    want3 = _film().get_image().copy()
    eng.render(2)
    want5 = _film().get_image().copy()
    common.reset_all()
    eng = setup_engine(_scene('s978'), nx, ny)
    eng.render(3)
    _film().mark()
    assert _same(_film().get_image(), want3)
    eng.render(2)
    _film().get_noise(0.05)
    _film().get_noise(0.05, map=True, remark=True)
    assert _same(_film().get_image(), want5)


def test_a_mark_behind_enqueued_launches_sees_them_all(fresh):
    nx, ny = 32, 32
    eng = setup_engine(_scene('s34'), nx, ny)
    film = _film()
    for _ in range(40):
        eng.render(1)
    film.mark()
    raw = film.get_raw(0)
    assert np.all(raw[:, 3] == 40) and _same(film.get_mark(), raw)
    for _ in range(24):
        eng.render(1)
    r = film.get_noise(0.05, map=True)                           # ... and so does an estimate
    _held('s34 40+24 enqueued', r, film.get_raw(0), raw, nx, ny, 0.05)
    assert r.valid == nx * ny


# ---------------------------------------------------------------- 4. a slab
def test_slab_columns_outside_are_not_valid(fresh):
    nx, ny = 56, 24
    eng = setup_engine(_scene('s34'), nx, ny, slab=(16, 40))
    film = _film()
    eng.render(4)
    film.mark()
    eng.render(4)
    F, M = film.get_raw(0).copy(), film.get_mark()
    w = F.reshape(nx, ny, 4)[..., 3]
    assert np.all(w[16:40] == 8) and not w[:16].any() and not w[40:].any()
    e, valid = noise_map(F, M)
    t = _thresholds(e, valid)[1]
    got = film.get_noise(t, map=True)
    _held('s34 56x24 slab 16..40', got, F, M, nx, ny, t)
    assert got.valid == 24 * ny and not got.map[:16].any() and not got.map[40:].any() and (got.map[16:40] > 0).any()
    cut = [np.ascontiguousarray(A.reshape(nx, ny, 4)[16:40]).reshape(-1, 4) for A in (F, M)]
    door, _ = _ctx().noise_eval(cut[0], cut[1], 24, ny, t)
    assert (door.valid, door.above, door.max) == (got.valid, got.above, got.max)
    assert abs(door.sum - got.sum) <= nx * ny * 2.0 ** -52 * door.sum             # (another film size: another order of the sum)
    assert _same(door.map, got.map[16:40])


# ---------------------------------------------------------------- 5. render_until on the device
def test_render_until_stops_at_the_first_check_or_at_the_cap(fresh):
    from ptina_amd import common
    nx, ny = 32, 32
    eng = setup_engine(_scene('s34'), nx, ny)
    r = eng.render_until(1e9, 64, min_spp=2)
    assert (r.spp, r.converged, len(r.history)) == (4, True, 1) and r.history[0][0] == 4
    assert r.history[0][1].valid == nx * ny and r.history[0][1].above == 0
    assert np.all(_film().get_raw(0)[:, 3] == 4)
    common.reset_all()
    eng = setup_engine(_scene('s34'), nx, ny)
    r = eng.render_until(0.0, 20, min_spp=4)
    assert (r.spp, r.converged) == (20, False) and [s for s, _ in r.history] == [8, 16, 20]
    assert all(st.above > 0 and st.valid == nx * ny for _, st in r.history)
    assert np.all(_film().get_raw(0)[:, 3] == 20)


def test_render_until_converges_inside_the_schedule(fresh):
    '''noise 0.05 on 90 % of the pixels: the CPU oracle alone passes first at 128 spp (fraction above 0.077 there, 0.179 at 64)'''
    from ptina_amd import common
    import ptina_amd.worker as worker
    nx, ny = 32, 32
    eng = setup_engine(_scene('s34'), nx, ny)
    r = eng.render_until(0.05, 1024, min_spp=2, fraction=0.1)
    report('render_until s34 32x32 noise 0.05 fraction 0.1: ' + ', '.join(f'{s} spp {st.above}/{st.valid}' for s, st in r.history))
    assert r.converged and 4 < r.spp < 1024
    assert [s for s, _ in r.history] == [4 << i for i in range(len(r.history))] and r.history[-1][0] == r.spp
    passes = [st.above <= 0.1 * st.valid for _, st in r.history]
    assert passes == [False] * (len(passes) - 1) + [True]
    assert all(st.valid == nx * ny and st.threshold == f32(0.05) for _, st in r.history)
    got = _film().get_raw(0).copy()
    assert np.all(got[:, 3] == r.spp)
    # the worker's call: the same loop on a fresh context, and its film the film of render(spp)
    common.reset_all()
    setup_engine(_scene('s34'), nx, ny)
    w = worker.render_until(0.05, 1024, min_spp=2, fraction=0.1)
    assert (w.spp, w.converged) == (r.spp, r.converged)
    assert [(s, st.valid, st.above, st.sum, st.max) for s, st in w.history] == [(s, st.valid, st.above, st.sum, st.max) for s, st in r.history]
    assert _same(_film().get_raw(0), got)
    common.reset_all()
    eng = setup_engine(_scene('s34'), nx, ny)
    eng.render(r.spp)
    assert _same(_film().get_raw(0), got)


def test_worker_get_noise_and_the_brute_engine(fresh):
    import ptina_amd.worker as worker
    from ptina_amd.engine.brute import BruteEngine
    nx, ny = 32, 32
    eng = setup_engine(_scene('s34'), nx, ny)
    eng.render(4)
    _film().mark()
    eng.render(4)
    a, b = worker.get_noise(0.05, map=True), _film().get_noise(0.05, map=True)
    assert (a.valid, a.above, a.sum, a.max) == (b.valid, b.above, b.sum, b.max) and a.map.tobytes() == b.map.tobytes()
    _film().clear()
    r = BruteEngine().render_until(0.05, 16, min_spp=2)
    assert r.spp in (4, 8, 16) and [s for s, _ in r.history] == [4, 8, 16][:len(r.history)] and r.history[-1][0] == r.spp
    assert all(st.valid == nx * ny for _, st in r.history)
    assert np.all(_film().get_raw(0)[:, 3] == r.spp)


# ---------------------------------------------------------------- 6. every stated error
def test_every_stated_error_raises_and_leaves_film_and_mark(fresh):
    from ptina_amd._lib import NoiseStats
    nx, ny = 16, 16
    eng = setup_engine(_scene('s34'), nx, ny)
    film, c = _film(), _ctx()
    eng.render(2)
    for call in (lambda: film.get_noise(0.05), film.get_mark):                  # no mark yet
        with pytest.raises(RuntimeError, match='no mark'):
            call()
    film.mark()
    eng.render(2)
    F, M = film.get_raw(0).copy(), film.get_mark()
    st = NoiseStats()
    fp = C.POINTER(C.c_float)
    for t in (-0.5, -1e-30, float('nan'), float('inf'), float('-inf')):
        with pytest.raises(RuntimeError, match='threshold must be finite and not negative'):
            film.get_noise(t, remark=True)
        with pytest.raises(RuntimeError, match='threshold must be finite and not negative'):
            c.noise_eval(F, M, nx, ny, t)
    with pytest.raises(RuntimeError, match='null map and null statistics'):
        c.call('mpt_get_noise', 0.05, 1, None, None)
    with pytest.raises(RuntimeError, match='null output'):
        c.call('mpt_get_mark', None)
    with pytest.raises(RuntimeError, match='null input'):
        c.call('mpt_noise_eval', 0.05, None, M.ctypes.data_as(fp), nx, ny, None, None, C.byref(st))
    for bad in ((0, 4), (4, 0), (-1, 4), (2 ** 15, 2 ** 15)):
        with pytest.raises(RuntimeError, match='max_filmsize'):
            c.call('mpt_noise_eval', 0.05, F.ctypes.data_as(fp), M.ctypes.data_as(fp), bad[0], bad[1], None, None, C.byref(st))
    assert _same(film.get_raw(0), F) and _same(film.get_mark(), M)
    assert film.get_noise(0.05).valid == nx * ny                                # (the context is still good)
    # one launch span per call, then nothing
    film.noise_kernel_time()
    film.get_noise(0.05, map=True)
    ms, n = film.noise_kernel_time()
    assert n == 1 and ms > 0
    assert film.noise_kernel_time() == (0.0, 0)
    c.noise_eval(F, M, nx, ny, 0.05)                                            # (the door is not timed)
    assert film.noise_kernel_time() == (0.0, 0)
    # a scene, camera or light change keeps the mark
    from ptina_amd.things import Camera, LightPool
    from ptina_amd import scenes
    Camera().set_perspective(scenes.BENCH_CAMERA)
    LightPool().clear()
    assert _same(film.get_mark(), M) and film.get_noise(0.05).valid == nx * ny
    # clear() drops it, and so does set_size
    film.clear()
    zero = film.get_raw(0).copy()
    assert not zero.any()
    for call in (lambda: film.get_noise(0.05, map=True, remark=True), film.get_mark):
        with pytest.raises(RuntimeError, match='no mark'):
            call()
    assert _same(film.get_raw(0), zero)
    film.mark()
    assert _same(film.get_mark(), zero)
    film.set_size(24, 8)
    for call in (lambda: film.get_noise(0.05), film.get_mark):
        with pytest.raises(RuntimeError, match='no mark'):
            call()
    film.mark()
    assert film.get_mark().shape == (24 * 8, 4)

'''
GPU tests (-m gpu) of adaptive sampling (FilmTable.select / get_selection / set_selection / get_samples, PathEngine.render_selected /
render_adaptive, mpt_adapt_*; ptina_amd/csrc/adapt_select.hip, adapt_kernel.hip).

The selection is held to tests/adaptive_ref.py (held to brute-force loops by tests/test_adaptive_cpu.py) fed with the very
accumulators the device holds: the list must be EQUAL as an array, in the device's stated order, and the statistics equal
mpt_noise_eval's field for field.  A list pass is held to the PathEngine in the strict build and to the path door (mpt_mlt_trace)
in both builds, bit for bit: it adds the same samples to the same pixels in the same order.
'''

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref
from helpers import setup_engine, report
from noise_ref import noise_map, synthetic_pair

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _thresholds(F, M):
    '''0, and values of e that occur -- the median and the largest -- so that > against >= shows'''
    e, valid = noise_map(F, M)
    ev = np.sort(e[valid])
    return [0.0] + ([float(ev[ev.size // 2]), float(ev[-1])] if ev.size else [0.5])


def _stats(r):
    return (r.valid, r.above, r.sum, r.max, r.threshold)


def _door_held(what, F, M, nx, ny, t, dilate):
    got, L = _ctx().adapt_eval(F, M, nx, ny, t, dilate)
    want = adaptive_ref.select_ordered(F, M, nx, ny, t, dilate)
    noise, _ = _ctx().noise_eval(F, M, nx, ny, t, map=False, remark=False)
    report(f'adapt door {what} {nx}x{ny} threshold {t:.9g} dilate {dilate}: {L.size} listed / {want.size}, above {got.above}, valid {got.valid}')
    assert L.dtype == np.int32 and np.array_equal(L, want), f'{what}: the list is not the restatement, in the device order'
    assert _stats(got) == _stats(noise), what                                  # field for field, the f64 sum included
    return got, L


# ---------------------------------------------------------------- 1. the selection door is the restatement
DOOR = [(1, 1), (3, 5), (16, 16), (17, 33), (32, 32), (257, 1), (1, 1025), (97, 61)]
# one pixel; less than a wave; one tile exactly; ragged tiles on both axes; four whole tiles; a film one pixel wide either way, one
# element into the last tile; several ragged tiles


@pytest.mark.parametrize('nx,ny', DOOR)
def test_selection_door_is_the_restatement(fresh, nx, ny):
    from ptina_amd.things import init_things
    init_things()
    F, M = synthetic_pair(100 + nx + 7 * ny, nx, ny)
    for t in _thresholds(F, M):
        for dilate in (0, 1):
            _door_held('synthetic', F, M, nx, ny, t, dilate)


def test_selection_door_on_poisoned_and_degenerate_films(fresh):
    from ptina_amd.things import init_things
    init_things()
    nx, ny = 33, 31
    F, M = synthetic_pair(21, nx, ny)                  # the poisoned film of test_noise_gpu.py
    rng = np.random.default_rng(22)
    for bad in (np.nan, np.inf, -np.inf, -2.5, 3e38, -3e38):
        for A in (F, M):
            rows = rng.choice(len(A), 12, replace=False)
            A[rows, rng.integers(0, 3, 12)] = f32(bad)
    F[0], M[0] = f32([np.inf, np.inf, np.inf, 8]), f32([1, 2, 3, 4])
    F[1], M[1] = f32([np.nan, np.inf, -1.0, 8]), f32([np.inf, np.inf, 0, 4])
    F[2, 3], M[2, 3] = np.inf, 1                       # an infinite weight: valid
    F[3, 3], M[3, 3] = np.nan, 1                       # NaN weights: not valid
    F[4, 3], M[4, 3] = 4, np.nan
    F[5], M[5] = f32([1e-42, 0, 1e-40, 2]), f32([1e-44, 1e-45, 0, 1])
    for t in _thresholds(F, M):
        for dilate in (0, 1):
            _, L = _door_held('poisoned', F, M, nx, ny, t, dilate)
            assert 3 not in L and 4 not in L
    # nothing valid: the mark is the film; no mark at all; no film
    F, M = synthetic_pair(23, nx, ny, invalid=0.0)
    for f, m in ((F, F), (F, np.zeros_like(M)), (np.zeros_like(F), np.zeros_like(M))):
        for dilate in (0, 1):
            got, L = _door_held('nothing valid', f, m, nx, ny, 0.0, dilate)
            assert got.valid == 0 and L.size == 0
    # everything above: every pixel valid with e > 0
    e, valid = noise_map(F, M)
    assert valid.all() and (e > 0).all()
    for dilate in (0, 1):
        got, L = _door_held('everything above', F, M, nx, ny, 0.0, dilate)
        assert L.size == nx * ny == got.above and np.array_equal(L, adaptive_ref.device_order(np.arange(nx * ny), ny))


def test_selection_door_calls_repeat_bit_for_bit(fresh):
    from ptina_amd.things import init_things
    init_things()
    nx, ny = 97, 61
    F, M = synthetic_pair(31, nx, ny)
    t = _thresholds(F, M)[1]
    a, la = _ctx().adapt_eval(F, M, nx, ny, t, 1)
    _ctx().adapt_eval(*synthetic_pair(32, 64, 50), 64, 50, 0.1, 1)            # (another film through the same buffers in between)
    b, lb = _ctx().adapt_eval(F, M, nx, ny, t, 1)
    assert la.tobytes() == lb.tobytes() and _stats(a) == _stats(b) and 0 < la.size < nx * ny


# ---------------------------------------------------------------- 2. strict build: a list pass against the PathEngine
def _prefix(scene, nx, ny, mode):
    '''a fresh context after render(4), mark(), render(4); returns (engine, F0, M0)'''
    from ptina_amd import common
    common.reset_all()
    eng = setup_engine(_scene(scene), nx, ny, mode=mode)
    eng.render(4)
    _film().mark()
    eng.render(4)
    return eng, _film().get_raw().copy(), _film().get_mark().copy()


@pytest.mark.parametrize('dilate', [0, 1])
@pytest.mark.parametrize('scene,nx,ny', [('s34', 24, 20), ('s978', 40, 24)])
def test_strict_list_pass_is_the_path_engines(fresh, scene, nx, ny, dilate):
    from ptina_amd.sampling.sobol import SobolSampler
    eng, F0, M0 = _prefix(scene, nx, ny, 'strict')
    e, valid = noise_map(F0, M0)
    t = float(np.sort(e[valid])[valid.sum() // 2])
    st, count = _film().select(t, dilate)
    noise = _film().get_noise(t)
    assert _stats(st) == _stats(noise)
    L = adaptive_ref.select(F0, M0, nx, ny, t, dilate)
    assert 0 < count < nx * ny and count == L.size
    got = _film().get_selection()
    assert np.array_equal(got, adaptive_ref.device_order(L, ny)) and np.array_equal(np.sort(got), L)
    aux = [_film().get_raw(1).copy(), _film().get_raw(2).copy()]
    assert _same(_film().get_raw(), F0) and _same(_film().get_mark(), M0)     # a selection writes neither film nor mark
    eng.render_selected(3, remark=True)
    F1, M1 = _film().get_raw().copy(), _film().get_mark().copy()
    sob_a = SobolSampler().state()
    assert _same(_film().get_raw(1), aux[0]) and _same(_film().get_raw(2), aux[1])
    assert np.array_equal(_film().get_selection(), got)                         # ... and a list pass keeps the selection
    eng_b, F0b, M0b = _prefix(scene, nx, ny, 'strict')
    assert _same(F0b, F0) and _same(M0b, M0)
    eng_b.render(3)
    FB = _film().get_raw().copy()
    sob_b = SobolSampler().state()
    off = np.ones(nx * ny, bool)
    off[L] = False
    assert _same(F1[L], FB[L]), f'{int((F1[L] != FB[L]).any(axis=1).sum())} of {L.size} listed pixels differ from the PathEngine'
    assert _same(F1[off], F0[off]) and _same(M1[L], F0[L]) and _same(M1[off], M0[off])
    assert np.all(F1[L, 3] == 11) and np.all(F1[off, 3] == 8)
    assert sob_a[0] == sob_b[0] and np.array_equal(sob_a[1], sob_b[1]) and _same(sob_a[2], sob_b[2])


# ---------------------------------------------------------------- 3. both builds: every sample is the path door's
def _door_vectors(nx, ny):
    '''the 32 draws of every pixel's path in the frame just rendered, as tests/test_mlt_gpu.py::test_path_door_equals_path_engine
    builds them (nx and ny are powers of two: (i + dx) / nx is the same f32 however the build divides)'''
    from ptina_amd.sampling import wanghash2
    from ptina_amd.sampling.sobol import SobolSampler
    _, _, P = SobolSampler().state()
    dim = P.shape[0]
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    h = wanghash2(i, j).astype(np.int64).reshape(-1, 1)
    k = np.arange(32, dtype=np.int64)[None, :]
    idx = ((h + k + 2**31) % 2**32 - 2**31) % dim
    X = P[idx].astype(np.float32)
    X[:, 0] = (i.reshape(-1).astype(np.float32) + X[:, 0]) / np.float32(nx)
    X[:, 1] = (j.reshape(-1).astype(np.float32) + X[:, 1]) / np.float32(ny)
    return X


def _checkerboard_and_a_tile(nx, ny):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    mask = (i + j) % 2 == 0
    mask[16:32, 0:16] = True
    return mask


@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_list_pass_samples_are_the_path_doors(fresh, mode):
    from ptina_amd.engine.mltpath import mlt_trace
    nx = ny = 32
    eng = setup_engine(_scene('s978'), nx, ny, mode=mode)
    eng.render(2)
    mask = _checkerboard_and_a_tile(nx, ny)
    _film().set_selection(mask)
    L = np.flatnonzero(mask.ravel())
    assert np.array_equal(np.sort(_film().get_selection()), L) and 0 < L.size < nx * ny
    off = ~mask.ravel()
    for step in range(3):
        before = _film().get_raw().copy()
        eng.render_selected(1)
        after = _film().get_raw().copy()
        rgb = mlt_trace(_door_vectors(nx, ny)[L])
        want = before[L, :3] + rgb                                            # one f32 add per channel
        assert _same(after[L, :3], want), f'step {step}: {int((after[L, :3] != want).any(axis=1).sum())} of {L.size} listed pixels differ'
        assert np.all(after[L, 3] == before[L, 3] + 1) and _same(after[off], before[off])
        assert np.any(rgb > 0)


# ---------------------------------------------------------------- 4. the split into launches does not show
def _twin(scene, nx, ny, mode, mask, **caps):
    from ptina_amd import common
    common.reset_all()
    eng = setup_engine(_scene(scene), nx, ny, mode=mode, **caps)
    eng.render(1)
    _film().set_selection(mask)
    return eng


@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_frames_in_one_call_or_many_give_the_same_film(fresh, mode):
    MAX_BATCH = 64                                                            # MPT_MAX_BATCH, frames per launch (csrc/mpt_types.h)
    nx, ny = 40, 24
    mask = np.random.default_rng(4).random((nx, ny)) < 0.4
    for frames in (5, MAX_BATCH + 6):                                         # ... and a call the library itself splits
        eng = _twin('s978', nx, ny, mode, mask)
        eng.render_selected(frames)
        one = _film().get_raw().copy()
        eng = _twin('s978', nx, ny, mode, mask)
        for _ in range(frames):
            eng.render_selected(1)
        many = _film().get_raw().copy()
        assert _same(one, many) and np.all(one[mask.ravel(), 3] == 1 + frames) and np.all(one[~mask.ravel(), 3] == 1)


def test_a_call_that_crosses_the_sample_buffer_cap(fresh):
    '''256 x 256 pixels listed x 64 frames x 16 bytes is the 64 MiB a launch's samples must stay under: the call is split'''
    nx = ny = 256
    mask = np.ones((nx, ny), bool)
    eng = _twin('s978', nx, ny, 'fast', mask)
    eng.render_selected(64)
    one = _film().get_raw().copy()
    ms = _film().adapt_kernel_time()
    eng = _twin('s978', nx, ny, 'fast', mask)
    for _ in range(64):
        eng.render_selected(1)
    many = _film().get_raw().copy()
    report(f'list pass 256x256 x 64 frames in one call: {ms[1]:.3f} ms')
    assert _same(one, many) and np.all(one[:, 3] == 65)


# ---------------------------------------------------------------- 5. the loop is the restatement (strict build)
_R = {}


def _strict_frames(n, nx=32, ny=32):
    '''R[f] = the strict build's raw film of frame f alone on a fresh context (the Sobol sampler runs on across clear)'''
    if 'R' not in _R:
        from ptina_amd import common
        common.reset_all()
        eng = setup_engine(_scene('s34'), nx, ny, mode='strict')
        R = np.empty((n, nx * ny, 4), f32)
        for f in range(n):
            _film().clear()
            eng.render(1)
            R[f] = _film().get_raw()
        R.setflags(write=False)
        _R['R'] = R
        common.reset_all()
    return _R['R']


def _history(r):
    return [(level, st.valid, st.above, active, kind) for level, st, active, kind in r.history]


@pytest.mark.parametrize('dilate,switch', [(0, 1.0), (1, 1.0), (1, 0.5)])
def test_the_loop_is_the_restatement(fresh, dilate, switch):
    nx = ny = 32
    R = _strict_frames(256)
    want = adaptive_ref.run_loop(R, nx, ny, 0.1, 256, min_spp=2, fraction=0.0, dilate=dilate, switch=switch)
    eng = setup_engine(_scene('s34'), nx, ny, mode='strict')
    r = eng.render_adaptive(0.1, 256, min_spp=2, fraction=0.0, dilate=dilate, switch=switch)
    report(f'render_adaptive strict s34 32x32 dilate {dilate} switch {switch}: {_history(r)}, {r.samples} samples = '
           f'{r.samples / (r.spp * nx * ny):.3f} of {r.spp} spp everywhere')
    F, M = _film().get_raw().copy(), _film().get_mark().copy()
    assert _history(r) == want.history and (r.spp, r.converged, r.samples) == (want.spp, want.converged, want.samples)
    assert _same(F, want.film) and _same(M, want.mark)
    assert isinstance(r.samples, int) and r.samples == int(_film().get_samples().astype(np.int64).sum())
    # what does not hang on the strict build's libm
    assert r.converged and 4 < r.spp <= 256 and r.samples < 0.5 * r.spp * nx * ny
    kinds = [h[3] for h in r.history]
    if switch == 0.5:
        assert kinds[1] == 'full' and 'list' in kinds[2:]
    else:
        assert kinds[0] == 'full' and all(k == 'list' for k in kinds[1:])
    # the worker's entry on a fresh context: the same film and history
    from ptina_amd import common
    import ptina_amd.worker as worker
    common.reset_all()
    setup_engine(_scene('s34'), nx, ny, mode='strict')
    w = worker.render_adaptive(0.1, 256, min_spp=2, fraction=0.0, dilate=dilate, switch=switch)
    assert _history(w) == _history(r) and w.samples == r.samples and _same(_film().get_raw(), F) and _same(_film().get_mark(), M)


# ---------------------------------------------------------------- 6. fast build: properties
def test_fast_build_loop_properties(fresh):
    from ptina_amd import common
    nx = ny = 32
    films = []
    for _ in range(2):
        common.reset_all()
        eng = setup_engine(_scene('s34'), nx, ny, mode='fast')
        r = eng.render_adaptive(0.1, 256, min_spp=2, fraction=0.0, dilate=1, switch=0.5)
        films.append(_film().get_raw().copy())
    report(f'render_adaptive fast s34 32x32: {_history(r)}, {r.samples} samples')
    assert r.converged
    st = _film().get_noise(0.1)
    assert st.above <= 0.0 * st.valid and st.valid == nx * ny
    w = _film().get_samples()
    assert w.shape == (nx, ny) and w.dtype == f32 and w.max() <= r.spp and r.samples == int(w.astype(np.int64).sum())
    img = _film().get_denoised(variance=4)
    assert img.shape == (nx, ny, 4) and np.isfinite(img).all()
    assert _same(films[0], films[1])


# ---------------------------------------------------------------- 7. a slab
@pytest.mark.parametrize('dilate', [0, 1])
def test_a_slab_lists_and_renders_only_its_own_columns(fresh, dilate):
    nx, ny = 56, 24
    eng = setup_engine(_scene('s978'), nx, ny, mode='fast', slab=(16, 40))
    r = eng.render_adaptive(0.05, 32, min_spp=2, dilate=dilate, switch=1.0)
    assert len(r.history) >= 3 and r.history[0][1].valid == 24 * ny
    F = _film().get_raw().reshape(nx, ny, 4)
    assert not F[:16].any() and not F[40:].any() and np.all(F[16:40, :, 3] >= 4)
    # a selection with everything above: the whole slab, and neither column 15 nor column 40
    st, count = _film().select(0.0, dilate)
    cols = _film().get_selection() // ny
    assert count == cols.size > 0 and cols.min() >= 16 and cols.max() <= 39
    assert st.above > 0 and (dilate == 0 or (cols == 16).any() and (cols == 39).any())
    before = _film().get_selection()
    with pytest.raises(RuntimeError, match='column 15'):
        _film().set_selection(np.array([15 * ny + 3, 16 * ny], np.int32))
    with pytest.raises(RuntimeError, match='column 40'):
        _film().set_selection(np.array([16 * ny, 40 * ny], np.int32))
    assert np.array_equal(_film().get_selection(), before)
    _film().set_selection(np.array([16 * ny, 39 * ny + ny - 1], np.int32))
    eng.render_selected(2)
    G = _film().get_raw().reshape(nx, ny, 4)
    assert not G[:16].any() and not G[40:].any() and G[16, 0, 3] == F[16, 0, 3] + 2 and G[39, ny - 1, 3] == F[39, ny - 1, 3] + 2


# ---------------------------------------------------------------- 8. every stated error
def test_every_stated_error(fresh):
    from ptina_amd._lib import NoiseStats
    nx, ny = 24, 20
    eng = setup_engine(_scene('s34'), nx, ny, mode='fast')
    c, film = _ctx(), _film()
    eng.render(2)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))

    def state():
        try:
            sel = film.get_selection()
        except RuntimeError:
            sel = None
        try:
            mark = film.get_mark().copy()
        except RuntimeError:
            mark = None
        return film.get_raw().copy(), mark, sel

    def refused(match, fn, exc=RuntimeError):
        before = state()
        with pytest.raises(exc, match=match):
            fn()
        after = state()
        assert _same(before[0], after[0])
        assert (before[1] is None) == (after[1] is None) and (before[1] is None or _same(before[1], after[1]))
        assert (before[2] is None) == (after[2] is None) and (before[2] is None or np.array_equal(before[2], after[2]))

    # no mark, no selection
    refused('mpt_adapt_select: no mark', lambda: film.select(0.1))
    refused('no selection', lambda: eng.render_selected(1))
    refused('no selection', lambda: film.get_selection())
    film.set_selection(np.arange(0, nx * ny, 3))
    refused('mpt_render_selected: no mark', lambda: eng.render_selected(1, remark=True))
    film.mark()
    eng.render(2)
    film.select(0.05, 1)
    # thresholds, dilate
    for bad in (-0.1, float('nan'), float('inf')):
        refused('mpt_adapt_select: threshold must be finite and not negative', lambda: film.select(bad))
        refused('mpt_adapt_eval: threshold must be finite and not negative',
                lambda: c.adapt_eval(np.zeros((4, 4), f32), np.zeros((4, 4), f32), 2, 2, bad))
    for bad in (-1, 2):
        refused('dilate must be 0 or 1', lambda: film.select(0.1, bad))
        refused('dilate must be 0 or 1', lambda: c.adapt_eval(np.zeros((4, 4), f32), np.zeros((4, 4), f32), 2, 2, 0.1, bad))
    # lists
    refused('entry 2 = 5 after 5: the list must be strictly ascending', lambda: film.set_selection(np.array([1, 5, 5, 9])))
    refused('entry 1 = 2 after 7', lambda: film.set_selection(np.array([7, 2])))
    refused('entry 0 = -1 outside', lambda: film.set_selection(np.array([-1, 2])))
    refused('entry 1 = %d outside' % (nx * ny), lambda: film.set_selection(np.array([0, nx * ny])))
    refused('the mask is', lambda: film.set_selection(np.zeros((ny, nx + 1), bool)), ValueError)
    refused('nframes must be >= 0', lambda: eng.render_selected(-1))
    # null pointers, a list too long for its room
    n = C.c_int(0)
    st = NoiseStats()
    refused('null list$', lambda: c.call('mpt_adapt_set_list', None, 3))
    refused('null list and null count', lambda: c.call('mpt_adapt_get_list', None, 0, None))
    have = film.get_selection().size
    assert have > 1
    small = np.zeros(have - 1, np.int32)
    refused('room for %d indices, the selection holds %d' % (have - 1, have), lambda: c.call('mpt_adapt_get_list', ip(small), have - 1, C.byref(n)))
    z = np.zeros((4, 4), f32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    refused('mpt_adapt_eval: null input', lambda: c.call('mpt_adapt_eval', 0.1, 1, None, fp(z), 2, 2, None, 0, C.byref(n), C.byref(st)))
    refused('mpt_adapt_eval: null input', lambda: c.call('mpt_adapt_eval', 0.1, 1, fp(z), None, 2, 2, None, 0, C.byref(n), C.byref(st)))
    refused('mpt_adapt_eval: null outputs', lambda: c.call('mpt_adapt_eval', 0.1, 1, fp(z), fp(z), 2, 2, None, 0, None, None))
    refused('mpt_adapt_eval: film 0x2', lambda: c.call('mpt_adapt_eval', 0.1, 1, fp(z), fp(z), 0, 2, None, 0, C.byref(n), None))
    Fs, Ms = synthetic_pair(3, 8, 8, invalid=0.0)
    refused('mpt_adapt_eval: room for 1 indices', lambda: c.call('mpt_adapt_eval', 0.0, 1, fp(Fs), fp(Ms), 8, 8, ip(small), 1, C.byref(n), None))
    # the loop's arguments
    refused('switch must be in', lambda: eng.render_adaptive(0.1, 64, switch=1.5), ValueError)
    refused('switch must be in', lambda: eng.render_adaptive(0.1, 64, switch=-0.5), ValueError)
    refused('max_spp must be at least 2 \\* min_spp', lambda: eng.render_adaptive(0.1, 31), ValueError)
    refused('dilate must be 0 or 1', lambda: eng.render_adaptive(0.1, 64, dilate=3), ValueError)
    # a camera change keeps the selection; clear() and set_size() drop it (and the mark)
    from ptina_amd.things import Camera
    from ptina_amd import scenes
    sel = film.get_selection()
    Camera().set_perspective(scenes.BENCH_CAMERA)
    assert np.array_equal(film.get_selection(), sel)
    eng.render_selected(1)
    film.clear()
    with pytest.raises(RuntimeError, match='no selection'):
        eng.render_selected(1)
    film.set_selection(np.array([3, 4]))
    film.set_size(nx, ny)
    with pytest.raises(RuntimeError, match='no selection'):
        film.get_selection()
    # an empty selection is a selection: nothing is launched, the sampler still advances
    from ptina_amd.sampling.sobol import SobolSampler
    film.set_selection(np.zeros(0, np.int32))
    t0, raw = SobolSampler().state()[0], film.get_raw().copy()
    eng.render_selected(3)
    assert SobolSampler().state()[0] == t0 + 3 and _same(film.get_raw(), raw) and film.get_selection().size == 0


def test_the_kernel_timer_reports_one_span_per_call(fresh):
    nx, ny = 24, 20
    eng = setup_engine(_scene('s34'), nx, ny, mode='fast')
    film = _film()
    eng.render(2)
    film.mark()
    eng.render(2)
    assert film.adapt_kernel_time() == (0.0, 0.0, 0)
    film.select(0.0, 1)
    select_ms, render_ms, n = film.adapt_kernel_time()
    assert n == 1 and select_ms > 0 and render_ms == 0
    eng.render_selected(2)
    eng.render_selected(70)                                                   # (two launches, one span)
    select_ms, render_ms, n = film.adapt_kernel_time()
    assert n == 2 and render_ms > 0 and select_ms == 0
    _ctx().adapt_eval(*synthetic_pair(1, 8, 8), 8, 8, 0.1)                    # the test door is not timed
    assert film.adapt_kernel_time() == (0.0, 0.0, 0)


# ---------------------------------------------------------------- 9. the exam script
def test_adaptive_exam_script(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'exams', 'adaptive_amd.py'), '--size', '64', '--noise', '0.1', '--min-spp', '4',
                        '--max-spp', '128', '--out', str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'render_until:' in r.stdout and 'render_adaptive:' in r.stdout
    for name in ('adaptive.png', 'sample_count.png'):
        assert (tmp_path / name).stat().st_size > 100 and (tmp_path / name).read_bytes()[:8] == b'\x89PNG\r\n\x1a\n'

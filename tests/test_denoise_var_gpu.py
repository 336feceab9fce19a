'''
GPU tests (-m gpu) of the variance-guided mode of the denoised read-backs (FilmTable.get_denoised(variance=...),
mpt_denoise_set_variance, mpt_denoise_eval; ptina_amd/csrc/denoise.hip) and of render_until(keep_mark=True).

Parity is the door (mpt_denoise_eval: the read-backs' own launches on the caller's accumulators) against tests/denoise_var_ref.py
(held to its definition by tests/test_denoise_var_cpu.py), by the rule of tests/test_denoise_gpu.py: with d = max |ref32 - ref64| /
(1 + |ref64|) on the same film -- what f32 arithmetic alone does to the filter there -- the GPU must stay within max(8 d, one f32
ulp) of ref64; the propagated variance likewise, on the scale of the film's median variance instead of 1.  The public path is then
held to the door bit for bit.  Measured on an MI355X: see DESIGN.md section 3.9.1.
'''

import numpy as np
import pytest

from helpers import setup_engine, report
from denoise_ref import MARKER
from denoise_var_ref import denoise_var_ref, random_film

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SIGMA = 4.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _scene(name):
    from ptina_amd import scenes
    return scenes.get_scene(name)


def _film():
    from ptina_amd.things import FilmTable
    return FilmTable()


def _ctx():
    from ptina_amd.common import ctx
    return ctx()


def _render_marked(scene, nx, ny, slab=None):
    '''4 frames, a mark, 4 frames more, 2 preview frames'''
    from ptina_amd.engine.preview import PreviewEngine
    eng = setup_engine(_scene(scene), nx, ny, slab=slab)
    eng.render(4)
    _film().mark()
    eng.render(4)
    PreviewEngine().render(2)
    return eng


def _state():
    '''the three passes and the mark, as the context holds them'''
    film = _film()
    return [film.get_raw(p).copy() for p in range(3)] + [film.get_mark().copy()]


# ---------------------------------------------------------------- 1. parity of the door with the restatement
@pytest.mark.parametrize('nx,ny', [(1, 1), (1, 70), (70, 1), (9, 65), (37, 29), (130, 70)])
def test_door_parity_on_synthetic_films(fresh, nx, ny):
    '''9x65 is one past the LDS tile both ways; 8 iterations at 37x29 put the stride beyond the film; a fifth of the pixels are not
    valid, lack a group or have no guides'''
    from ptina_amd.things import init_things
    init_things()
    film = random_film(1000 * nx + ny, nx, ny)
    valid = film[0].reshape(nx, ny, 4)[..., 3] != 0
    worst = [0.0, 0.0]
    for iterations in (1, 3, 5, 8):
        for demodulate in (True, False):
            kw = dict(iterations=iterations, demodulate=demodulate)
            got, gv = _ctx().denoise_eval(*film, nx, ny, variance=SIGMA, var=True, **kw)
            assert got.shape == (nx, ny, 4) and got.dtype == np.float32 and gv.shape == (nx, ny) and gv.dtype == np.float32
            r64, v64 = denoise_var_ref(*film, nx, ny, SIGMA, dtype=np.float64, **kw)
            r32, v32 = denoise_var_ref(*film, nx, ny, SIGMA, dtype=np.float32, **kw)
            d = float((np.abs(r32.astype(np.float64) - r64) / (1 + np.abs(r64))).max())
            err = float((np.abs(got.astype(np.float64) - r64) / (1 + np.abs(r64))).max())
            med = float(np.median(v64[valid])) if valid.any() else 1.0
            dv = float((np.abs(v32.astype(np.float64) - v64) / (med + np.abs(v64))).max())
            errv = float((np.abs(gv.astype(np.float64) - v64) / (med + np.abs(v64))).max())
            report(f'denoise variance door {nx}x{ny} {kw}: image d = {d:.3e}, GPU vs ref64 {err:.3e} = {err / d if d > 0 else 0.0:.2f} d; '
                   f'variance (median {med:.3e}) d = {dv:.3e}, GPU vs ref64 {errv:.3e} = {errv / dv if dv > 0 else 0.0:.2f} d')
            worst = [max(worst[0], err / max(d, ULP / 8)), max(worst[1], errv / max(dv, ULP / 8))]
            assert np.isfinite(got).all() and np.isfinite(gv).all()
            assert np.array_equal(got[~valid], np.tile(np.float32(MARKER), (int((~valid).sum()), 1)))
            assert np.all(got[valid][:, 3] == 1) and np.all(gv[~valid] == 0) and np.all(gv >= 0)
            assert err <= max(8 * d, ULP), f'{nx}x{ny} {kw}: image {err:.3e} exceeds max(8 d, ulp) = {max(8 * d, ULP):.3e}'
            assert errv <= max(8 * dv, ULP), f'{nx}x{ny} {kw}: variance {errv:.3e} exceeds max(8 d, ulp) = {max(8 * dv, ULP):.3e}'
    report(f'denoise variance door {nx}x{ny}: worst image {worst[0]:.2f} d, worst variance {worst[1]:.2f} d')


def test_door_without_variance_is_the_fixed_filter_and_zero_iterations_the_resolve(fresh):
    '''sigma_variance = 0 through the door is get_denoised's filter on a film of the caller's; iterations = 0 resolves, guided or not,
    and hands out v_0'''
    from denoise_ref import denoise_ref
    from ptina_amd.things import init_things
    init_things()
    nx, ny = 37, 29
    film = random_film(5, nx, ny)
    got = _ctx().denoise_eval(*film[:3], None, nx, ny)
    r64, r32 = (denoise_ref(*film[:3], nx, ny, dtype=t) for t in (np.float64, np.float32))
    d = float((np.abs(r32.astype(np.float64) - r64) / (1 + np.abs(r64))).max())
    assert float((np.abs(got.astype(np.float64) - r64) / (1 + np.abs(r64))).max()) <= max(8 * d, ULP)
    img, v0 = _ctx().denoise_eval(*film, nx, ny, variance=SIGMA, var=True, iterations=0)
    r32, v32 = denoise_var_ref(*film, nx, ny, SIGMA, iterations=0, dtype=np.float32)
    assert _same(img, r32) and _same(v0, v32)                    # (correctly rounded operations only: equal, not close)
    assert _same(img, _ctx().denoise_eval(*film[:3], None, nx, ny, iterations=0))


# ---------------------------------------------------------------- 2. the two stencil kernels
def test_guided_lds_and_gather_kernels_give_the_same_bits(fresh):
    from ptina_amd.things import init_things
    init_things()
    nx, ny = 130, 70
    film = random_film(7, nx, ny)
    assert _ctx().get_option('denoise_lds') == 1
    a, va = _ctx().denoise_eval(*film, nx, ny, variance=SIGMA, var=True)
    _ctx().set_option('denoise_lds', 0)
    b, vb = _ctx().denoise_eval(*film, nx, ny, variance=SIGMA, var=True)
    assert _same(a, b) and _same(va, vb)
    assert np.count_nonzero(va) > 0.7 * nx * ny


# ---------------------------------------------------------------- 3. the public path is the door
def test_public_path_is_the_door_bit_for_bit(fresh):
    import ptina_amd.worker as worker
    nx, ny = 37, 29
    _render_marked('s34', nx, ny)
    film, c = _film(), _ctx()
    before = _state()
    assert np.all(before[0][:, 3] == 8) and np.all(before[3][:, 3] == 4) and np.all(before[1][:, 3] == 2)
    fixed = film.get_denoised().copy()
    for kw in (dict(), dict(iterations=2, demodulate=False), dict(iterations=8, sigma_albedo=0.3)):
        got = film.get_denoised(variance=SIGMA, **kw).copy()
        assert _same(got, c.denoise_eval(*before, nx, ny, variance=SIGMA, **kw)), kw
        assert _same(got, worker.get_denoised(variance=SIGMA, **kw))
        for dkw in (dict(), dict(layout='display', op='reinhard', exposure=0.5)):
            want, E = c.display_eval(got.reshape(-1, 4), nx, ny, **dkw)
            assert np.array_equal(film.get_display(denoised=True, variance=SIGMA, **dkw, **kw), want), (kw, dkw)
            assert np.float32(film.last_exposure) == E
            assert np.array_equal(worker.get_display(denoised=True, variance=SIGMA, **dkw, **kw), want)
    assert not _same(film.get_denoised(variance=SIGMA), fixed)   # (the mode does something on a rendered film)
    assert _same(film.get_denoised(variance=SIGMA, iterations=0), film.get_image(0))
    # variance=None afterwards: the fixed filter, and the state the Python callers never see is back at 0
    assert _same(film.get_denoised(), fixed) and c.get_denoise_variance() == 0.0
    assert _same(film.get_denoised(variance=0), fixed)
    film.get_display(denoised=True, variance=SIGMA)
    assert np.array_equal(film.get_display(denoised=True), c.display_eval(fixed.reshape(-1, 4), nx, ny)[0])
    for a, b in zip(before, _state()):
        assert _same(a, b)


def test_guided_filter_on_a_slab_is_the_door_on_its_columns(fresh):
    '''a context that renders columns [16, 40) of a 64x24 film: the rest is not valid, and nothing leaks across'''
    nx, ny = 64, 24
    _render_marked('s34', nx, ny, slab=(16, 40))
    state = _state()
    w = state[0].reshape(nx, ny, 4)[..., 3]
    assert np.all(w[16:40] == 8) and not w[:16].any() and not w[40:].any()
    got = _film().get_denoised(variance=SIGMA)
    assert np.all(got[:16] == np.float32(MARKER)) and np.all(got[40:] == np.float32(MARKER))
    cut = [r.reshape(nx, ny, 4)[16:40].reshape(-1, 4) for r in state]
    assert _same(got[16:40], _ctx().denoise_eval(*cut, 24, ny, variance=SIGMA))


# ---------------------------------------------------------------- 4. every stated error
def test_every_stated_error_raises_and_leaves_film_mark_and_setting(fresh):
    import ctypes as C
    from ptina_amd.engine.preview import PreviewEngine
    nx, ny = 16, 16
    eng = setup_engine(_scene('s34'), nx, ny)
    film, c = _film(), _ctx()
    eng.render(2)
    PreviewEngine().render(1)
    from ptina_amd._lib import display_params, denoise_params, DISPLAY_DENOISED
    fp = C.POINTER(C.c_float)
    raws = [film.get_raw(p).copy() for p in range(3)]
    out, out8 = np.empty((nx, ny, 4), np.float32), np.empty((nx, ny, 4), np.uint8)
    for call in (lambda: film.get_denoised(variance=SIGMA), lambda: film.get_denoised(variance=SIGMA, iterations=0),
                 lambda: film.get_display(denoised=True, variance=SIGMA)):
        with pytest.raises(RuntimeError, match='no mark'):                      # no mark yet
            call()
    # (the Python calls set the value they are given first; the C calls behind them leave the setting alone)
    c.set_denoise_variance(2.5)
    for it in (5, 0):
        with pytest.raises(RuntimeError, match='mpt_get_denoised: no mark'):
            c.call('mpt_get_denoised', C.byref(denoise_params(iterations=it)), out.ctypes.data_as(fp))
    with pytest.raises(RuntimeError, match='mpt_get_display: no mark'):
        c.call('mpt_get_display', C.byref(display_params(DISPLAY_DENOISED)), None, out8.ctypes.data_as(C.POINTER(C.c_uint8)), None)
    assert c.get_denoise_variance() == 2.5
    for p in range(3):
        assert _same(film.get_raw(p), raws[p])
    film.get_denoised()                                                         # (the fixed filter needs no mark)
    film.mark()
    eng.render(2)
    before = _state()
    want = film.get_denoised(variance=SIGMA).copy()
    c.set_denoise_variance(2.5)
    for bad in (-1.0, -1e-30, float('nan'), float('inf'), float('-inf')):
        for call in (lambda: film.get_denoised(variance=bad), lambda: film.get_display(denoised=True, variance=bad),
                     lambda: c.denoise_eval(*before, nx, ny, variance=bad)):
            with pytest.raises(RuntimeError, match='sigma_variance must be finite and not negative'):
                call()
        assert c.get_denoise_variance() == 2.5
    with pytest.raises(TypeError, match='only apply with denoised=True'):
        film.get_display(variance=SIGMA)
    with pytest.raises(RuntimeError, match='sigma_color must be finite and positive'):      # validated, though not used
        film.get_denoised(variance=SIGMA, sigma_color=0)
    with pytest.raises(RuntimeError, match='mark must be given'):
        c.denoise_eval(*before[:3], None, nx, ny, variance=SIGMA)
    with pytest.raises(RuntimeError, match='mark must be given'):
        c.denoise_eval(*before, nx, ny)
    with pytest.raises(RuntimeError, match='var_out needs'):
        c.denoise_eval(*before[:3], None, nx, ny, var=True)
    with pytest.raises(RuntimeError, match='null output'):
        c.call('mpt_denoise_get_variance', None)
    ptr = [a.ctypes.data_as(fp) for a in before]
    with pytest.raises(RuntimeError, match='null input'):
        c.call('mpt_denoise_eval', None, 0.0, ptr[0], None, ptr[2], None, nx, ny, out.ctypes.data_as(fp), None)
    for bx, by in ((0, 4), (4, 0), (-1, 4), (2 ** 15, 2 ** 15)):
        with pytest.raises(RuntimeError, match='max_filmsize'):
            c.call('mpt_denoise_eval', None, 0.0, ptr[0], ptr[1], ptr[2], None, bx, by, out.ctypes.data_as(fp), None)
    for a, b in zip(before, _state()):
        assert _same(a, b)
    assert _same(film.get_denoised(variance=SIGMA), want)                       # (the context is still good)
    # clear() drops the mark, and the guided read-backs say so; the fixed ones go on
    film.clear()
    eng.render(2)
    with pytest.raises(RuntimeError, match='no mark'):
        film.get_denoised(variance=SIGMA)
    assert c.get_denoise_variance() == np.float32(SIGMA)
    film.get_denoised()


# ---------------------------------------------------------------- 5. render_until leaves a mark to filter by
def test_render_until_keep_mark_is_the_same_render_and_leaves_the_last_mark(fresh):
    from ptina_amd import common
    from ptina_amd.engine.preview import PreviewEngine
    import ptina_amd.worker as worker
    nx, ny = 32, 32
    eng = setup_engine(_scene('s34'), nx, ny)
    r = eng.render_until(0.0, 20, min_spp=4)
    assert (r.spp, r.converged) == (20, False)
    want = _film().get_raw(0).copy()
    assert np.all(_film().get_mark()[:, 3] == 20)                               # the last check re-marked: no second group is left
    common.reset_all()
    setup_engine(_scene('s34'), nx, ny)
    k = worker.render_until(0.0, 20, min_spp=4, keep_mark=True)
    assert (k.spp, k.converged) == (r.spp, r.converged)
    assert [(s, st.valid, st.above, st.sum, st.max) for s, st in k.history] == [(s, st.valid, st.above, st.sum, st.max) for s, st in r.history]
    assert _same(_film().get_raw(0), want)
    assert np.all(_film().get_mark()[:, 3] == 16)                               # the sample count before the last batch
    PreviewEngine().render(1)
    state = _state()
    got = _film().get_denoised(variance=SIGMA)
    assert _same(got, _ctx().denoise_eval(*state, nx, ny, variance=SIGMA)) and np.all(got[..., 3] == 1)
    # a run that converges at its first check keeps the mark of min_spp samples
    common.reset_all()
    eng = setup_engine(_scene('s34'), nx, ny)
    from ptina_amd.engine import render_until
    k = render_until(eng, 1e9, 64, min_spp=2, keep_mark=True)
    assert (k.spp, k.converged) == (4, True) and np.all(_film().get_mark()[:, 3] == 2)

'''
GPU tests (-m gpu) of FilmTable.get_denoised (mpt_get_denoised; ptina_amd/csrc/denoise.hip): the edge-avoiding A-Trous filter of
film pass 0 guided by the albedo and normal passes.

Parity is against tests/denoise_ref.py (held to its definition by tests/test_denoise_cpu.py) fed with the very accumulators the
context holds (get_raw(0..2)), on |gpu - ref64| / (1 + |ref64|).  The bound is measured, not chosen: d = max |ref32 - ref64| /
(1 + |ref64|) on the same film is what f32 arithmetic alone does to this filter there, and the GPU must stay within 8 d (two
independent f32 roundings plus two exp implementations 1-2 ulp apart, and the freedom in the order of the 25 taps).
Measured on an MI355X: see DESIGN.md section 3.9.
'''

import numpy as np
import pytest

from helpers import setup_engine, report
from denoise_ref import denoise_ref, MARKER, DEFAULTS

pytestmark = pytest.mark.gpu

VARIANTS = [{}, {'demodulate': False}, {'iterations': 1}, {'iterations': 3}, {'iterations': 8}, {'sigma_color': 0.5}]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scene(name):
    from ptina_amd import scenes
    return scenes.get_scene(name)


def _render(scene, nx, ny, frames, preview, slab=None):
    '''a fresh context with `frames` path frames in pass 0 and `preview` preview frames in passes 1 and 2'''
    from ptina_amd.engine.preview import PreviewEngine
    eng = setup_engine(_scene(scene), nx, ny, slab=slab)
    if frames:
        eng.render(frames)
    if preview:
        PreviewEngine().render(preview)
    return eng


def _raws():
    from ptina_amd.things import FilmTable
    return [FilmTable().get_raw(p).copy() for p in range(3)]


def _parity(what, nx, ny, raws, mask=None, **kw):
    '''get_denoised(**kw) of the current context against the restatement on `raws`; returns the GPU image'''
    from ptina_amd.things import FilmTable
    got = FilmTable().get_denoised(**kw)
    assert got.shape == (nx, ny, 4) and got.dtype == np.float32
    ref64 = denoise_ref(*raws, nx, ny, **{**DEFAULTS, **kw}, dtype=np.float64)
    ref32 = denoise_ref(*raws, nx, ny, **{**DEFAULTS, **kw}, dtype=np.float32)
    d = float((np.abs(ref32.astype(np.float64) - ref64) / (1 + np.abs(ref64))).max())
    err = np.abs(got.astype(np.float64) - ref64) / (1 + np.abs(ref64))
    worst = np.unravel_index(int(err.argmax()), err.shape)
    report(f'denoise {what} {kw or "defaults"}: d = max|ref32 - ref64|/(1+|ref64|) = {d:.3e}; GPU vs ref64 {float(err.max()):.3e} '
           f'= {float(err.max()) / d if d > 0 else 0.0:.2f} d at pixel {worst[:2]} channel {worst[2]}')
    assert np.isfinite(got).all()
    valid = raws[0].reshape(nx, ny, 4)[..., 3] != 0
    assert np.array_equal(got[~valid], np.tile(np.float32(MARKER), (int((~valid).sum()), 1)))
    assert np.all(got[valid][:, 3] == 1)
    assert float(err.max()) <= 8 * d, f'{what} {kw}: GPU {float(err.max()):.3e} exceeds 8 d = {8 * d:.3e} at {worst}'
    return got


# ---------------------------------------------------------------- 1. parity with the restatement
@pytest.mark.parametrize('scene,nx,ny', [('s978', 48, 40), ('s34', 37, 29)])
def test_parity_small_films(fresh, scene, nx, ny):
    '''no multiple of any tile, and smaller than the last iterations' reach: most of their taps fall outside the film'''
    _render(scene, nx, ny, 4, 2)
    raws = _raws()
    assert np.all(raws[0][:, 3] == 4) and np.all(raws[1][:, 3] == 2)
    for kw in VARIANTS:
        _parity(f'{scene} {nx}x{ny}', nx, ny, raws, **kw)


def test_parity_many_tiles_ragged(fresh):
    _render('s34', 130, 70, 1, 1)
    _parity('s34 130x70', 130, 70, _raws())


def test_parity_without_guides(fresh):
    '''no preview frame: passes 1 and 2 are empty and the filter is guided by colour alone -- defined, not an error'''
    _render('s978', 48, 40, 4, 0)
    raws = _raws()
    assert not raws[1].any() and not raws[2].any()
    _parity('s978 48x40 no guides', 48, 40, raws)
    _parity('s978 48x40 no guides', 48, 40, raws, demodulate=False)


def test_parity_slab(fresh):
    '''a context that renders columns [16, 40) of a 64x24 film: the rest is not valid, and nothing leaks across'''
    from ptina_amd.things import FilmTable
    nx, ny = 64, 24
    _render('s34', nx, ny, 4, 2, slab=(16, 40))
    raws = _raws()
    w = raws[0].reshape(nx, ny, 4)[..., 3]
    assert np.all(w[16:40] == 4) and not w[:16].any() and not w[40:].any()
    got = _parity('s34 64x24 slab 16..40', nx, ny, raws)
    assert np.all(got[:16] == np.float32(MARKER)) and np.all(got[40:] == np.float32(MARKER))
    # what lies outside the slab weighs nothing: the slab alone, cut out as a film of its own, filters to the same pixels
    cut = [r.reshape(nx, ny, 4)[16:40].reshape(-1, 4) for r in raws]
    alone = denoise_ref(*cut, 24, ny, dtype=np.float64)
    whole = denoise_ref(*raws, nx, ny, dtype=np.float64)
    assert np.array_equal(alone, whole[16:40])
    assert np.array_equal(_bits(FilmTable().get_raw(0)), _bits(raws[0]))


@pytest.mark.parametrize('nx,ny', [(1, 1), (1, 9), (9, 1)])
def test_parity_degenerate_films(fresh, nx, ny):
    _render('s34', nx, ny, 4, 2)
    _parity(f's34 {nx}x{ny}', nx, ny, _raws())


def test_lds_and_gather_kernels_give_the_same_bits(fresh):
    '''the strides 1 and 2 run from a tile in LDS, or as gathers like the larger ones (option "denoise_lds"): same arithmetic in
    the same order, so not one bit may differ'''
    from ptina_amd.common import ctx
    from ptina_amd.things import FilmTable
    _render('s34', 130, 70, 2, 1)
    assert ctx().get_option('denoise_lds') == 1
    a = FilmTable().get_denoised()
    ctx().set_option('denoise_lds', 0)
    b = FilmTable().get_denoised()
    assert np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------- 2. iterations = 0
def test_zero_iterations_is_get_image_bit_for_bit(fresh):
    from ptina_amd.things import FilmTable
    _render('s978', 48, 40, 3, 1, slab=(0, 41))
    a = FilmTable().get_denoised(iterations=0)
    b = FilmTable().get_image(0)
    assert np.array_equal(_bits(a), _bits(b))
    assert np.all(a[41:] == np.float32(MARKER)) and np.all(a[:41, :, 3] == 1)


# ---------------------------------------------------------------- 3. nothing existing moves
def test_film_passes_are_not_written_and_calls_repeat(fresh):
    from ptina_amd.things import FilmTable
    _render('s978', 48, 40, 4, 2)
    before = _raws()
    a = FilmTable().get_denoised()
    b = FilmTable().get_denoised()
    after = _raws()
    for p in range(3):
        assert np.array_equal(_bits(before[p]), _bits(after[p])), f'pass {p} changed'
    assert np.array_equal(_bits(a), _bits(b))
    assert a is not b


@pytest.mark.parametrize('read_between', [False, True])
def test_render_around_a_denoise_is_the_uninterrupted_render(fresh, read_between):
    '''render(2), get_denoised, render(2), get_image == render(4), get_image, bit for bit; PathEngine.render() hints the array of the
    next get_image(0) (mpt_hint_image), so the denoise runs between a hint and the call that spends it -- also with that
    get_image called right before and right after the denoise'''
    from ptina_amd import common
    from ptina_amd.things import FilmTable
    nx, ny = 48, 40
    _render('s978', nx, ny, 4, 0)
    want = FilmTable().get_image().copy()
    common.reset_all()
    _render('s978', nx, ny, 2, 0)
    two = FilmTable().get_image().copy()
    common.reset_all()
    eng = _render('s978', nx, ny, 0, 0)
    eng.render(2)
    if read_between:
        assert np.array_equal(_bits(FilmTable().get_image()), _bits(two))
    FilmTable().get_denoised()
    if read_between:
        assert np.array_equal(_bits(FilmTable().get_image()), _bits(two))
    eng.render(2)
    FilmTable().get_denoised(iterations=2)
    got = FilmTable().get_image()
    assert np.array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------- 4. it denoises
def test_denoised_image_is_closer_to_the_converged_one(fresh):
    '''mean squared error against this context's own 512-frame image: the filtered 4-frame image must beat the plain one'''
    from ptina_amd.things import FilmTable
    eng = _render('s978', 48, 40, 4, 2)
    noisy = FilmTable().get_image().copy()
    den = FilmTable().get_denoised().copy()
    eng.render(508)
    ref = FilmTable().get_image()
    assert np.all(FilmTable().get_raw(0)[:, 3] == 512)

    def mse(x):
        return float(((x[..., :3].astype(np.float64) - ref[..., :3]) ** 2).mean())
    report(f'denoise s978 48x40, 4 frames + 2 preview: mse noisy {mse(noisy):.4e}, denoised {mse(den):.4e}, ratio {mse(den) / mse(noisy):.3f}')
    assert mse(den) < mse(noisy)


# ---------------------------------------------------------------- 5. errors
def test_bad_parameters_raise_and_a_grown_film_works(fresh):
    from ptina_amd.things import FilmTable
    _render('s34', 16, 16, 1, 1)
    with pytest.raises(RuntimeError, match='iterations must be in 0..8'):
        FilmTable().get_denoised(iterations=9)
    with pytest.raises(RuntimeError, match='sigma_color must be finite and positive'):
        FilmTable().get_denoised(sigma_color=0)
    with pytest.raises(RuntimeError, match='sigma_normal must be finite and positive'):
        FilmTable().get_denoised(sigma_normal=float('nan'))
    with pytest.raises(RuntimeError, match='sigma_albedo must be finite and positive'):
        FilmTable().get_denoised(sigma_albedo=float('inf'))
    FilmTable().get_denoised()                                  # (the context is still good)
    from ptina_amd.common import ctx
    from ptina_amd.engine.path import PathEngine
    from ptina_amd.engine.preview import PreviewEngine
    import ctypes as C
    from ptina_amd._lib import DenoiseParams
    cap = ctx().caps.max_filmsize
    nx, ny = 300, 200
    assert 16 * 16 < nx * ny <= cap
    FilmTable().set_size(nx, ny)                                # the film and the filter's buffers are reallocated
    FilmTable().clear()
    PathEngine().render(1)
    PreviewEngine().render(1)
    _parity('s34 300x200 after set_size', nx, ny, _raws())
    import ptina_amd.worker as worker
    assert np.array_equal(_bits(worker.get_denoised(iterations=2)), _bits(FilmTable().get_denoised(iterations=2)))
    assert C.sizeof(DenoiseParams) == 20                        # mpt_denoise_params: five 4-byte fields, no padding

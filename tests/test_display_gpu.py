'''
GPU tests (-m gpu) of FilmTable.get_display (mpt_get_display; ptina_amd/csrc/display.hip): the film metered, tone-mapped,
transfer-encoded, dithered and quantised to 8-bit RGBA on the device.

Parity is against tests/display_ref.py (held to closed forms by tests/test_display_cpu.py) fed with the very accumulators the
context holds (get_raw), by the byte rule (display_ref.byte_rule): with u64 the f64 restatement's value in front of the floor, a
byte must be floor(u64); only where u64 lies within tau of an integer may it be the neighbour, never more than 1 off; tau = 8 d,
d = max |u32 - u64| of the f32 restatement on the same film -- measured per film, not chosen (two independent f32 roundings, pow /
log / exp implementations an ulp or two apart, the reduction's order).  The bytes so excused must be at most 1 % of a film's colour
bytes.  The exposure must be within 8 |E32 - E64| of E64, and never held tighter than one f32 ulp.
Measured on an MI355X: see DESIGN.md section 3.10.
'''

import ctypes as C

import numpy as np
import pytest

from helpers import setup_engine, report
from display_ref import byte_rule, display_layout, synthetic_film, MARKER8, OPS, TRANSFERS

pytestmark = pytest.mark.gpu


def _scene(name):
    from ptina_amd import scenes
    return scenes.get_scene(name)


def _render(scene, nx, ny, frames, preview=0, slab=None):
    from ptina_amd.engine.preview import PreviewEngine
    eng = setup_engine(_scene(scene), nx, ny, slab=slab)
    if frames:
        eng.render(frames)
    if preview:
        PreviewEngine().render(preview)
    return eng


def _film():
    from ptina_amd.things import FilmTable
    return FilmTable()


def _door(raw, nx, ny, **kw):
    from ptina_amd.common import ctx
    return ctx().display_eval(raw, nx, ny, **kw)


def _to_film_layout(a, layout):
    '''[ny][nx][4] rows top-down -> [nx][ny][4]'''
    return np.ascontiguousarray(np.swapaxes(a[::-1], 0, 1)) if layout == 'display' else a


def _held(what, got, E, raw, nx, ny, layout='film', **kw):
    '''`got` (as the call returned it) and the exposure `E` against the restatement on `raw`'''
    assert got.dtype == np.uint8 and got.shape == ((ny, nx, 4) if layout == 'display' else (nx, ny, 4))
    r = byte_rule(_to_film_layout(got, layout), raw, nx, ny, **kw)
    share = r['excused'] / r['colour_bytes'] if r['colour_bytes'] else 0.0
    ulp = float(np.spacing(np.float32(r['E64'])))
    e_bound = max(8 * abs(r['E32'] - r['E64']), ulp)
    report(f'display {what} {layout} {kw}: d = max|u32 - u64| = {r["d"]:.3e} bytes, tau = {r["tau"]:.3e}; excused {r["excused"]} of '
           f'{r["colour_bytes"]} colour bytes = {100 * share:.4f} %, outside the rule {r["bad"]}, worst {r["worst"]}; exposure {float(E):.9g} '
           f'vs ref64 {r["E64"]:.9g}: off {abs(float(E) - r["E64"]):.3e}, bound {e_bound:.3e} (|E32 - E64| = {abs(r["E32"] - r["E64"]):.3e}, ulp {ulp:.3e})')
    assert r['bad'] == 0 and r['worst'] <= 1, f'{what} {layout} {kw}: {r["bad"]} bytes outside the byte rule (tau {r["tau"]:.3e}), worst {r["worst"]}'
    assert r['excused'] <= 0.01 * r['colour_bytes'], f'{what} {layout} {kw}: {r["excused"]} excused bytes exceed 1 % of {r["colour_bytes"]}'
    if kw.get('exposure'):
        assert np.float32(E) == np.float32(kw['exposure'])
    else:
        assert abs(float(E) - r['E64']) <= e_bound, f'{what} {kw}: exposure {float(E)!r} vs {r["E64"]!r}, bound {e_bound:.3e}'
    return r


def _cases():
    for op in OPS:
        for transfer in TRANSFERS:
            for dither in (True, False):
                for exposure in (None, 0.3):
                    yield dict(op=op, transfer=transfer, dither=dither, exposure=exposure)


# ---------------------------------------------------------------- 1, 2. parity on rendered films
@pytest.mark.parametrize('scene,nx,ny', [('s34', 37, 29), ('s978', 48, 40)])
def test_parity_rendered_films(fresh, scene, nx, ny):
    '''ragged against the 64 x 16 tile and the 4096-element metering run; every operator, transfer, dither, layout, exposure mode'''
    _render(scene, nx, ny, 4)
    film = _film()
    raw = film.get_raw(0).copy()
    assert np.all(raw[:, 3] == 4)
    for kw in _cases():
        for layout in ('film', 'display'):
            got = film.get_display(layout=layout, **kw)
            _held(f'{scene} {nx}x{ny}', got, film.last_exposure, raw, nx, ny, layout=layout, **kw)


def test_parity_many_tiles_ragged(fresh):
    nx, ny = 130, 70
    _render('s34', nx, ny, 1)
    film = _film()
    raw = film.get_raw(0).copy()
    got = film.get_display(layout='display')
    _held('s34 130x70', got, film.last_exposure, raw, nx, ny, layout='display')
    got = film.get_display(layout='display', op='ptina', exposure=0.3, transfer='gamma')        # the reference's functor
    _held('s34 130x70', got, film.last_exposure, raw, nx, ny, layout='display', op='ptina', exposure=0.3, transfer='gamma')


@pytest.mark.parametrize('id', [1, 2])
def test_parity_preview_passes(fresh, id):
    '''albedo and normal: the normal pass holds negative sums, which the sanitiser shows as black'''
    nx, ny = 48, 40
    _render('s978', nx, ny, 1, preview=2)
    film = _film()
    raw = film.get_raw(id).copy()
    assert np.all(raw[:, 3] == 2) and (id == 1 or (raw[:, :3] < 0).any())
    _held(f's978 pass {id}', film.get_display(id=id), film.last_exposure, raw, nx, ny)


# ---------------------------------------------------------------- 3. the transpose, exactly
@pytest.mark.parametrize('nx,ny', [(37, 29), (130, 70), (64, 64)])
def test_display_layout_is_the_film_layout_transposed_and_flipped(fresh, nx, ny):
    from ptina_amd.things import init_things
    init_things()
    raw = synthetic_film(nx * 1000 + ny, nx, ny)
    for kw in (dict(), dict(dither=False, exposure=0.3, op='reinhard')):
        a, Ea = _door(raw, nx, ny, layout='film', **kw)
        b, Eb = _door(raw, nx, ny, layout='display', **kw)
        assert a.shape == (nx, ny, 4) and b.shape == (ny, nx, 4) and Ea == Eb
        assert np.array_equal(b, display_layout(a))
        assert np.array_equal(b, np.swapaxes(a, 0, 1)[::-1])


# ---------------------------------------------------------------- 4. the door on synthetic accumulators
SYNTHETIC = [(15, 1, 1), (12, 1, 67), (13, 67, 1), (14, 33, 31)]          # the films tests/test_display_cpu.py measures the cap on
# the metering's second stage, at the default parameters only: one element into the second workgroup's run of 4096; a fold lane
# takes two partials (1 048 577 pixels, inside the default max_filmsize of 2^21)
SYNTHETIC_FOLD = [(7, 1, 4097), (8, 1, 256 * 4096 + 1)]


@pytest.mark.parametrize('seed,nx,ny', SYNTHETIC + SYNTHETIC_FOLD)
def test_door_on_synthetic_films(fresh, seed, nx, ny):
    from ptina_amd.things import init_things
    init_things()
    raw = synthetic_film(seed, nx, ny)
    assert (raw[:, 3] != 0).any()
    fold = (seed, nx, ny) in SYNTHETIC_FOLD
    for kw in [dict()] if fold else _cases():
        for layout in ('film',) if fold else ('film', 'display'):
            got, E = _door(raw, nx, ny, layout=layout, **kw)
            _held(f'synthetic {seed} {nx}x{ny}', got, E, raw, nx, ny, layout=layout, **kw)


def test_door_on_poisoned_and_degenerate_films(fresh):
    from ptina_amd.things import init_things
    init_things()
    nx, ny = 33, 31
    marker = np.uint8(MARKER8)
    # NaN, +-inf, negatives and 3e38 injected into valid pixels
    raw = synthetic_film(21, nx, ny, invalid=0.1)
    ok = np.flatnonzero(raw[:, 3] != 0)
    rng = np.random.default_rng(22)
    for k, bad in enumerate([np.nan, np.inf, -np.inf, -2.5, 3e38, -3e38]):
        rows = rng.choice(ok, 12, replace=False)
        raw[rows, rng.integers(0, 3, 12)] = np.float32(bad)
    raw[ok[0], :3] = np.float32([np.nan, np.inf, -1.0])
    raw[ok[1], :3] = np.float32(3e38)
    for kw in _cases():
        got, E = _door(raw, nx, ny, **kw)
        assert np.isfinite(E) and E > 0
        _held('poisoned 33x31', got, E, raw, nx, ny, **kw)
        px = got.reshape(-1, 4)
        assert px[ok[0]].tolist() == [0, 255, 0, 255] and px[ok[1]].tolist() == [255, 255, 255, 255]
    # a black film (valid, all sums zero): Lavg = 1e-4, every colour byte 0 whatever the dither adds
    raw = np.zeros((nx * ny, 4), np.float32)
    raw[:, 3] = 3
    for kw in (dict(), dict(op='linear', transfer='gamma', dither=False)):
        got, E = _door(raw, nx, ny, **kw)
        _held('black 33x31', got, E, raw, nx, ny, **kw)
        assert not got[..., :3].any() and np.all(got[..., 3] == 255)
    # no valid pixel: E == 1 and every pixel the marker, in both layouts, whatever the colour sums hold
    raw = synthetic_film(23, nx, ny, invalid=0.0)
    raw[:, 3] = 0
    for layout in ('film', 'display'):
        got, E = _door(raw, nx, ny, layout=layout)
        assert E == 1 and np.all(got == marker)
        _held('all invalid 33x31', got, E, raw, nx, ny, layout=layout)
    # alternate columns invalid
    raw = synthetic_film(24, nx, ny, invalid=0.0)
    raw.reshape(nx, ny, 4)[1::2, :, 3] = 0
    for layout in ('film', 'display'):
        got, E = _door(raw, nx, ny, layout=layout)
        _held('alternate columns 33x31', got, E, raw, nx, ny, layout=layout)
        f = _to_film_layout(got, layout)
        assert np.all(f[1::2] == marker) and np.all(f[0::2, :, 3] == 255)
    # the metering's shape depends on the pixel count alone: the valid columns alone, as a film of their own, meter the same
    cut = np.ascontiguousarray(raw.reshape(nx, ny, 4)[0::2]).reshape(-1, 4)
    assert _door(cut, (nx + 1) // 2, ny)[1] == E


# ---------------------------------------------------------------- 5. the denoised source
def test_denoised_source_is_the_door_on_get_denoised(fresh):
    '''the filter's image never visits the host, and converts to the very bytes the door gives for get_denoised()'s array: alpha 1
    is a weight of 1 (rgb / 1 is exact), the marker rows' alpha 0 a weight of 0'''
    nx, ny = 48, 40
    _render('s978', nx, ny, 4, preview=2, slab=(0, 41))
    film = _film()
    for dn in (dict(), dict(iterations=2, demodulate=False), dict(iterations=0)):
        img = film.get_denoised(**dn).copy()
        assert np.all(img[41:, :, 3] == 0) and np.all(img[:41, :, 3] == 1)
        for kw in (dict(), dict(layout='display', op='reinhard', transfer='gamma', dither=False), dict(exposure=0.3, op='ptina')):
            got = film.get_display(denoised=True, **kw, **dn)
            want, E = _door(img.reshape(-1, 4), nx, ny, **kw)
            assert np.array_equal(got, want), (dn, kw)
            assert np.float32(film.last_exposure) == E
    # and iterations = 0 is pass 0 itself
    assert np.array_equal(film.get_display(denoised=True, iterations=0), film.get_display())
    with pytest.raises(RuntimeError, match='iterations must be in 0..8'):
        film.get_display(denoised=True, iterations=9)
    with pytest.raises(TypeError):
        film.get_display(iterations=2)


# ---------------------------------------------------------------- 6. a slab
def test_slab_columns_outside_are_the_marker_and_do_not_meter(fresh):
    nx, ny = 64, 24
    _render('s34', nx, ny, 4, slab=(16, 40))
    film = _film()
    raw = film.get_raw(0).copy()
    w = raw.reshape(nx, ny, 4)[..., 3]
    assert np.all(w[16:40] == 4) and not w[:16].any() and not w[40:].any()
    marker = np.uint8(MARKER8)
    for layout in ('film', 'display'):
        got = film.get_display(layout=layout)
        _held('s34 64x24 slab 16..40', got, film.last_exposure, raw, nx, ny, layout=layout)
        f = _to_film_layout(got, layout)
        assert np.all(f[:16] == marker) and np.all(f[40:] == marker) and np.all(f[16:40, :, 3] == 255)
    cut = np.ascontiguousarray(raw.reshape(nx, ny, 4)[16:40]).reshape(-1, 4)
    assert _door(cut, 24, ny)[1] == np.float32(film.last_exposure)


# ---------------------------------------------------------------- 7. hygiene
def test_calls_repeat_and_write_no_film_pass(fresh):
    from ptina_amd.common import ctx
    import ptina_amd.worker as worker
    nx, ny = 48, 40
    _render('s978', nx, ny, 4, preview=2)
    film = _film()
    before = [film.get_raw(p).copy() for p in range(3)]
    a = film.get_display()
    Ea = film.last_exposure
    b = film.get_display()
    assert a is not b and np.array_equal(a, b) and film.last_exposure == Ea
    c = film.get_display(denoised=True, layout='display')
    assert np.array_equal(c, film.get_display(denoised=True, layout='display'))
    for p in range(3):
        assert np.array_equal(before[p].view(np.uint32), film.get_raw(p).view(np.uint32)), f'pass {p} changed'
    assert ctx().get_option('zero_copy') == 1
    ctx().set_option('zero_copy', 0)
    assert np.array_equal(film.get_display(), a) and film.last_exposure == Ea
    assert np.array_equal(film.get_display(denoised=True, layout='display'), c)
    ctx().set_option('zero_copy', 1)
    # a buffer that is not page-locked memory of the library's takes the device image and a copy
    from ptina_amd._lib import display_params
    out = np.zeros((nx, ny, 4), np.uint8)
    used = C.c_float(0)
    ctx().call('mpt_get_display', C.byref(display_params()), None, out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(used))
    assert np.array_equal(out, a) and np.float32(used.value) == np.float32(Ea)
    ctx().call('mpt_get_display', None, None, out.ctypes.data_as(C.POINTER(C.c_uint8)), None)        # NULL = the defaults
    assert np.array_equal(out, a)
    assert np.array_equal(worker.get_display(op='ptina', exposure=0.3), film.get_display(op='ptina', exposure=0.3))
    film.display_kernel_time()
    film.get_display()
    ms, n = film.display_kernel_time()
    assert n == 1 and ms > 0
    assert film.display_kernel_time() == (0.0, 0)


def test_get_display_leaves_the_image_hint_intact(fresh):
    '''render(); get_display(); get_image() returns the image of a context that never called get_display, bit for bit:
    PathEngine.render() hints the array of the next get_image(0), and get_display runs between the hint and the call that spends it'''
    from ptina_amd import common
    nx, ny = 48, 40
    eng = _render('s978', nx, ny, 0)
    eng.render(3)
    want3 = _film().get_image().copy()
    eng.render(2)
    want5 = _film().get_image().copy()
    common.reset_all()
    eng = _render('s978', nx, ny, 0)
    eng.render(3)
    _film().get_display()
    _film().get_display(denoised=True, layout='display')
    assert np.array_equal(_film().get_image().view(np.uint32), want3.view(np.uint32))
    eng.render(2)
    _film().get_display(layout='display')
    assert np.array_equal(_film().get_image().view(np.uint32), want5.view(np.uint32))


# ---------------------------------------------------------------- 8. errors
def test_every_stated_error_raises_and_leaves_the_film(fresh):
    from ptina_amd.common import ctx
    from ptina_amd._lib import display_params
    nx, ny = 16, 16
    _render('s34', nx, ny, 2)
    film = _film()
    before = film.get_raw(0).copy()
    bad = [(dict(op=4), 'unknown op'), (dict(op=-1), 'unknown op'), (dict(transfer=2), 'unknown transfer'), (dict(layout=2), 'unknown layout'),
           (dict(id=3), 'out of range'), (dict(id=-2), 'out of range'), (dict(id=-1), 'out of range'),
           (dict(exposure=-0.5), 'exposure'), (dict(exposure=float('nan')), 'exposure'), (dict(exposure=float('inf')), 'exposure')]
    for name in ('key', 'white', 'gamma'):
        for v in (0.0, -1.0, float('nan'), float('inf')):
            bad.append(({name: v}, name + ' must be finite and positive'))
    for kw, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            film.get_display(**kw)
    with pytest.raises(RuntimeError, match='null output'):
        ctx().call('mpt_get_display', C.byref(display_params()), None, None, None)
    with pytest.raises(RuntimeError, match='null'):
        ctx().call('mpt_display_eval', C.byref(display_params()), None, 4, 4, None, None)
    with pytest.raises(RuntimeError, match='max_filmsize'):
        ctx().call('mpt_display_eval', None, before.ctypes.data_as(C.POINTER(C.c_float)), 0, 4,
                   np.zeros(64, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)), None)
    with pytest.raises(RuntimeError, match='unknown op'):
        _door(before, nx, ny, op=9)
    assert np.array_equal(before.view(np.uint32), film.get_raw(0).view(np.uint32))
    film.get_display()                                           # (the context is still good)
    assert C.sizeof(type(display_params())) == 36

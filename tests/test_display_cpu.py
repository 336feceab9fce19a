'''
CPU tests of the 8-bit display read-back (FilmTable.get_display, mpt_get_display): tests/display_ref.py, the numpy restatement the
GPU is held to (tests/test_display_gpu.py), is checked here against closed forms that share no code with it -- each operator and
transfer at hand-computed points, the Bayer matrix, the sanitiser, the metering, the layouts -- and the cap of the byte rule is
measured for the restatement's own two precisions.  Then the boundary: write_png, the struct's layout as the C compiler sees it,
and the three symbols the library must export.
'''

import ctypes as C
import math
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from display_ref import (display_ref, display_layout, bayer, sanitise, tone, transfer_curve, exposure_of, luminance, byte_rule,
                         synthetic_film, MARKER8, OPS, TRANSFERS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]


def _tol(T):
    return 4e-6 if T is np.float32 else 1e-13


# ---------------------------------------------------------------- operators and transfers
@pytest.mark.parametrize('T', DTYPES)
def test_operators_at_hand_computed_points(T):
    assert np.array_equal(tone([0.0, 0.25, 1.0, 7.0], 'linear', T=T), T([0, 0.25, 1, 1]))
    # PTINA: v / (v + 0.155) * 1.019; at v = 0.155 exactly half of 1.019
    assert abs(float(tone(T(0.155), 'ptina', T=T)) - 0.5095) < _tol(T)
    assert abs(float(tone(T(1.0), 'ptina', T=T)) - 1.019 / 1.155) < _tol(T)
    assert float(tone(T(100.0), 'ptina', T=T)) == 1.0                       # 1.0174...: clamped
    # REINHARD: v (1 + v / white^2) / (1 + v); reaches 1 exactly at v = white
    assert abs(float(tone(T(1.0), 'reinhard', white=4.0, T=T)) - (1 + 1 / 16) / 2) < _tol(T)
    assert abs(float(tone(T(4.0), 'reinhard', white=4.0, T=T)) - 1.0) < _tol(T)
    assert abs(float(tone(T(2.0), 'reinhard', white=2.0, T=T)) - 1.0) < _tol(T)
    assert abs(float(tone(T(1.0), 'reinhard', white=1e9, T=T)) - 0.5) < _tol(T)      # white -> infinity: v / (1 + v)
    # ACES (Narkowicz): v (2.51 v + 0.03) / (v (2.43 v + 0.59) + 0.14)
    assert abs(float(tone(T(1.0), 'aces', T=T)) - 2.54 / 3.16) < _tol(T)
    assert abs(float(tone(T(0.5), 'aces', T=T)) - 0.5 * 1.285 / (0.5 * 1.805 + 0.14)) < _tol(T)
    assert float(tone(T(50.0), 'aces', T=T)) == 1.0
    for op in OPS:
        assert float(tone(T(0.0), op, T=T)) == 0.0
        assert float(tone(T(1e18), op, T=T)) == 1.0 and float(tone(T(3e38), 'linear', T=T)) == 1.0


@pytest.mark.parametrize('T', DTYPES)
def test_transfers_at_hand_computed_points(T):
    assert float(transfer_curve(T(0.0), 'srgb', T=T)) == 0.0
    assert abs(float(transfer_curve(T(0.002), 'srgb', T=T)) - 0.02584) < _tol(T)
    assert abs(float(transfer_curve(T(1.0), 'srgb', T=T)) - 1.0) < _tol(T)
    assert abs(float(transfer_curve(T(0.5), 'srgb', T=T)) - (1.055 * 0.5 ** (1 / 2.4) - 0.055)) < _tol(T)
    assert abs(float(transfer_curve(T(0.5), 'srgb', T=T)) - 0.7353569830524495) < _tol(T)
    # the two branches meet at the threshold to 1e-7
    lo, hi = 12.92 * 0.0031308, 1.055 * 0.0031308 ** (1 / 2.4) - 0.055
    assert abs(lo - hi) < 1e-7
    assert abs(float(transfer_curve(T(0.25), 'gamma', gamma=2.0, T=T)) - 0.5) < _tol(T)
    assert abs(float(transfer_curve(T(0.5), 'gamma', gamma=2.2, T=T)) - 0.5 ** (1 / float(np.float32(2.2)))) < _tol(T)      # (the parameters are the f32 values the C ABI receives)
    assert float(transfer_curve(T(0.0), 'gamma', T=T)) == 0.0 and float(transfer_curve(T(1.0), 'gamma', T=T)) == 1.0


@pytest.mark.parametrize('T', DTYPES)
def test_operators_and_transfers_are_monotone(T):
    v = np.concatenate([[0.0], np.exp(np.linspace(np.log(1e-8), np.log(1e18), 4001))]).astype(T)
    for op in OPS:
        for white in (0.5, 4.0, 100.0):
            t = tone(v, op, white=white, T=T)
            assert t.dtype == T and np.all(np.diff(t) >= -(4e-7 if T is np.float32 else 1e-15)), (op, white)
            assert t[0] == 0 and t[-1] == 1 and t.min() >= 0 and t.max() <= 1
    t = np.linspace(0, 1, 5001).astype(T)
    for tr in TRANSFERS:
        s = transfer_curve(t, tr, T=T)
        assert s.dtype == T and np.all(np.diff(s) >= 0), tr


def test_ptina_preset_is_the_reference_functor():
    '''ptina/wip/tonemapping.py:15-18: x = x * 0.3 (exposure); x = x / (x + 0.155) * 1.019; x ** (1 / 2.2), written out here'''
    rng = np.random.default_rng(5)
    c = rng.uniform(0, 6, (7 * 5, 3))
    raw = np.concatenate([c * 2, np.full((35, 1), 2.0)], axis=1).astype(np.float32)
    u, by, valid, E = display_ref(raw, 7, 5, op='ptina', exposure=0.3, transfer='gamma', gamma=2.2, dither=False)
    x = raw[:, :3].astype(np.float64) / 2 * np.float64(np.float32(0.3))
    x = x / (x + 0.155) * 1.019
    x = np.clip(x, 0, 1) ** (1 / np.float64(np.float32(2.2)))
    assert E == np.float32(0.3) and valid.all()
    assert np.allclose(u.reshape(-1, 3), 255 * x + 0.5, rtol=0, atol=1e-10)
    assert np.array_equal(by[..., :3].reshape(-1, 3), np.floor(255 * x + 0.5).astype(np.uint8))


# ---------------------------------------------------------------- dither, sanitiser, metering, layouts
def test_bayer_matrix():
    xs, ys = np.meshgrid(np.arange(8), np.arange(8), indexing='ij')
    M = bayer(xs, ys)
    assert sorted(M.ravel().tolist()) == list(range(64))
    # the 2x2 corner [[0, 2], [3, 1]] (rows y, columns x) lives in the top two bits
    assert (M[:2, :2].T >> 4).tolist() == [[0, 2], [3, 1]]
    # the recursive construction, written on its own: M_2n = [[4 M_n, 4 M_n + 2], [4 M_n + 3, 4 M_n + 1]]
    m = np.zeros((1, 1), np.int64)
    for _ in range(3):
        m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
    assert np.array_equal(M.T, m)
    assert np.array_equal(bayer(xs + 8, ys + 16), M) and np.array_equal(bayer(xs + 1, ys)[:-1], M[1:])
    # every threshold (M + 0.5) / 64 lies strictly inside (0, 1) and their mean is 0.5: the dither adds no bias
    B = (M + 0.5) / 64
    assert B.min() > 0 and B.max() < 1 and B.mean() == 0.5


@pytest.mark.parametrize('T', DTYPES)
def test_sanitiser(T):
    got = sanitise(np.float32([np.nan, -1.0, -np.inf, -0.0, 0.0, 2.5, 3e38, np.inf]), T)
    assert got.dtype == T
    assert np.array_equal(got, T([0, 0, 0, 0, 0, 2.5, np.float32(3e38) if T is np.float32 else min(float(np.float32(3e38)), 3.0e38), 3.0e38]))
    assert np.isfinite(got).all()
    # through the whole chain: a NaN / negative / -inf channel is black, an inf / 3e38 one is white, for every operator
    raw = np.float32([[np.nan, -3.0, -np.inf, 1.0], [np.inf, 3e38, 1e30, 1.0], [0.5, 0.5, 0.5, 1.0]])
    for op in OPS:
        for exposure in (None, 0.3):
            u, by, valid, E = display_ref(raw, 3, 1, op=op, exposure=exposure, dither=False, dtype=T)
            assert np.isfinite(u).all() and np.isfinite(E)
            assert by[0, 0].tolist() == [0, 0, 0, 255] and by[1, 0].tolist() == [255, 255, 255, 255], (op, exposure)


@pytest.mark.parametrize('T', DTYPES)
def test_metering(T):
    # a grey film of luminance L: Lavg = 1e-4 + L, E = key / Lavg
    raw = np.tile(np.float32([1.0, 1.0, 1.0, 4.0]), (6, 1))           # c = 0.25 each, Y = 0.25
    u, by, valid, E = display_ref(raw, 3, 2, key=0.18, dtype=T)
    assert abs(float(E) - float(np.float32(0.18)) / 0.2501) < (3e-7 if T is np.float32 else 1e-12)
    # the geometric mean: luminances 0.01 and 1 (grey) meter as sqrt((1e-4 + 0.01) (1e-4 + 1))
    raw = np.float32([[0.01, 0.01, 0.01, 1], [1, 1, 1, 1], [0, 0, 0, 0], [5, 5, 5, 0]])
    c = sanitise(raw[:, :3] / np.where(raw[:, 3:4] == 0, 1, raw[:, 3:4]), T).reshape(2, 2, 3)
    valid = raw[:, 3].reshape(2, 2) != 0
    want = 0.5 / math.sqrt(0.0101 * 1.0001)
    assert abs(float(exposure_of(c, valid, 0.5, T)) - want) < 4e-7 * want
    assert abs(float(luminance(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]], T), T).sum()) - 2.0) < 1e-6
    # no valid pixel: E = 1, every pixel the marker
    u, by, valid, E = display_ref(np.zeros((12, 4), np.float32), 4, 3, dtype=T)
    assert E == 1 and type(E) is T and not valid.any() and np.all(by == np.uint8(MARKER8))
    # an all-black valid film: Lavg = 1e-4, E = key / 1e-4, and the image is black with alpha 255
    raw = np.tile(np.float32([0, 0, 0, 2]), (12, 1))
    u, by, valid, E = display_ref(raw, 4, 3, dither=False, dtype=T)
    assert abs(float(E) - 1800.0) < 2e-3 and np.all(by[..., :3] == 0) and np.all(by[..., 3] == 255)
    # a manual exposure is used as given
    assert display_ref(raw, 4, 3, exposure=0.3, dtype=T)[3] == T(np.float32(0.3))


def test_layouts():
    raw = synthetic_film(3, 5, 3)
    film = display_ref(raw, 5, 3)[1]
    disp = display_layout(film)
    assert disp.shape == (3, 5, 4) and disp.flags['C_CONTIGUOUS']
    assert np.array_equal(disp, np.swapaxes(film, 0, 1)[::-1])
    flat = disp.reshape(-1)
    for x in range(5):
        for y in range(3):
            at = ((3 - 1 - y) * 5 + x) * 4
            assert np.array_equal(flat[at:at + 4], film[x, y])


# ---------------------------------------------------------------- the byte rule's cap, for the restatement's own two precisions
SYNTHETIC = [(15, 1, 1), (12, 1, 67), (13, 67, 1), (14, 33, 31)]          # (seed, nx, ny): the films tests/test_display_gpu.py gives the door
# ... and the two it gives the door at the default parameters only, for the metering's second stage: one element into the second
# workgroup's run of 4096, and one partial more than the fold has lanes
SYNTHETIC_FOLD = [(7, 1, 4097), (8, 1, 256 * 4096 + 1)]


def synthetic_cases():
    for op in OPS:
        for transfer in TRANSFERS:
            for dither in (True, False):
                for exposure in (None, 0.3):
                    yield dict(op=op, transfer=transfer, dither=dither, exposure=exposure)


def test_f32_restatement_stays_inside_the_cap_on_the_synthetic_films():
    '''ref32 against ref64 alone: what differs from floor(u64) must be excused by the rule (tau = 8 d) and be at most 1 % of the
    colour bytes of the film, for every operator, transfer, dither and exposure mode'''
    worst = (0.0, None)
    for seed, nx, ny in SYNTHETIC + SYNTHETIC_FOLD:
        raw = synthetic_film(seed, nx, ny)
        assert (raw[:, 3] != 0).any()
        for kw in [dict()] if (seed, nx, ny) in SYNTHETIC_FOLD else synthetic_cases():
            b32 = display_ref(raw, nx, ny, dtype=np.float32, **kw)[1]
            r = byte_rule(b32, raw, nx, ny, **kw)
            assert r['bad'] == 0 and r['worst'] <= 1, (seed, nx, ny, kw, r)
            assert r['excused'] <= 0.01 * r['colour_bytes'], (seed, nx, ny, kw, r)
            if r['colour_bytes'] and r['excused'] / r['colour_bytes'] >= worst[0]:
                worst = (r['excused'] / r['colour_bytes'], (seed, nx, ny, kw, r['tau']))
    print('largest excused share of ref32 against ref64: %.4f %% at %s' % (100 * worst[0], worst[1]))


# ---------------------------------------------------------------- write_png
def _decode_png(path):
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    w, h, depth, ctype, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (2, 6)
    ch = 4 if ctype == 6 else 3
    lines = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * ch)
    assert not lines[:, 0].any()
    return lines[:, 1:].reshape(h, w, ch)


@pytest.mark.parametrize('shape', [(3, 5, 4), (1, 1, 4), (40, 48, 4), (7, 2, 3)])
def test_write_png_round_trip(tmp_path, shape):
    from ptina_amd.image import write_png
    a = np.random.default_rng(1).integers(0, 256, shape, dtype=np.uint8)
    path = str(tmp_path / 'a.png')
    write_png(path, a)
    assert np.array_equal(_decode_png(path), a)
    write_png(path, a[:, ::-1])                                  # a view that is not contiguous
    assert np.array_equal(_decode_png(path), a[:, ::-1])
    with pytest.raises(ValueError):
        write_png(path, a.astype(np.float32))
    with pytest.raises(ValueError):
        write_png(path, a[..., 0])


# ---------------------------------------------------------------- the boundary
def test_display_params_layout_matches_the_c_compiler():
    from ptina_amd._lib import DisplayParams
    gcc = shutil.which('gcc') or shutil.which('cc')
    assert gcc, 'no C compiler'
    fields = [name for name, _ in DisplayParams._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "miptina.h"\n'
           'int main(void) { printf("%zu", sizeof(mpt_display_params)); ' +
           ' '.join('printf(" %%zu", offsetof(mpt_display_params, %s));' % f for f in fields) +
           ' printf(" %d %d %d %d %d %d %d %d %d", MPT_DISPLAY_DENOISED, MPT_TONE_LINEAR, MPT_TONE_PTINA, MPT_TONE_REINHARD, MPT_TONE_ACES,'
           ' MPT_TRANSFER_SRGB, MPT_TRANSFER_GAMMA, MPT_LAYOUT_FILM, MPT_LAYOUT_DISPLAY); return 0; }\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'p.c'), 'w').write(src)
        subprocess.run([gcc, '-I', os.path.join(ROOT, 'include'), os.path.join(d, 'p.c'), '-o', os.path.join(d, 'p')], check=True)
        out = subprocess.run([os.path.join(d, 'p')], capture_output=True, text=True, check=True).stdout.split()
    nums = [int(x) for x in out]
    assert nums[0] == C.sizeof(DisplayParams) == 36
    assert nums[1:1 + len(fields)] == [getattr(DisplayParams, f).offset for f in fields]
    from ptina_amd import _lib
    assert nums[1 + len(fields):] == [_lib.DISPLAY_DENOISED, _lib.TONE_OPS['linear'], _lib.TONE_OPS['ptina'], _lib.TONE_OPS['reinhard'],
                                      _lib.TONE_OPS['aces'], _lib.TRANSFERS['srgb'], _lib.TRANSFERS['gamma'], _lib.LAYOUTS['film'],
                                      _lib.LAYOUTS['display']]
    assert sorted(_lib.TONE_OPS) == sorted(OPS) and sorted(_lib.TRANSFERS) == sorted(TRANSFERS)


def test_library_exports_the_display_symbols():
    from ptina_amd import _lib
    lib = _lib.load_library()
    for name in ('mpt_get_display', 'mpt_display_kernel_time', 'mpt_display_eval'):
        assert hasattr(lib, name), f'libmiptina.so lacks {name}'
        assert name in _lib.SIGNATURES


def test_display_params_builder():
    from ptina_amd import _lib
    p = _lib.display_params()
    assert (p.source, p.op, p.transfer, p.layout, p.dither) == (0, 3, 0, 0, 1)
    assert p.exposure == 0 and abs(p.key - 0.18) < 1e-7 and p.white == 4 and abs(p.gamma - 2.2) < 1e-6
    p = _lib.display_params(source=2, op='PTina', transfer='gamma', layout='display', dither=False, exposure=0.3)
    assert (p.source, p.op, p.transfer, p.layout, p.dither) == (2, 1, 1, 1, 0) and abs(p.exposure - 0.3) < 1e-7
    with pytest.raises(ValueError, match='unknown op'):
        _lib.display_params(op='filmic')

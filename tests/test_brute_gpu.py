'''
GPU tests (-m gpu) of the brute-force engine (BruteEngine; csrc/brute_kernel.hip).

Against the reference's executed source (tests/golden/reference_brute.npz, made by
tests/golden/make_reference_brute_golden.py: the reference's own BruteEngine run on numpy in f32 and f64), both builds,
the three cases of the path fixture, with the tolerances tests/test_reference_path_gpu.py uses for the same comparison
(the arithmetic of a brute bounce is a subset of path_trace's).

Properties, none with a number that is not derived: runs repeat bit for bit and split freely into launches and slabs;
frames of the three engines that write film pass 0 add in call order on one Sobol sampler; a scene without any light is
exactly black; and, the reason to have the engine, in a scene lit by the world light only (where path_trace traces no
shadow ray and weights nothing) the PathEngine's and the BruteEngine's tile means agree within 5 standard errors, the
standard error measured from independent blocks of both engines.
'''

import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import setup_engine, assert_parity, FAST, _report, tile_means

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'reference_brute.npz')
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import make_reference_path_golden as G   # noqa: E402  (scene definitions only; nothing of the reference is imported)


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _brute():
    from ptina_amd.engine.brute import BruteEngine
    return BruteEngine()


def _raw(pas=0):
    from ptina_amd.things import FilmTable
    return FilmTable().get_raw(pas).copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _time():
    from ptina_amd.sampling.sobol import SobolSampler
    return SobolSampler().state()[0]


# ---------------------------------------------------------------- 1. the reference's executed source
@pytest.mark.parametrize('mode', ['strict', 'fast'])
@pytest.mark.parametrize('name', sorted(G.CASES))
def test_hip_brute_renders_what_the_reference_source_renders(gold, fresh, mode, name):
    from ptina_amd.things import FilmTable
    key, nx, ny, spp = G.CASES[name]
    assert [int(x) for x in gold[f'f32/{name}/size']] == [nx, ny, spp]
    scene, lights, world = G.scene_of(key)
    setup_engine(scene, nx, ny, mode=mode, lights=lights, world=world)
    eng = _brute()
    assert _time() == 64
    film = FilmTable()
    eng.render()                                   # the fixture's call sequence: render(); clear(); spp x render()
    film.get_image()
    film.clear()
    for _ in range(spp):
        eng.render()
    raw = film.get_raw().astype(np.float64)
    assert np.all(raw[:, 3] == spp)
    for prec in ('f32', 'f64'):
        want = gold[f'{prec}/{name}/film']
        assert np.array_equal(raw[:, 3], want[:, 3])
        err = np.abs(raw[:, :3] - want[:, :3]) / (np.abs(want[:, :3]) + 1e-3 * spp)
        worst = float(err.max())
        msg = (f'brute {mode} {name} vs reference-source {prec} film: worst relative difference of a pixel sum {worst:.2e} '
               f'(pixel {int(err.max(axis=1).argmax())}), mean radiance {want[:, :3].mean() / spp:.4f}')
        print(msg)
        _report(msg)
        if mode == 'strict':
            f32, f64 = gold[f'f32/{name}/film'], gold[f'f64/{name}/film']
            spread = float((np.abs(f32[:, :3] - f64[:, :3]) / (np.abs(f64[:, :3]) + 1e-3 * spp)).max())
            assert worst <= (1e-4 if prec == 'f32' else max(1e-4, 1.5 * spread)), msg + f' (reference f32-vs-f64 spread {spread:.2e})'
    if mode == 'fast':
        want = gold[f'f64/{name}/film']
        img = (raw[:, :3] / raw[:, 3:4]).reshape(nx, ny, 3)
        ref = (want[:, :3] / want[:, 3:4]).reshape(nx, ny, 3)
        assert_parity(img, ref, *FAST, what=f'brute fast {name} vs reference-source f64 film')
        assert abs(img.mean() - ref.mean()) <= 0.01 * ref.mean()
    assert _time() == int(gold[f'f32/{name}/sobol_time']) == int(gold[f'f64/{name}/sobol_time']) == 64 + 1 + spp


# ---------------------------------------------------------------- 2. determinism, batching, slabs
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_determinism_and_batching(fresh, mode):
    from ptina_amd import common, scenes

    def run(split):
        common.reset_all()
        setup_engine(scenes.scene_s978(), 70, 50, mode=mode)       # ragged: not multiples of the 16x16 tile
        eng = _brute()
        if split:
            for _ in range(8):
                eng.render(1)
                _raw()                                             # a read-back between: eight launches
        else:
            eng.render(8)
        return _raw(), _time()

    a, ta = run(False)
    b, tb = run(True)
    c, tc = run(False)
    assert np.all(a[:, 3] == 8) and np.isfinite(a).all() and a[:, :3].sum() > 0
    assert np.array_equal(_bits(a), _bits(b)), f'{int((_bits(a) != _bits(b)).any(axis=1).sum())} pixels differ between render(8) and 8 x render(1)'
    assert np.array_equal(_bits(a), _bits(c))
    assert ta == tb == tc == 64 + 8


def test_more_frames_than_one_batch(fresh):
    '''a request above the kernels' batch limit (64 frames) is split and is the same film as its pieces'''
    from ptina_amd import common, scenes
    films = []
    for pieces in ((70,), (64, 6), (30, 40)):
        common.reset_all()
        setup_engine(scenes.scene_s34(), 32, 32, mode='fast')
        eng = _brute()
        for k in pieces:
            eng.render(k)
        films.append(_raw())
        assert _time() == 64 + 70
    assert np.all(films[0][:, 3] == 70)
    assert np.array_equal(_bits(films[0]), _bits(films[1])) and np.array_equal(_bits(films[0]), _bits(films[2]))


@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_slabs_reassemble_bit_identically(fresh, mode):
    from ptina_amd import common, scenes
    nx, ny, spp = 50, 37, 4
    setup_engine(scenes.scene_s34(), nx, ny, mode=mode)
    _brute().render(spp)
    full = _raw().reshape(nx, ny, 4)
    parts = np.zeros_like(full)
    for x0, x1 in ((0, 23), (23, 50)):
        common.reset_all()
        setup_engine(scenes.scene_s34(), nx, ny, mode=mode, slab=(x0, x1))
        _brute().render(spp)
        got = _raw().reshape(nx, ny, 4)
        assert np.all(got[:x0] == 0) and np.all(got[x1:] == 0)
        parts[x0:x1] = got[x0:x1]
    assert np.array_equal(_bits(parts), _bits(full))
    assert np.all(full[..., 3] == spp)


def test_stripes_reassemble_bit_identically(fresh):
    from ptina_amd import common, scenes
    from ptina_amd.common import ctx
    nx, ny, spp = 100, 37, 3
    setup_engine(scenes.scene_s34(), nx, ny, mode='fast')
    _brute().render(spp)
    full = _raw().reshape(nx, ny, 4)
    total = np.zeros_like(full)
    for rank in range(3):
        common.reset_all()
        setup_engine(scenes.scene_s34(), nx, ny, mode='fast')
        ctx().call('mpt_set_stripes', 16, rank, 3)
        _brute().render(spp)
        got = _raw().reshape(nx, ny, 4)
        assert np.all((got[..., 3] == 0) | (got[..., 3] == spp))
        assert not np.any((total[..., 3] > 0) & (got[..., 3] > 0))      # no column rendered twice
        total += got
    assert np.array_equal(_bits(total), _bits(full))


# ---------------------------------------------------------------- 3. call order, shared sampler, the other passes
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_call_order_with_path_engine_and_shared_sampler(fresh, mode):
    from ptina_amd import common, scenes
    from ptina_amd.things import FilmTable

    def run(readback):
        common.reset_all()
        path = setup_engine(scenes.scene_s34(), 48, 40, mode=mode)
        brute = _brute()
        steps, times = [], []
        for eng in (path, brute, path):
            eng.render()
            if readback:
                FilmTable().get_image()
                steps.append(_raw())
                times.append(_time())
        return _raw(), steps, times, _time()

    fused, _, _, t_fused = run(False)
    stepped, steps, times, t_stepped = run(True)
    assert np.array_equal(_bits(fused), _bits(stepped))
    assert t_fused == t_stepped == 64 + 3
    assert times == [65, 66, 67]                               # one Sobol point per frame, whichever engine rendered it
    assert [float(s[0, 3]) for s in steps] == [1.0, 2.0, 3.0] and np.all(fused[:, 3] == 3)
    # the brute frame is the middle one: it used Sobol point 66, not 65 or 67
    common.reset_all()
    setup_engine(scenes.scene_s34(), 48, 40, mode=mode)
    brute = _brute()
    from ptina_amd.sampling.sobol import SobolSampler
    SobolSampler().update()
    brute.render()
    alone = _raw()
    assert _time() == 66
    mid = steps[1].astype(np.float64)[:, :3] - steps[0].astype(np.float64)[:, :3]
    # (a difference of two f32 sums against one f32 sample: one rounding of the larger sum)
    assert np.all(np.abs(mid - alone[:, :3]) <= 2.0 ** -23 * np.abs(steps[1][:, :3]).astype(np.float64) + 1e-30)


def test_early_image_is_not_stale_after_a_brute_frame(fresh):
    from ptina_amd import scenes
    from ptina_amd.things import FilmTable
    path = setup_engine(scenes.scene_s34(), 32, 32, mode='fast')
    brute = _brute()
    path.render()
    brute.render()
    img = FilmTable().get_image()
    raw = _raw()
    assert np.all(raw[:, 3] == 2)
    assert np.allclose(img.reshape(-1, 4)[:, :3], raw[:, :3] / raw[:, 3:4], rtol=1e-6, atol=0)


def test_preview_passes_untouched_and_metropolis_lands_between(fresh):
    from ptina_amd import common, scenes
    from ptina_amd.engine.preview import PreviewEngine
    from ptina_amd.engine.mltpath import MLTPathEngine
    nx = ny = 32

    def run(readback):
        common.reset_all()
        setup_engine(scenes.scene_s34(), nx, ny, mode='fast')
        brute = _brute()
        mlt = MLTPathEngine(nchains=2**12, seed=4)
        PreviewEngine().render(2)
        p1, p2 = _raw(1), _raw(2)
        steps = []
        for eng in (brute, mlt, brute):
            eng.render()
            if readback:
                steps.append(_raw())
        return _raw(), steps, p1, p2, _raw(1), _raw(2), _time()

    fused, _, p1, p2, q1, q2, t = run(False)
    stepped, steps, *_ = run(True)
    assert np.array_equal(_bits(fused), _bits(stepped))
    assert np.array_equal(_bits(p1), _bits(q1)) and np.array_equal(_bits(p2), _bits(q2)) and np.all(p1[:, 3] == 2)
    assert t == 64 + 2 + 2                                     # two preview frames, two brute frames; Metropolis draws none
    w = [0.0] + [s[:, 3].astype(np.float64).sum() for s in steps]
    assert np.diff(w).tolist() == [nx * ny, 2**12, nx * ny]


# ---------------------------------------------------------------- 4. no light at all
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_no_lights_and_black_world_is_exactly_black(fresh, mode):
    from ptina_amd import scenes
    setup_engine(scenes.scene_s978(), 64, 48, mode=mode, lights=[], world=([0.0, 0.0, 0.0, 0.0], -1))
    _brute().render(5)
    raw = _raw()
    assert np.all(raw[:, 3] == 5)
    assert not raw[:, :3].any()


# ---------------------------------------------------------------- 5. an independent estimator of the same integral
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_brute_and_path_engine_agree_under_a_world_light_only(fresh, mode):
    '''No pool lights: path_trace's LightPool().sample returns nothing, no shadow ray is traced and no weight applied, so both
    engines estimate the same integral (they differ in the Sobol dimensions a bounce reads and in the 1e-6 throughput cut-off).
    K blocks per engine on consecutive Sobol ranges; per 8x8-pixel tile and channel the difference of the two engines' means must
    lie within 5 standard errors, the standard error taken from the spread of the K blocks of both engines.'''
    from ptina_amd import scenes
    from ptina_amd.things import FilmTable
    nx = ny = 64
    K, spp = 16, 64
    path = setup_engine(scenes.scene_s34(), nx, ny, mode=mode, lights=[], world=([1.0, 1.0, 1.0, 1.0], -1))
    brute = _brute()
    means = {}
    for label, eng in (('path', path), ('brute', brute)):
        blocks = []
        for _ in range(K):
            FilmTable().clear()
            eng.render(spp)
            raw = _raw().astype(np.float64).reshape(nx, ny, 4)
            assert np.all(raw[..., 3] == spp) and np.isfinite(raw).all()
            blocks.append(tile_means(raw[..., :3] / spp, 8))
        means[label] = np.array(blocks)                         # [K][8][8][3]
    assert _time() == 64 + 2 * K * spp
    mp, mb = means['path'].mean(axis=0), means['brute'].mean(axis=0)
    se = np.sqrt(means['path'].var(axis=0, ddof=1) / K + means['brute'].var(axis=0, ddof=1) / K)
    z = np.abs(mp - mb) / np.where(se > 0, se, 1.0)
    z = np.where((se == 0) & (mp != mb), np.inf, z)
    msg = (f'brute vs path, world light only, {mode}: worst tile difference {float(z.max()):.2f} standard errors, '
           f'mean radiance path {mp.mean():.5f} brute {mb.mean():.5f}, median relative standard error {float(np.median(se / mp)):.2e}')
    print(msg)
    _report(msg)
    assert mp.mean() > 0.05                                     # the world light reaches the room: the test is not about black
    assert (z <= 5.0).all(), msg


# ---------------------------------------------------------------- 6. the reference-named demo script
def test_matball_exam_script(tmp_path):
    out = tmp_path / 'matball.npy'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'exams', 'matball_amd.py'), '--size', '96', '--frames', '8',
                        '--metallic', '0.7', '--roughness', '0.3', '--out', str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    img = np.load(out)
    assert img.shape == (96, 96, 4) and np.isfinite(img).all() and img[..., :3].mean() > 0

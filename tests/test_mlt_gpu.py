'''
GPU tests of the Metropolis engine (MLTPathEngine; csrc/mlt_kernel.hip): the path door equals the
PathEngine, one chain step equals the numpy restatement of mltpath.py (tests/test_mlt_cpu.py), LSP = 1
converges to the path engine, runs repeat bit for bit and split freely, the invariants of a long run, its
interplay with PathEngine frames in one film, and the reference-named demo script.
'''

import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import setup_engine, FAST, tile_means
from test_mlt_cpu import propose, accept_mask, splat_cells, reset_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _scene(name):
    from ptina_amd import scenes
    return scenes.get_scene(name)


def _mlt(nchains, seed=0, lsp=None, sigma=None):
    from ptina_amd.engine.mltpath import MLTPathEngine
    e = MLTPathEngine(nchains=nchains, seed=seed)
    if lsp is not None:
        e.LSP[None] = lsp
    if sigma is not None:
        e.Sigma[None] = sigma
    return e


def _raw():
    from ptina_amd.things import FilmTable
    return FilmTable().get_raw().copy()


# ---------------------------------------------------------------- 1. the path door is the PathEngine's path
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_path_door_equals_path_engine(fresh, mode):
    from ptina_amd.sampling import wanghash2
    from ptina_amd.sampling.sobol import SobolSampler
    from ptina_amd.engine.mltpath import mlt_trace
    nx = ny = 64
    eng = setup_engine(_scene('s978'), nx, ny, mode=mode)
    eng.render()
    film = _raw()
    _, _, P = SobolSampler().state()
    dim = P.shape[0]
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    h = wanghash2(i, j).astype(np.int64).reshape(-1, 1)                      # film element i * ny + j
    k = np.arange(32, dtype=np.int64)[None, :]
    idx = ((h + k + 2**31) % 2**32 - 2**31) % dim                         # int32 counter, Python floor-mod (sobol.py:123)
    X = P[idx].astype(np.float32)
    X[:, 0] = (i.reshape(-1).astype(np.float32) + X[:, 0]) / np.float32(nx)   # (i + dx) / nx in f32, as path_begin
    X[:, 1] = (j.reshape(-1).astype(np.float32) + X[:, 1]) / np.float32(ny)
    rgb = mlt_trace(X)
    assert np.all(film[:, 3] == 1.0)
    if mode == 'strict':
        assert np.array_equal(rgb.view(np.int32), film[:, :3].view(np.int32)), \
            f'{int((rgb != film[:, :3]).any(axis=1).sum())} pixels differ'
    else:
        from helpers import assert_parity
        assert_parity(rgb.reshape(nx, ny, 3), film[:, :3].reshape(nx, ny, 3), *FAST, what='mlt door fast')


# ---------------------------------------------------------------- 2. one chain step = the numpy restatement
@pytest.mark.parametrize('lsp,sigma', [(0.25, 0.01), (0.0, 0.05), (1.0, 0.01), (0.5, 0.2)])
def test_chain_step_matches_numpy(fresh, lsp, sigma):
    from ptina_amd.things import FilmTable
    from ptina_amd.engine.mltpath import mlt_trace
    n, seed, it0, nx, ny = 4096, 11, 5, 64, 48
    setup_engine(_scene('s978'), nx, ny, mode='strict')
    e = _mlt(n, seed, lsp, sigma)
    rng = np.random.default_rng(3)
    X = rng.random((n, 32), dtype=np.float32)
    X[X >= 1] = 0
    large, Xn = propose(seed, X, it0, lsp, sigma)
    Ln = mlt_trace(Xn)
    tol_chains = max(1, int(0.001 * n))

    # (a) L_old = 0: every finite proposal is accepted -- the state shows the proposals
    FilmTable().clear()
    e.set_state(X, np.zeros((n, 3), np.float32), it0)
    e.render(1)
    X1, L1, it1 = e.get_state()
    assert it1 == it0 + 1
    ok = np.isfinite(Ln).all(axis=1)
    bad = np.abs(X1 - Xn).max(axis=1) > 1e-6
    bad |= ok & ~np.all(np.isclose(L1, Ln, rtol=1e-5, atol=1e-6), axis=1)
    assert int(bad[ok].sum()) <= tol_chains, f'{int(bad[ok].sum())} proposals differ'
    # film increments: the proposals' radiance at their cells, w = 1 each
    film = _raw()
    want = np.zeros((nx * ny, 4), np.float64)
    cells = splat_cells(Xn, nx, ny)
    np.add.at(want, cells, np.concatenate([Ln.astype(np.float64), np.ones((n, 1))], axis=1))
    assert film[:, 3].sum() == n
    moved = np.zeros(nx * ny, bool)
    moved[cells[bad]] = True
    assert np.allclose(film[~moved, :3], want[~moved, :3], rtol=1e-4, atol=1e-5, equal_nan=True)

    # (b) L_old = trace(X): the accept decisions
    Lo = mlt_trace(X)
    FilmTable().clear()
    e.set_state(X, Lo, it0)
    e.render(1)
    X2, L2, _ = e.get_state()
    acc, coin, a = accept_mask(seed, n, it0, Ln, Lo)
    want_X = np.where(acc[:, None], Xn, X)
    differ = np.abs(X2 - want_X).max(axis=1) > 1e-6
    near = np.abs(coin - a) < 1e-5                                         # coins within 1e-5 of the threshold may go either way
    assert int((differ & ~near).sum()) <= tol_chains, f'{int((differ & ~near).sum())} accept decisions differ'
    assert int(differ.sum()) <= tol_chains + int(near.sum())
    if lsp == 0.0:
        assert not large.any()
    if lsp == 1.0:
        assert large.all()


# ---------------------------------------------------------------- 3. LSP = 1 converges to the path engine
def test_lsp1_converges_to_path_engine(fresh):
    from ptina_amd.things import FilmTable
    nx = ny = 32
    eng = setup_engine(_scene('s34'), nx, ny, mode='fast')
    refs = []
    for _ in range(4):                                                      # 4 consecutive batches of 256 spp of the Sobol path engine
        FilmTable().clear()
        eng.render(256)
        refs.append(tile_means(FilmTable().get_image(), 8))
    ref = np.mean(refs, axis=0)
    se_ref = np.std(refs, axis=0, ddof=1) / np.sqrt(len(refs))
    FilmTable().clear()
    e = _mlt(2**18, seed=5, lsp=1.0)
    batches = []
    for b in range(8):                                                      # 8 independent images of ~256 proposals per pixel
        FilmTable().clear()
        e.render(1)
        img = FilmTable().get_image()
        assert np.isfinite(img).all()
        batches.append(tile_means(img, 8))
    m = np.mean(batches, axis=0)
    se = np.std(batches, axis=0, ddof=1) / np.sqrt(len(batches))
    # bound: 6 standard errors of the difference, from the per-tile standard errors measured over the MLT's 8 independent
    # batches and the path engine's 4 batches
    bound = 6.0 * np.sqrt(se ** 2 + se_ref ** 2)
    worst = float((np.abs(m - ref) / bound).max())
    print(f'LSP=1 vs PathEngine: worst |diff| / bound = {worst:.3f}')
    assert np.all(np.abs(m - ref) <= bound), worst


# ---------------------------------------------------------------- 4. the chains sample in proportion to luminance
def _world_only_scene():
    '''two triangles behind the camera (never hit) and a smooth, textured world light: L is a noise-free function of
    the screen position'''
    from ptina_amd import scenes
    p, n, t = scenes.quad((-1, -1, 50), (1, -1, 50), (1, 1, 50), (-1, 1, 50), (0, 0, 1))
    verts = scenes._pack(p, n, t)
    S, T = np.meshgrid((np.arange(512) + 0.5) / 512, (np.arange(256) + 0.5) / 256, indexing='ij')
    env = np.ones((512, 256, 4), np.float32)
    wave = np.sin(2 * np.pi * 12 * S) * np.cos(2 * np.pi * 6 * T)          # ~2 periods across the view each way
    env[..., 0] = 1.0 + 0.6 * wave
    env[..., 1] = 0.9 + 0.5 * np.sin(2 * np.pi * 9 * S + 1.0)
    env[..., 2] = 1.1 + 0.4 * np.cos(2 * np.pi * 8 * T)
    return verts, np.zeros(2, np.int32), [scenes.material()], [env]


def _chi2_sf(x, k):
    '''chi-square survival function by the Wilson-Hilferty cube-root normal approximation (accurate to ~1e-3 at k = 63)'''
    import math
    z = ((x / k) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * k))) / math.sqrt(2.0 / (9.0 * k))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def test_stationary_distribution_follows_luminance(fresh):
    from ptina_amd.things import FilmTable
    nx = ny = 64
    eng = setup_engine(_world_only_scene(), nx, ny, mode='fast', lights=[], world=((1.0, 1.0, 1.0, 1.0), 0))
    eng.render(64)
    ref = FilmTable().get_image()[..., :3].astype(np.float64)
    assert np.isfinite(ref).all() and ref.min() > 0.1
    lum = ref.mean(axis=2)
    print(f'world-only scene: luminance {lum.min():.3f} .. {lum.max():.3f}, mean {lum.mean():.3f}')

    n = 2**18
    e = _mlt(n, seed=21)                                                   # LSP 0.25, Sigma 0.01 (the reference's defaults)
    e.render(100)                                                          # burn-in: a large step is accepted with probability
    X, L, _ = e.get_state()                                                # >= 0.25 * min(L) / max(L) per iteration
    # chain positions on 8 x 8 bins of (dim 0, dim 1) against the bin-integrated luminance (a bin = 8 x 8 pixels)
    obs = np.histogram2d(X[:, 0], X[:, 1], bins=8, range=[[0, 1], [0, 1]])[0]
    w = lum.reshape(8, nx // 8, 8, ny // 8).sum(axis=(1, 3))
    exp = n * w / w.sum()
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    pval = _chi2_sf(chi2, 63)
    print(f'chain positions vs luminance: chi2 {chi2:.1f} on 63 dof, p = {pval:.3g}')
    assert pval > 1e-3, (chi2, pval)
    # and the histogram is not the uniform one: the test can tell the two apart
    assert _chi2_sf(float(((obs - n / 64) ** 2 / (n / 64)).sum()), 63) < 1e-6

    # the film: a pixel shows the mean of the proposals that landed on it.  L is smooth, so that mean lies within the range
    # of L over the pixel, bounded by the largest difference between the pixel's and a neighbour's path-traced value
    FilmTable().clear()
    e.render(20)
    img = FilmTable().get_image()
    assert (img[..., 3] == 1.0).all()
    pad = np.pad(ref, ((1, 1), (1, 1), (0, 0)), mode='edge')
    rng = np.max([np.abs(pad[1 + di:1 + di + nx, 1 + dj:1 + dj + ny] - ref)
                  for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1))], axis=0)
    diff = np.abs(img[..., :3] - ref)
    bound = rng + 1e-3 * ref
    print(f'MLT film vs PathEngine: worst |diff| / bound = {float((diff / bound).max()):.3f}')
    assert (diff <= bound).all()


# ---------------------------------------------------------------- 5. determinism
def test_determinism_and_launch_split(fresh):
    from ptina_amd.things import FilmTable
    setup_engine(_scene('s978'), 64, 64, mode='fast')
    e = _mlt(2**14, seed=1)
    e.render(8)
    f_a, s_a = _raw(), e.get_state()
    FilmTable().clear(); e.reset()
    e.render(8)
    f_b, s_b = _raw(), e.get_state()
    FilmTable().clear(); e.reset()
    for _ in range(8):
        e.render(1)
        _raw()                                                              # a read-back between: eight launches
    f_c, s_c = _raw(), e.get_state()
    for f, s in ((f_b, s_b), (f_c, s_c)):
        assert np.array_equal(f.view(np.int32), f_a.view(np.int32))
        assert np.array_equal(s[0].view(np.int32), s_a[0].view(np.int32))
        assert np.array_equal(s[1].view(np.int32), s_a[1].view(np.int32)) and s[2] == s_a[2] == 8
    FilmTable().clear()
    e.seed = 2
    e.reset()
    e.render(8)
    assert not np.array_equal(_raw(), f_a)


def test_reset_state_matches_numpy(fresh):
    setup_engine(_scene('s34'), 16, 16, mode='fast')
    e = _mlt(1000, seed=9)
    X, L, it = e.get_state()
    assert it == 0 and not L.any()
    assert np.array_equal(X, reset_state(9, 1000))


# ---------------------------------------------------------------- 6. invariants of a long run
def test_invariants_long_run_and_odd_film(fresh):
    from ptina_amd.things import FilmTable
    from ptina_amd.sampling.sobol import SobolSampler
    setup_engine(_scene('s978'), 512, 512, mode='fast')
    t0 = SobolSampler().time
    e = _mlt(2**18, seed=3)
    e.render(200)
    film = _raw()
    X, L, it = e.get_state()
    assert it == 200
    assert film[:, 3].astype(np.float64).sum() == 2**18 * 200
    assert np.isfinite(film).all() and np.isfinite(X).all() and np.isfinite(L).all()
    assert (X >= 0).all() and (X < 1).all()
    assert SobolSampler().time == t0                                        # MLT does not touch the Sobol state
    FilmTable().set_size(1000, 600)
    FilmTable().clear()
    e.LSP[None] = 1.0
    e.reset()
    e.render(40)
    w = _raw()[:, 3].reshape(1000, 600)
    assert w.astype(np.float64).sum() == 2**18 * 40
    assert (w[0] > 0).all() and (w[-1] > 0).all() and (w[:, 0] > 0).all() and (w[:, -1] > 0).all()


# ---------------------------------------------------------------- 7. interplay with PathEngine frames
def test_interplay_with_path_engine(fresh):
    from ptina_amd import common
    from ptina_amd.things import FilmTable
    from ptina_amd.sampling.sobol import SobolSampler

    def run(readback):
        common.reset_all()
        eng = setup_engine(_scene('s34'), 32, 32, mode='fast')
        e = _mlt(2**12, seed=4)
        steps = []
        for kind, k in (('p', 2), ('m', 3), ('p', 1), ('m', 2), ('m', 1), ('p', 3)):
            (eng.render if kind == 'p' else e.render)(k)
            if readback:
                steps.append(_raw())
        return _raw(), steps, SobolSampler().time

    fused, _, t_fused = run(False)
    stepped, steps, t_stepped = run(True)
    assert np.array_equal(fused.view(np.int32), stepped.view(np.int32))   # call order, fused or not
    assert t_fused == t_stepped
    # each step added exactly its own samples: PathEngine 1024 per frame, MLT 4096 per iteration
    w = [0.0] + [s[:, 3].astype(np.float64).sum() for s in steps]
    assert np.diff(w).tolist() == [2048, 3 * 4096, 1024, 2 * 4096, 4096, 3 * 1024]

    # the PathEngine frames are those of a run without MLT, less the MLT contribution
    common.reset_all()
    eng = setup_engine(_scene('s34'), 32, 32, mode='fast')
    eng.render(6)
    path_only = _raw()
    common.reset_all()
    setup_engine(_scene('s34'), 32, 32, mode='fast')
    e = _mlt(2**12, seed=4)
    e.render(6)
    mlt_only = _raw()
    assert np.array_equal(fused[:, 3], path_only[:, 3] + mlt_only[:, 3])
    assert np.allclose(fused[:, :3], path_only[:, :3] + mlt_only[:, :3], rtol=1e-5, atol=1e-5)

    # get_image after PathEngine().render(); MLTPathEngine().render() shows both (no stale early image)
    common.reset_all()
    eng = setup_engine(_scene('s34'), 32, 32, mode='fast')
    e = _mlt(2**12, seed=4)
    eng.render(); e.render()
    img = FilmTable().get_image()
    raw = _raw()
    assert np.array_equal(img[..., 3].reshape(-1), np.where(raw[:, 3] > 0, 1.0, 0.0).astype(np.float32))
    nz = raw[:, 3] > 0
    assert raw[:, 3].sum() == 1024 + 4096
    assert np.allclose(img.reshape(-1, 4)[nz, :3], raw[nz, :3] / raw[nz, 3:4], rtol=1e-6, atol=0)


def test_mlt_render_refuses_a_split_film(fresh):
    from ptina_amd.common import ctx
    setup_engine(_scene('s34'), 32, 32, mode='fast')
    e = _mlt(2**10)
    ctx().call('mpt_set_stripes', 16, 0, 2)
    with pytest.raises(RuntimeError, match='one GPU'):
        e.render(1)


# ---------------------------------------------------------------- 8. the reference-named demo script
def test_metropolis_exam_script(tmp_path):
    out = tmp_path / 'mlt.npy'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'exams', 'metropolis_amd.py'), '--size', '128', '--frames', '4',
                        '--lsp', '0.3', '--sigma', '0.02', '--out', str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    img = np.load(out)
    assert img.shape == (128, 128, 4) and np.isfinite(img).all() and img[..., :3].mean() > 0

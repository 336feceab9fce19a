'''
CPU tests of adaptive sampling's numpy restatement (tests/adaptive_ref.py): the selection against
brute-force Python loops, the device's list order, engine.render_adaptive's loop on the CPU oracle's per-frame films -- the
oracle's numbers are deterministic here -- and on stubs, and the ABI.  The host-side validation of mpt_adapt_set_list needs a
context, and a context needs a device (mpt_create refuses without one): it is covered on the GPU,
tests/test_adaptive_gpu.py::test_every_stated_error.
'''

import numpy as np
import pytest

from adaptive_ref import run_loop, select, select_ordered, device_order, TILE
from noise_ref import noise_map, synthetic_pair, f32
from helpers import setup_oracle

SIZES = [(1, 1), (3, 5), (16, 16), (17, 33), (97, 61)]


def thresholds(F, M):
    '''0, the median e and the largest e of the valid pixels'''
    e, valid = noise_map(F, M)
    ev = np.sort(e[valid])
    return [0.0] if not ev.size else [0.0, float(ev[ev.size // 2]), float(ev[-1])]


# ---------------------------------------------------------------- the selection
@pytest.mark.parametrize('nx,ny', SIZES)
def test_select_against_brute_force_loops(nx, ny):
    seed = 0
    while True:                                                  # (a 1 x 1 film: draw until its pixel is valid)
        F, M = synthetic_pair(1000 * nx + ny + seed, nx, ny)
        if noise_map(F, M)[1].any():
            break
        seed += 1
    e, valid = noise_map(F, M)
    e, valid = e.reshape(nx, ny), valid.reshape(nx, ny)
    for t in thresholds(F, M):
        above = [[bool(valid[i, j]) and bool(e[i, j] > f32(t)) for j in range(ny)] for i in range(nx)]
        for dilate in (0, 1):
            want = []
            for i in range(nx):
                for j in range(ny):
                    near = above[i][j]
                    if dilate:
                        for a in range(max(i - 1, 0), min(i + 2, nx)):             # no wrap-around at the film's edges
                            for b in range(max(j - 1, 0), min(j + 2, ny)):
                                near = near or above[a][b]
                    if valid[i, j] and near:
                        want.append(i * ny + j)
            got = select(F, M, nx, ny, t, dilate)
            assert got.dtype == np.int32 and got.tolist() == want, (nx, ny, t, dilate)
            act = np.zeros(nx * ny, bool)
            act[got] = True
            assert act[np.flatnonzero(np.array(above).ravel())].all()                  # above pixels are active
            assert not act[~valid.ravel()].any()                                       # a pixel that is not valid never is
            if dilate == 0:
                assert np.array_equal(act.reshape(nx, ny), np.array(above))
        # the largest e is not above itself (>, not >=), zero is below every positive e
        assert select(F, M, nx, ny, thresholds(F, M)[-1], 0).size == 0


def test_an_invalid_pixel_beside_an_above_one_is_never_listed_and_corners_do_not_wrap():
    nx, ny = 5, 4
    F = np.zeros((nx * ny, 4), f32)
    M = np.zeros((nx * ny, 4), f32)
    F[:] = (2, 2, 2, 4)
    M[:] = (1, 1, 1, 2)                                  # every pixel valid with e = 0
    F[0] = (40, 40, 40, 4)                               # the corner (0, 0) is noisy
    M[1, 3] = 0                                          # its neighbour (0, 1) has no samples in the mark: not valid
    assert select(F, M, nx, ny, 0.5, 0).tolist() == [0]
    # dilated: (1, 0) and (1, 1) join; (0, 1) is not valid; nothing at the far edges (0, 3), (4, 0), (4, 3) wraps in
    assert select(F, M, nx, ny, 0.5, 1).tolist() == [0, 1 * ny + 0, 1 * ny + 1]
    F[nx * ny - 1] = (40, 40, 40, 4)                     # and the opposite corner (4, 3)
    assert select(F, M, nx, ny, 0.5, 1).tolist() == [0, 4, 5, 3 * ny + 2, 3 * ny + 3, 4 * ny + 2, 4 * ny + 3]


def test_device_order_is_tile_major_then_lane_order():
    nx, ny = 17, 33
    every = np.arange(nx * ny)
    got = device_order(every, ny)
    want = []
    for ti in range((nx + TILE - 1) // TILE):
        for tj in range((ny + TILE - 1) // TILE):
            for lane in range(TILE * TILE):
                i, j = ti * TILE + lane // TILE, tj * TILE + lane % TILE
                if i < nx and j < ny:
                    want.append(i * ny + j)
    assert got.tolist() == want and sorted(want) == every.tolist()
    F, M = synthetic_pair(5, nx, ny)
    L = select_ordered(F, M, nx, ny, 0.0, 1)
    assert np.array_equal(np.sort(L), select(F, M, nx, ny, 0.0, 1)) and np.array_equal(L, device_order(np.sort(L), ny))
    src = open(__import__('os').path.join(__import__('os').path.dirname(__file__), '..', 'ptina_amd', 'csrc', 'mpt_types.h')).read()
    assert '#define MPT_TILE %d' % TILE in src


# ---------------------------------------------------------------- the loop on the CPU oracle's films
_FRAMES = {}


def oracle_frames(oracle_mod, scene, nx, ny, n):
    '''R[f] = the raw film of frame f alone (clear, one frame, read back: the Sobol sampler runs on across clear), computed once'''
    key = (scene, nx, ny)
    if key not in _FRAMES or _FRAMES[key].shape[0] < n:
        from ptina_amd import scenes
        o = setup_oracle(oracle_mod, scenes.get_scene(scene), nx, ny)
        R = np.empty((n, nx * ny, 4), f32)
        for f in range(n):
            o.clear()
            o.render(1)
            R[f] = o.get_film_raw(0)
        assert np.all(R[:, :, 3] == 1)
        R.setflags(write=False)
        _FRAMES[key] = R
    return _FRAMES[key]


def check_invariants(r, R, nx, ny):
    w = r.film[:, 3]
    assert w.max() <= r.spp and w.min() >= r.history[0][0]                   # no w above the level; every pixel has the first two groups
    assert r.samples == int(w.astype(np.int64).sum())
    assert [h[0] for h in r.history] == sorted(h[0] for h in r.history) and r.history[-1][0] == r.spp
    # a pixel never listed after check c keeps film and mark from then on: replay the passes on the pixels each one touched
    film, mark, stopped, lo = np.zeros_like(r.film), np.zeros_like(r.film), np.zeros(nx * ny, np.int64), 0
    for c, (level, valid, above, active, kind) in enumerate(r.history):
        touched = np.ones(nx * ny, bool)
        if kind == 'list':
            touched[:] = False
            touched[r.lists[c - 1]] = True
        before, mark_before = film.copy(), mark.copy()
        for f in range(lo, level):
            if f == (r.history[0][0] // 2 if c == 0 else lo):
                mark[touched] = film[touched]
            film[touched] += R[f][touched]
        assert np.array_equal(film[~touched], before[~touched]) and np.array_equal(mark[~touched], mark_before[~touched])
        stopped[touched] = level
        lo = level
    assert np.array_equal(film.view(np.uint32), r.film.view(np.uint32)) and np.array_equal(mark.view(np.uint32), r.mark.view(np.uint32))
    assert np.all(w <= stopped)                   # no more than the level of the last pass that listed it (less: dilation lists a pixel again after a pass without it)


@pytest.mark.parametrize('dilate,above,level,mean_w,w_levels', [
    (0, [585, 257, 67, 7, 0], 64, 9.6, (4, 64)),
    (1, [585, 402, 182, 77, 16, 1, 0], 256, 50.6, (8, 256)),
])
def test_run_loop_on_the_oracles_films_s34(oracle_mod, dilate, above, level, mean_w, w_levels):
    nx = ny = 32
    R = oracle_frames(oracle_mod, 's34', nx, ny, 512)
    r = run_loop(R, nx, ny, 0.1, 512, min_spp=2, fraction=0.0, dilate=dilate, switch=1.0)
    print(dilate, r.history, r.samples, float(r.film[:, 3].mean()))
    assert [h[2] for h in r.history] == above
    assert r.converged and r.spp == level
    assert all(h[4] == 'list' for h in r.history[1:]) and r.history[0][4] == 'full'
    assert round(float(r.film[:, 3].mean()), 1) == mean_w
    assert (int(r.film[:, 3].min()), int(r.film[:, 3].max())) == w_levels
    if dilate == 0:                                  # without dilation a pixel that stops never comes back: w is the level it stopped at
        assert set(r.film[:, 3].astype(int).tolist()) <= {h[0] for h in r.history}
    check_invariants(r, R, nx, ny)


def test_run_loop_with_switch_zero_is_render_until(oracle_mod):
    nx = ny = 32
    R = oracle_frames(oracle_mod, 's34', nx, ny, 512)
    for dilate in (0, 1):
        r = run_loop(R, nx, ny, 0.1, 512, min_spp=2, fraction=0.0, dilate=dilate, switch=0.0)
        assert all(h[4] == 'full' for h in r.history) and np.all(r.film[:, 3] == r.spp) and np.all(r.mark[:, 3] == r.spp // 2)
        assert r.samples == r.spp * nx * ny
        full = np.zeros_like(r.film)
        for f in range(r.spp):
            full += R[f]
        assert np.array_equal(full.view(np.uint32), r.film.view(np.uint32))
        check_invariants(r, R, nx, ny)
    # a switch in between: full passes while many pixels are active, list passes after
    r = run_loop(R, nx, ny, 0.1, 512, min_spp=2, fraction=0.0, dilate=1, switch=0.5)
    kinds = [h[4] for h in r.history]
    assert kinds[1] == 'full' and 'list' in kinds and r.converged
    check_invariants(r, R, nx, ny)
    # the cap ends a loop that has not converged
    r = run_loop(R, nx, ny, 0.0, 24, min_spp=2, fraction=0.0, dilate=1, switch=1.0)
    assert not r.converged and r.spp == 24 and [h[0] for h in r.history] == [4, 8, 16, 24]
    check_invariants(r, R, nx, ny)


# ---------------------------------------------------------------- engine.render_adaptive's schedule, on stubs
class StubFilm:
    '''a film of `valid` pixels whose selection is what the test says it is at each level'''

    def __init__(self, engine, at, valid=100):
        self.engine, self.at, self.valid, self.log = engine, at, valid, engine.log

    def mark(self):
        self.log.append(('mark',))

    def select(self, noise, dilate=1):
        from ptina_amd._lib import NoiseStats, NoiseResult
        above, active = self.at(self.engine.level)
        self.log.append(('select', noise, dilate))
        return NoiseResult(NoiseStats(self.valid, above, 0.0, 0.0, noise)), active


class StubEngine:
    def __init__(self):
        self.level, self.log = 0, []

    def render(self, nframes=1):
        self.log.append(('render', nframes))
        self.level += nframes

    def render_selected(self, nframes=1, remark=False):
        self.log.append(('selected', nframes, remark))
        self.level += nframes


def test_render_adaptive_schedule_on_stubs():
    from ptina_amd.engine import render_adaptive, RenderAdaptive
    at = {8: (60, 80), 16: (30, 40), 32: (5, 9), 64: (0, 0)}
    eng = StubEngine()
    r = render_adaptive(eng, 0.05, 1024, min_spp=4, dilate=1, switch=0.5, film=StubFilm(eng, lambda level: at[level]))
    assert isinstance(r, RenderAdaptive) and (r.spp, r.converged) == (64, True)
    assert eng.log == [('render', 4), ('mark',), ('render', 4), ('select', 0.05, 1), ('mark',), ('render', 8), ('select', 0.05, 1),
                       ('selected', 16, True), ('select', 0.05, 1), ('selected', 32, True), ('select', 0.05, 1)]
    assert [(h[0], h[1].above, h[2], h[3]) for h in r.history] == [(8, 60, 80, 'full'), (16, 30, 40, 'full'), (32, 5, 9, 'list'), (64, 0, 0, 'list')]
    assert r.samples == 8 * 100 + 8 * 100 + 16 * 40 + 32 * 9 and isinstance(r.samples, int)
    # the fraction, the cap and the capped last pass
    eng = StubEngine()
    r = render_adaptive(eng, 0.05, 20, min_spp=4, fraction=0.05, switch=1.0, film=StubFilm(eng, lambda level: (6, 10)))
    assert (r.spp, r.converged) == (20, False) and [h[0] for h in r.history] == [8, 16, 20]
    assert eng.log[-2] == ('selected', 4, True)
    eng = StubEngine()
    r = render_adaptive(eng, 0.05, 20, min_spp=4, fraction=0.06, switch=1.0, film=StubFilm(eng, lambda level: (6, 10)))
    assert (r.spp, r.converged, len(r.history)) == (8, True, 1)


def test_render_adaptive_refuses_bad_arguments_before_it_renders():
    from ptina_amd.engine import render_adaptive
    for kw in (dict(max_spp=64, min_spp=0), dict(max_spp=31, min_spp=16), dict(max_spp=64, switch=-0.1), dict(max_spp=64, switch=1.5),
               dict(max_spp=64, switch=float('nan')), dict(max_spp=64, dilate=2), dict(max_spp=64, dilate=-1)):
        eng = StubEngine()
        with pytest.raises(ValueError, match='render_adaptive'):
            render_adaptive(eng, 0.05, film=StubFilm(eng, lambda level: (0, 0)), **kw)
        assert eng.log == []


def test_the_engine_the_worker_and_the_film_expose_adaptive_sampling():
    import inspect
    import ptina_amd.worker as worker
    import ptina_amd.engine as engine
    from ptina_amd.engine.path import PathEngine
    from ptina_amd.engine.brute import BruteEngine
    from ptina_amd.engine.mltpath import MLTPathEngine
    from ptina_amd.things import FilmTable
    assert list(inspect.signature(PathEngine.render_adaptive).parameters) == ['self', 'noise', 'max_spp', 'min_spp', 'fraction', 'dilate', 'switch']
    assert list(inspect.signature(engine.render_adaptive).parameters) == ['engine', 'noise', 'max_spp', 'min_spp', 'fraction', 'dilate', 'switch', 'film']
    d = inspect.signature(engine.render_adaptive).parameters
    assert (d['min_spp'].default, d['dilate'].default, d['fraction'].default, d['switch'].default) == (16, 1, 0.0, None)
    assert 0.05 <= engine.DEFAULT_SWITCH <= 1.0 and round(engine.DEFAULT_SWITCH / 0.05) * 0.05 == pytest.approx(engine.DEFAULT_SWITCH)
    assert list(inspect.signature(PathEngine.render_selected).parameters) == ['self', 'nframes', 'remark']
    for cls in (BruteEngine, MLTPathEngine):
        assert not hasattr(cls, 'render_adaptive') and not hasattr(cls, 'render_selected')
    assert callable(worker.render_adaptive) and 'render_adaptive' not in worker._PASS_THROUGH
    for name in ('select', 'get_selection', 'set_selection', 'get_samples', 'adapt_kernel_time'):
        assert callable(getattr(FilmTable, name))
    ns = {}
    exec('from ptina.engine.path import *', ns)
    assert ns['render_adaptive'] is engine.render_adaptive and ns['RenderAdaptive'] is engine.RenderAdaptive
    for text in (engine.render_adaptive.__doc__,):
        assert 'biased' in text and 'min_spp' in text and 'factor k' in text


def test_the_abi_declares_the_adaptive_entry_points():
    from ptina_amd import _lib
    lib = _lib.load_library()
    for s in ('mpt_adapt_select', 'mpt_adapt_get_list', 'mpt_adapt_set_list', 'mpt_render_selected', 'mpt_adapt_eval', 'mpt_adapt_kernel_time'):
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    # without a context every entry fails loudly
    assert lib.mpt_render_selected(None, 1, 0) == 1 and b'null context' in lib.mpt_last_error()
    assert lib.mpt_adapt_set_list(None, None, 0) == 1 and lib.mpt_adapt_select(None, 0.1, 1, None, None) == 1

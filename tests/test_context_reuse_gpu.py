'''
One context walked through growing and shrinking sizes (-m gpu): models, films, the Metropolis slab and the launch ring.  Every
buffer of the context is grown in place (csrc/miptina_ctx.h: DevBuf and the capacity groups), so what a reused context computes
must be what a fresh context computes at that size, bit for bit -- and a destroyed context must give its memory back, with
every stream, event and mapped word it made on the way (the owners of csrc/miptina_ctx.h).
Failed allocations are not provoked here.
'''

import ctypes as C

import numpy as np
import pytest

from helpers import setup_engine
from ptina_amd import scenes

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- 1. models through one context
# growth, a shrink under a kept capacity, growth past it; across the 8192 faces between the host and the device SAH pass and the
# 1024 of the finish kernel alone; 2 and 1 faces: one internal node, none
MODEL_SIZES = [2, 9000, 300, 20000, 1, 1500]
# (gpu_build, sah_build, wide_build): the default builders, the host LBVH, the host SAH pass + the host collapse
BUILDERS = [(1, -1, 1), (0, -1, 1), (1, 0, 0)]
TREE_OPTIONS = ['tree_depth', 'fast_depth', 'wide_nodes', 'wide_depth', 'wide_stack', 'sah_fallback']


def _built(c, builders):
    '''build with the given builders and download what the build leaves behind: the LBVH arrays, the wide records, the options'''
    from ptina_amd import _lib
    from ptina_amd.things import BVHTree
    for key, value in zip(('gpu_build', 'sah_build', 'wide_build'), builders):
        c.set_option(key, value)
    BVHTree().build()
    out = {k: np.asarray(v) for k, v in BVHTree().to_numpy().items()}
    nw = C.c_int(0)
    c.call('mpt_get_wide', None, None, 0, C.byref(nw))
    w = np.zeros((nw.value, 8, 4), np.float32)
    q = np.zeros((nw.value, 4, 4), np.float32)
    if nw.value:
        c.call('mpt_get_wide', _lib.fptr(w), _lib.fptr(q), nw.value, C.byref(nw))
    out['wnode'], out['qnode'] = w, q
    for k in TREE_OPTIONS:
        out[k] = np.asarray(c.get_option(k))
    return out


def test_models_through_one_context(fresh):
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import init_things, ModelPool
    models = {n: scenes.scene_random_tris(n, seed=n, edge=0.05)[:2] for n in MODEL_SIZES}
    want = {}
    for n in MODEL_SIZES:
        for b in BUILDERS:
            reset_all()
            init_things()
            ModelPool().load(*models[n])
            want[n, b] = _built(ctx(), b)
    reset_all()
    init_things()
    for n in MODEL_SIZES:
        ModelPool().load(*models[n])
        for b in BUILDERS:
            got = _built(ctx(), b)
            assert got.keys() == want[n, b].keys()
            for k, v in want[n, b].items():
                assert got[k].shape == v.shape and got[k].dtype == v.dtype and got[k].tobytes() == v.tobytes(), \
                    f'n {n}, builders {b}: {k} of the reused context differs from a fresh context\'s'
    # (the cases did take the paths they are here for)
    assert want[9000, BUILDERS[0]]['wide_nodes'] > 0 and want[1, BUILDERS[0]]['wide_nodes'] == 0
    assert want[2, BUILDERS[0]]['wide_nodes'] == 1


# ---------------------------------------------------------------- 2. films through one context
FILM_SIZES = [(64, 48), (200, 120), (32, 32), (256, 130)]


def _film_results(eng):
    '''4 path frames (and one preview frame for the denoiser's guides) from Sobol index 0 into a cleared film'''
    from ptina_amd.things import FilmTable
    from ptina_amd.engine.preview import PreviewEngine
    from ptina_amd.sampling.sobol import SobolSampler
    SobolSampler().reset()
    FilmTable().clear()
    eng.render(4)
    PreviewEngine().render(1)
    f = FilmTable()
    return [f.get_raw().copy(), np.array(f.get_image()), np.array(f.get_denoised())]


def test_films_through_one_context(fresh):
    from ptina_amd.common import reset_all
    from ptina_amd.things import FilmTable
    scene = scenes.scene_s34()
    want = {}
    for nx, ny in FILM_SIZES:
        reset_all()
        want[nx, ny] = _film_results(setup_engine(scene, nx, ny, mode='fast'))
    reset_all()
    eng = setup_engine(scene, *FILM_SIZES[0], mode='fast')
    for nx, ny in FILM_SIZES:
        FilmTable().set_size(nx, ny)
        got = _film_results(eng)
        for what, g, w in zip(('get_raw', 'get_image', 'get_denoised'), got, want[nx, ny]):
            assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), \
                f'{nx}x{ny}: {what} of the reused context differs from a fresh context\'s in {int((_bits(g) != _bits(w)).sum())} words'
        assert np.all(got[0][:, 3] == 4.0)


# ---------------------------------------------------------------- 3. the Metropolis slab after a film growth
def test_metropolis_slab_after_a_film_growth(fresh):
    '''chains, seed and iterations of test_mlt_gpu.py::test_determinism_and_launch_split.  The slab's record capacity stays
    (8 x 2^14 records both times) while its run table grows with the film'''
    from ptina_amd.common import reset_all
    from ptina_amd.things import FilmTable
    from ptina_amd.engine.mltpath import MLTPathEngine
    scene = scenes.get_scene('s978')

    def run():
        FilmTable().clear()
        e = MLTPathEngine(nchains=2**14, seed=1)
        e.reset()
        e.render(8)
        return FilmTable().get_raw().copy()

    setup_engine(scene, 96, 64, mode='fast')
    want = run()
    reset_all()
    setup_engine(scene, 32, 32, mode='fast')
    small = run()
    assert small[:, 3].sum() == 8 * 2**14
    FilmTable().set_size(96, 64)
    got = run()
    assert got[:, 3].sum() == 8 * 2**14
    assert np.array_equal(_bits(got), _bits(want)), f'{int((_bits(got) != _bits(want)).any(axis=1).sum())} pixels differ'


# ---------------------------------------------------------------- 4. destroy gives the memory back
def _free_bytes():
    '''hipMemGetInfo of the HIP runtime the library has loaded'''
    from ptina_amd import _lib
    _lib.load_library()
    with open('/proc/self/maps') as f:
        path = next(line.split()[-1] for line in f if 'libamdhip64' in line)
    hip = C.CDLL(path)
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


LEAK_CYCLES, LEAK_FACES, LEAK_FILM = 20, 20000, 256
PARENT_LOSS = 0                       # bytes the parent commit loses over the same cycles (MI355X, profiles/r12_host_refactor.json)
LEAK_ALLOWED = 2 * PARENT_LOSS


def test_destroy_gives_the_memory_back(fresh):
    '''20 cycles of init_things, load, build, 256 x 256 film, 4 frames, get_denoised, reset_all; the device's free memory before
    the first and after the last.  The parent of the commit that gave the buffers owners freed every one of them by hand in
    mpt_destroy, so what it loses over the same cycles is the HIP runtime keeping pools of its own: 0 bytes, measured on MI355X.
    Twice that is allowed: 0 bytes.  The allowance must stay below a quarter of what 20 cycles allocate (film 9 175 040 + tree
    11 279 712 bytes per cycle, counted below), so one group that is not freed cannot pass.
    Three cycles run before the first reading: in a process whose first contexts these are, the runtime's first-use allocations
    would otherwise be counted as the context's.  Per cycle of 45 in a fresh process, parent and change alike: 310 378 496 bytes,
    134 217 728, then 0 forty-three times -- two cycles settle it, a third is margin.'''
    from ptina_amd.common import reset_all
    from ptina_amd.things import FilmTable
    scene = scenes.scene_random_tris(LEAK_FACES, seed=LEAK_FACES, edge=0.05)

    def cycle():
        eng = setup_engine(scene, LEAK_FILM, LEAK_FILM, mode='fast')
        eng.render(4)
        FilmTable().get_denoised()
        reset_all()

    for _ in range(3):
        cycle()
    before = _free_bytes()
    for _ in range(LEAK_CYCLES):
        cycle()
    lost = before - _free_bytes()
    # bytes per pixel: 3 passes, the resolved image, 4 denoiser buffers of 16, the exported image of 12; per face: the model (96 + 4),
    # tgeo, tshade (64 each), tfast (48); per internal node: snode (32), fnode (64), wnode (128), qnode (64)
    film = LEAK_FILM * LEAK_FILM * (8 * 16 + 12)
    tree = LEAK_FACES * (96 + 4 + 64 + 64 + 48) + (LEAK_FACES - 1) * (32 + 64 + 128 + 64)
    print(f'free memory lost over {LEAK_CYCLES} cycles: {lost} bytes; one cycle allocates at least {film} + {tree} bytes; allowed {LEAK_ALLOWED}')
    assert LEAK_ALLOWED < LEAK_CYCLES * film // 4 < LEAK_CYCLES * (film + tree) // 4
    assert lost <= LEAK_ALLOWED, f'{lost} bytes of device memory did not come back after {LEAK_CYCLES} contexts'


# ---------------------------------------------------------------- 5. ring sizes through one context
# (pipe_depth, grid_div): two slots, all six with the smallest launches, three, what the library picks, two again
RING_WALK = [(2, 1), (6, 4), (3, 2), (0, 0), (2, 1)]
RING_FRAMES = (2, 2, 1, 2, 2, 1, 2, 2)                # eight launches of `batch` = 2 frames at the most: a ring of six slots wraps


def _ring_film(eng, depth, div):
    from ptina_amd.common import ctx
    from ptina_amd.things import FilmTable
    from ptina_amd.sampling.sobol import SobolSampler
    c = ctx()
    c.set_option('pipe_depth', depth)
    c.set_option('grid_div', div)
    SobolSampler().reset()
    FilmTable().clear()
    for frames in RING_FRAMES:
        eng.render(frames)
        c.call('mpt_flush')
    return FilmTable().get_raw().copy()


@pytest.mark.parametrize('lds', [1, 0])
def test_ring_sizes_through_one_context(fresh, lds):
    '''The slots of the launch ring (csrc/miptina_ctx.h MptRingSlot: stream, events, slab, points, queue heads, spill strip) are
    grown when a launch first needs them; the other tests give every ring configuration a context of its own.  Here one
    context walks through them, and every film must be the film of a fresh context with two slots, word for word.
    lds = 0: the 4-wide gather kernel, whose per-slot spill strips are then the ones grown; its wanted film is a fresh
    context's under the same option.'''
    from ptina_amd.common import ctx, reset_all
    scene = scenes.scene_s34()

    def context():
        reset_all()
        eng = setup_engine(scene, 64, 48, mode='fast')
        ctx().set_option('batch', 2)
        ctx().set_option('lds', lds)
        return eng

    want = _ring_film(context(), 2, 1)
    assert np.all(want[:, 3] == sum(RING_FRAMES))
    eng = context()
    for depth, div in RING_WALK:
        got = _ring_film(eng, depth, div)
        if not lds:
            assert ctx().get_option('last_kernel') == 2
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), \
            f'lds {lds}, pipe_depth {depth}, grid_div {div}: {int((_bits(got) != _bits(want)).sum())} words differ from a fresh context\'s film'
        assert np.all(got[:, 3] == sum(RING_FRAMES))


# ---------------------------------------------------------------- 6. every lazily made resource, then destroy
def test_every_lazily_made_resource_then_destroy(fresh):
    '''Three contexts that each make everything a context makes on demand -- the probe and the stress stream, the Metropolis
    engine's state and slab, the denoiser's and the display's buffers, timing events of all five launch timers -- and are then
    destroyed.  Cycles 2 and 3 compute what cycle 1 computed, bit for bit, and the device's free memory after cycle 3 is not
    below its value after cycle 2 (cycle 1 settles the runtime's own pools: test_destroy_gives_the_memory_back).
    The probe is the smallest the library accepts: 64 lanes with the 4 bytes of LDS per lane it asks for.'''
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import FilmTable
    from ptina_amd.engine.mltpath import MLTPathEngine
    from ptina_amd.engine.brute import BruteEngine
    from ptina_amd.engine.preview import PreviewEngine
    scene = scenes.scene_s34()

    def cycle():
        eng = setup_engine(scene, 32, 32, mode='fast')
        c, f = ctx(), FilmTable()
        eng.render(2)
        c.call('mpt_probe_kernel', 64, 256, None)
        c.call('mpt_stress_copies', 1, 2)
        c.call('mpt_stress_copies', 1, 0)                # ... waited for
        mlt = MLTPathEngine(nchains=2**10, seed=1)
        mlt.reset()
        mlt.render(2)
        brute = BruteEngine()
        brute.render(1)
        PreviewEngine().render(1)
        out = [np.array(f.get_denoised()), np.array(f.get_display())]
        out += [np.float32(f.last_exposure), f.get_raw().copy()]
        a, b, n = C.c_double(0), C.c_double(0), C.c_int(0)
        c.call('mpt_mlt_kernel_time', C.byref(a), C.byref(b), C.byref(n))
        launches = {'path': c.kernel_time()[1], 'mlt': n.value, 'brute': brute.kernel_time()[1],
                    'denoise': f.denoise_kernel_time()[1], 'display': f.display_kernel_time()[1]}
        assert all(v >= 1 for v in launches.values()), launches
        reset_all()
        return out, _free_bytes()

    first, _ = cycle()
    second, free2 = cycle()
    third, free3 = cycle()
    assert first[2] > 0 and first[3][:, 3].sum() >= 32 * 32 * 2 + 2 * 2**10      # (the path frames and the Metropolis splats at least)
    for n, got in ((2, second), (3, third)):
        for what, g, w in zip(('get_denoised', 'get_display', 'exposure_used', 'get_raw'), got, first):
            assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), f'cycle {n}: {what} differs from cycle 1'
    print(f'free memory after cycle 2: {free2} bytes, after cycle 3: {free3} bytes')
    assert free3 >= free2, f'{free2 - free3} bytes of device memory did not come back with the third context'

'''
CPU tests of the Metropolis engine's boundary (MLTPathEngine, ptina_amd/engine/mltpath.py): the C ABI
declares and binds its calls, the reference's module name resolves, and the numpy restatement of its
counter-based RNG (the contract of csrc/mlt_kernel.hip) gives the hand-worked values
and only uniforms in (0, 1).  The restatement below is also the one tests/test_mlt_gpu.py steps chains with.
'''

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MLT_CALLS = ('mpt_mlt_reset', 'mpt_mlt_set_param', 'mpt_mlt_render', 'mpt_mlt_get_state', 'mpt_mlt_set_state',
             'mpt_mlt_trace', 'mpt_mlt_kernel_time')

# ---------------------------------------------------------------- numpy restatement of mlt_kernel.hip
SLOT_LARGE, SLOT_ACCEPT, RESET_ITER = 0, 33, 0xffffffff


def pcg(v):
    v = np.asarray(v, np.uint32)
    with np.errstate(over='ignore'):
        s = v * np.uint32(747796405) + np.uint32(2891336453)
        w = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
    return (w >> np.uint32(22)) ^ w


def mlt_hash(seed, chain, it, slot):
    u32 = lambda x: np.asarray(x, np.uint64).astype(np.uint32)    # noqa: E731  (wrapping keys)
    with np.errstate(over='ignore'):
        h = pcg(u32(seed))
        h = pcg(h + u32(chain))
        h = pcg(h + u32(it))
        return pcg(h + u32(slot))


def mlt_uniform(seed, chain, it, slot):
    '''((h >> 9) + 0.5) * 2^-23: exact in f32, in (0, 1)'''
    h = mlt_hash(seed, chain, it, slot)
    return ((h >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def erfinv(x):
    '''common.py:338-352 in f32'''
    x = np.asarray(x, np.float32)
    sgn = np.where(x < 0, np.float32(-1), np.float32(1))
    y = (np.float32(1) - x) * (np.float32(1) + x)
    lnx = np.log(y)
    tt1 = np.float32(2.0 / (np.pi * 0.147)) + np.float32(0.5) * lnx
    tt2 = np.float32(1.0 / 0.147) * lnx
    return sgn * np.sqrt(-tt1 + np.sqrt(tt1 * tt1 - tt2))


def normaldist(u):
    return np.float32(np.sqrt(np.float32(2))) * erfinv(np.asarray(u, np.float32) * np.float32(2) - np.float32(1))


def wrap01(x):
    '''(x % 1) as Taichi computes it (x - floor(x)), a result of 1.0 wrapped to 0.0'''
    r = (x - np.floor(x)).astype(np.float32)
    return np.where(r >= np.float32(1), np.float32(0), r).astype(np.float32)


def reset_state(seed, nchains):
    c = np.arange(nchains, dtype=np.uint32)[:, None]
    j = np.arange(32, dtype=np.uint32)[None, :]
    return mlt_uniform(seed, c, RESET_ITER, 1 + j)


def propose(seed, X, it, lsp, sigma):
    '''mltpath.py:58-64 for every chain: (large-step mask, X_new)'''
    n = X.shape[0]
    c = np.arange(n, dtype=np.uint32)
    large = mlt_uniform(seed, c, it, SLOT_LARGE) < np.float32(lsp)
    u = mlt_uniform(seed, c[:, None], it, 1 + np.arange(32, dtype=np.uint32)[None, :])
    small = wrap01(X.astype(np.float32) + np.float32(sigma) * normaldist(u))
    return large, np.where(large[:, None], u, small).astype(np.float32)


def accept_mask(seed, n, it, L_new, L_old):
    '''mltpath.py:71-82: random() < min(1, (avg(L_new) + 1e-10) / (avg(L_old) + 1e-10)); NaN never accepted'''
    an = (L_new.astype(np.float32).sum(axis=1) / np.float32(3)) + np.float32(1e-10)
    ao = (L_old.astype(np.float32).sum(axis=1) / np.float32(3)) + np.float32(1e-10)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = an / ao
        acc = np.where(ratio > 1, np.float32(1), ratio)
        coin = mlt_uniform(seed, np.arange(n, dtype=np.uint32), it, SLOT_ACCEPT)
        return coin < acc, coin, acc


def splat_cells(X, nx, ny):
    i = np.clip(np.floor(X[:, 0] * np.float32(nx)).astype(np.int64), 0, nx - 1)
    j = np.clip(np.floor(X[:, 1] * np.float32(ny)).astype(np.int64), 0, ny - 1)
    return i * ny + j


# ---------------------------------------------------------------- tests
def test_header_and_ctypes_table_carry_the_mlt_calls():
    from ptina_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'miptina.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(mpt_[a-z0-9_]+)\s*\(', src))
    for name in MLT_CALLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name


def test_library_exports_the_mlt_calls():
    from ptina_amd import _lib
    lib = _lib.load_library()
    for name in MLT_CALLS:
        assert hasattr(lib, name), name


def test_reference_module_name_resolves():
    import ptina  # noqa: F401
    import importlib
    m = importlib.import_module('ptina.engine.mltpath')
    import ptina_amd.engine.mltpath as real
    assert m is real
    assert hasattr(m, 'MLTPathEngine') and hasattr(m, 'PathEngine') and hasattr(m, 'FilmTable')
    from ptina_amd.common import _singletons
    assert real.MLTPathEngine in _singletons        # @register: common.reset_all drops it


def test_pcg_hash_hand_worked_values():
    # pcg(0) by hand: s = 0 * 747796405 + 2891336453 = 2891336453; s >> 28 = 10, so the shift is 14: s >> 14 = 176473;
    # 176473 ^ s = 2891250268; * 277803737 mod 2^32 = 129708028 = w; w >> 22 = 30; 30 ^ w = 129708002
    assert 2891336453 >> 28 == 10 and 2891336453 >> 14 == 176473 and 176473 ^ 2891336453 == 2891250268
    assert (2891250268 * 277803737) % 2**32 == 129708028 and 129708028 >> 22 == 30 and 30 ^ 129708028 == 129708002
    assert int(pcg(0)) == 129708002
    assert int(pcg(1)) == 2831084092
    assert int(pcg(0xffffffff)) == 3861530882
    # the nested hash over (seed, chain, iteration, slot): pinned values (the kernel's reset stream is tied to this
    # restatement bit for bit on the GPU, tests/test_mlt_gpu.py::test_reset_state_matches_numpy)
    for key, want in (((0, 0, 0, 0), 2368882721), ((0, 1, 0, 0), 2010352870), ((7, 4095, 3, 33), 821400715),
                      ((1, 262143, 0xffffffff, 32), 569041930)):
        assert int(mlt_hash(*key)) == want
    assert int(mlt_hash(0, 0, 0, 0)) == int(pcg(int(pcg(int(pcg(int(pcg(0)) + 0)) + 0)) + 0))
    assert float(mlt_uniform(0, 0, 0, 0)) == ((2368882721 >> 9) + 0.5) * 2.0 ** -23


def test_uniforms_lie_in_the_open_interval():
    # the extremes of the mapping are exact and inside (0, 1)
    lo = (np.float32(0) + np.float32(0.5)) * np.float32(2.0 ** -23)
    hi = (np.float32((0xffffffff >> 9)) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert 0.0 < lo and hi < 1.0 and float(hi) == 1.0 - 2.0 ** -24
    # and a large sample of the generator
    c = np.arange(1 << 16, dtype=np.uint32)[:, None]
    u = mlt_uniform(12345, c, 7, np.arange(34, dtype=np.uint32)[None, :])
    assert u.dtype == np.float32
    assert (u > 0).all() and (u < 1).all()
    assert abs(float(u.mean()) - 0.5) < 2e-3
    assert np.isfinite(normaldist(u)).all()


def test_small_step_wrap_and_splat_clamp_edge_cases():
    # a coordinate just below 0 moves to just below 1, and one that rounds to 1.0 wraps to 0.0
    x = wrap01(np.array([-1e-9, -0.25, 1.25, 0.999999999, 1.0], np.float32))
    assert (x >= 0).all() and (x < 1).all()
    assert x[0] == 0.0 and x[1] == 0.75 and x[2] == 0.25 and x[4] == 0.0
    # the largest coordinate lands in the last column and row; the clamp keeps any product that reached the width in the film
    top = np.float32(1.0 - 2.0 ** -24)
    assert splat_cells(np.array([[top, top]], np.float32), 1000, 600)[0] == 999 * 600 + 599
    assert splat_cells(np.array([[1.0, 1.0], [0.0, 0.0]], np.float32), 1000, 600).tolist() == [999 * 600 + 599, 0]


def test_reset_and_proposal_restatement_shapes():
    X = reset_state(3, 64)
    assert X.shape == (64, 32) and (X > 0).all() and (X < 1).all()
    for lsp in (0.0, 0.25, 1.0):
        large, Xn = propose(3, X, 0, lsp, 0.01)
        assert Xn.dtype == np.float32 and (Xn >= 0).all() and (Xn < 1).all()
        if lsp == 0.0:
            assert not large.any() and np.abs(((Xn - X + 0.5) % 1) - 0.5).max() < 0.1
        if lsp == 1.0:
            assert large.all()

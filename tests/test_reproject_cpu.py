'''
The film's reprojection without a GPU: the numpy restatement (tests/reproject_ref.py) on cases worked by hand, the refusal rule
as the library's pure function (mpt_history_allowed, csrc/history_rule.h), the entries' answers to a NULL context, and the
share of the 978-triangle scene that a camera yaw of 2 degrees leaves its history (what test_reproject_gpu.py's "it helps" relies on).
'''

import ctypes as C

import numpy as np
import pytest

import reproject_ref as rr

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def film(nx, ny, seed=1, spp=16):
    '''accumulators of `spp` samples a pixel with random radiance sums, a -0 and a denormal among them'''
    rng = np.random.default_rng(seed)
    F = np.empty((nx * ny, 4), f32)
    F[:, :3] = rng.random((nx * ny, 3), dtype=f32) * f32(spp)
    F[:, 3] = spp
    F[0, 0], F[-1, 1] = f32(-0.0), f32(1e-41)
    return F


def flat_view(nx, ny, depth=5.0):
    '''a kept view that sees face 0 of object 0 at one depth everywhere'''
    return np.zeros(nx * ny, np.int32), np.zeros(nx * ny, np.int32), np.full(nx * ny, depth, f32)


@pytest.mark.parametrize('nx,ny', [(1, 1), (16, 16), (20, 12)])
def test_identity_keeps_every_word(nx, ny):
    F = film(nx, ny)
    face, obj, depth = flat_view(nx, ny)
    out, n = rr.resample(F, face, obj, depth, rr.identity_records(nx, ny, 0, 5.0), nx, ny, max_history=np.inf)
    assert np.array_equal(bits(out), bits(F))
    assert n == dict(kept=nx * ny, static=nx * ny, background_kept=0, disoccluded=0, offscreen=0, background_reset=0)
    # at the cap exactly nothing is scaled; below it the count comes down to the cap and the mean stays
    out16, _ = rr.resample(F, face, obj, depth, rr.identity_records(nx, ny, 0, 5.0), nx, ny, max_history=16)
    assert np.array_equal(bits(out16), bits(F))
    out4, _ = rr.resample(F, face, obj, depth, rr.identity_records(nx, ny, 0, 5.0), nx, ny, max_history=4)
    assert np.all(out4[:, 3] == 4)
    assert np.allclose(out4[:, :3] / 4, F[:, :3] / 16, rtol=1e-6, atol=1e-40)


def test_a_shift_by_whole_pixels_comes_back_shifted_exactly():
    nx, ny, dx, dy = 20, 12, 3, -2
    F = film(nx, ny, 2)
    face, obj, depth = flat_view(nx, ny)
    i, j = np.meshgrid(np.arange(nx, dtype=f32), np.arange(ny, dtype=f32), indexing='ij')
    m = rr.records(nx, ny, 0, i + dx, j + dy, 5.0, rr.NONE)
    out, n = rr.resample(F, face, obj, depth, m, nx, ny, max_history=np.inf)
    out, F3 = out.reshape(nx, ny, 4), F.reshape(nx, ny, 4)
    want = np.zeros_like(F3)
    want[:nx - dx, -dy:] = F3[dx:, :ny + dy]
    assert np.array_equal(bits(out), bits(want))
    assert n['kept'] == (nx - dx) * (ny + dy) and n['offscreen'] == nx * ny - n['kept'] and n['static'] == 0 and n['disoccluded'] == 0


def test_a_tap_outside_the_film_renormalises():
    nx, ny = 4, 4
    F = film(nx, ny, 3)
    face, obj, depth = flat_view(nx, ny)
    m = rr.records(nx, ny, 0, -0.25, 1.0, 5.0)              # taps (-1, 1) [outside, weight 0.25] and (0, 1) [0.75]
    out, n = rr.resample(F, face, obj, depth, m, nx, ny, max_history=np.inf)
    want = (f32(0.75) * F.reshape(nx, ny, 4)[0, 1]) / f32(0.75)
    assert np.array_equal(bits(out), bits(np.tile(want, (nx * ny, 1)))) and n['kept'] == 16
    m = rr.records(nx, ny, 0, 3.5, 3.5, 5.0)                # beyond the last pixel's centre: one tap in the film
    out, _ = rr.resample(F, face, obj, depth, m, nx, ny, max_history=np.inf)
    assert np.array_equal(bits(out[0]), bits((f32(0.25) * F.reshape(nx, ny, 4)[3, 3]) / f32(0.25)))
    for fx, fy in ((-1.0, 1.0), (4.0, 1.0), (1.0, -1.5), (np.nan, 1.0), (1e30, 1.0), (-np.inf, 0.0)):
        out, n = rr.resample(F, face, obj, depth, rr.records(nx, ny, 0, fx, fy, 5.0), nx, ny)
        assert not out.any() and n['offscreen'] == 16, (fx, fy)


def test_a_rejected_id_or_depth_renormalises_and_all_rejected_gives_zeros():
    nx, ny = 4, 4
    F = film(nx, ny, 4)
    F3 = F.reshape(nx, ny, 4)
    face, obj, depth = flat_view(nx, ny)
    obj = obj.reshape(nx, ny).copy()
    depth = depth.reshape(nx, ny).copy()
    m = rr.records(nx, ny, 0, 1.5, 1.5, 5.0)                # taps (1,1) (1,2) (2,1) (2,2), a quarter each
    obj[1, 2] = 7                                           # another object
    depth[2, 1] = f32(5.0) * (f32(1) + f32(0.021))          # just outside 2 %
    depth[2, 2] = f32(5.0) * (f32(1) - f32(0.019))          # just inside
    out, n = rr.resample(F, face, obj, depth, m, nx, ny, max_history=np.inf)
    A = (f32(-0.0) + f32(0.25) * F3[1, 1]) + f32(0.25) * F3[2, 2]
    assert np.array_equal(bits(out[5]), bits(A / f32(0.5))) and n['kept'] == 16
    F3[1, 1, 3] = 0                                         # a tap without samples
    out, _ = rr.resample(F, face, obj, depth, m, nx, ny, max_history=np.inf)
    assert np.array_equal(bits(out[5]), bits((f32(0.25) * F3[2, 2]) / f32(0.25)))
    obj[2, 2] = 7
    out, n = rr.resample(F, face, obj, depth, m, nx, ny)
    assert not out.any() and n == dict(kept=0, static=0, background_kept=0, disoccluded=16, offscreen=0, background_reset=0)


def test_background_pixels():
    nx, ny = 4, 4
    F = film(nx, ny, 5)
    face = np.full(nx * ny, -1, np.int32)
    face[3] = 2                                             # the kept view saw a face there: not background then
    obj, depth = np.where(face < 0, -1, 0).astype(np.int32), np.full(nx * ny, 1e6, f32)
    i, j = np.meshgrid(np.arange(nx, dtype=f32), np.arange(ny, dtype=f32), indexing='ij')
    kept = rr.records(nx, ny, -1, i, j, 0.0, rr.BACKGROUND)
    out, n = rr.resample(F, face, obj, depth, kept, nx, ny, max_history=np.inf)
    want = F.copy()
    want[3] = 0
    assert np.array_equal(bits(out), bits(want)) and n['background_kept'] == 15 and n['background_reset'] == 1
    out, n = rr.resample(F, face, obj, depth, rr.records(nx, ny, -1), nx, ny)
    assert not out.any() and n['background_reset'] == 16
    # the share: columns of another context come back empty and are not counted
    out, n = rr.resample(F, face, obj, depth, kept, nx, ny, max_history=np.inf, own=[False, True, True, False])
    assert not out.reshape(nx, ny, 4)[[0, 3]].any() and n['background_kept'] == 8 and sum(n.values()) == 8


# ---------------------------------------------------------------- the refusal rule
def test_history_allowed_names_every_refusal():
    from ptina_amd._lib import history_allowed
    ok = dict(have=True, kept_size=(64, 48), size=(64, 48), kept_faces=978, nfaces=978, tree_valid=True)
    assert history_allowed(**ok) == (0, '')
    assert history_allowed(**ok, max_history=np.inf) == (0, '')
    cases = [(dict(have=False), 1, ['no history', 'keep_history()']),
             (dict(size=(64, 47)), 2, ['the film is 64x47', 'kept at 64x48']),
             (dict(size=(48, 64)), 2, ['the film is 48x64']),
             (dict(nfaces=979), 3, ['the model has 979 faces', 'kept for 978']),
             (dict(tree_valid=False), 4, ['BVH not built', 'build_tree()']),
             (dict(max_history=0.0), 5, ['max_history', 'positive or +inf', 'got 0']),
             (dict(max_history=-1.0), 5, ['max_history']),
             (dict(max_history=np.nan), 5, ['max_history', 'nan']),
             (dict(depth_tol=0.0), 6, ['depth_tol', 'finite and positive']),
             (dict(depth_tol=np.inf), 6, ['depth_tol', 'inf']),
             (dict(depth_tol=np.nan), 6, ['depth_tol'])]
    for change, verdict, words in cases:
        rc, why = history_allowed(**dict(ok, **change))
        assert rc == verdict and why.startswith('reproject: ') and all(w in why for w in words), (change, rc, why)
    # the order of the refusals: the first cause is the one named
    assert history_allowed(**dict(ok, have=False, size=(1, 1), nfaces=0, tree_valid=False, max_history=0, depth_tol=0))[0] == 1
    assert history_allowed(**dict(ok, size=(1, 1), nfaces=0, tree_valid=False, max_history=0, depth_tol=0))[0] == 2
    assert history_allowed(**dict(ok, nfaces=0, tree_valid=False, max_history=0, depth_tol=0))[0] == 3
    assert history_allowed(**dict(ok, tree_valid=False, max_history=0, depth_tol=0))[0] == 4
    assert history_allowed(**dict(ok, max_history=0, depth_tol=0))[0] == 5


def test_history_allowed_cuts_its_words_to_the_buffer():
    from ptina_amd import _lib
    lib = _lib.load_library()
    for cap in (0, 1, 8, 40):
        why = C.create_string_buffer(b'x' * 63, 64)
        assert lib.mpt_history_allowed(0, 1, 1, 1, 1, 0, 0, 1, 32.0, 0.02, why if cap else None, cap) == 1
        if cap:
            assert len(why.value) == cap - 1 and why.raw[cap:63] == b'x' * (63 - cap)
    assert lib.mpt_history_allowed(0, 1, 1, 1, 1, 0, 0, 1, 32.0, 0.02, None, 64) == 1


def test_a_null_context_fails_with_the_calls_name():
    from ptina_amd import _lib
    lib = _lib.load_library()
    calls = dict(mpt_history_keep=(), mpt_history_reproject=(None, None), mpt_history_drop=(), mpt_history_get_motion=(None,),
                 mpt_history_get_gbuffer=(None, None, None), mpt_history_eval=(None, None, None, None, None, None, 1, 1, None, None),
                 mpt_history_kernel_time=(None, None, None))
    for name, args in calls.items():
        assert getattr(lib, name)(None, *args) != 0
        assert name in _lib.last_error() and 'null context' in _lib.last_error(), (name, _lib.last_error())


def test_the_python_surface():
    from ptina_amd import _lib, worker
    from ptina_amd.filmtable import FilmTable
    for name in ('keep_history', 'reproject', 'get_motion', 'drop_history', 'history_kernel_time'):
        assert callable(getattr(FilmTable, name))
    assert callable(worker.keep_history) and callable(worker.reproject)
    assert _lib.MOTION_DTYPE.itemsize == 20 and _lib.MOTION_DTYPE == rr.MOTION_DTYPE
    assert C.sizeof(_lib.HistoryStats) == 48 and C.sizeof(_lib.HistoryParams) == 8
    p = _lib.history_params()
    assert (p.max_history, p.depth_tol) == (32.0, f32(0.02))
    st = _lib.HistoryStats(5, 2, 3, 1, 4, 7)
    r = _lib.HistoryResult(st)
    assert r.astuple() == (5, 2, 3, 1, 4, 7) and r.pixels == 20 and r.kept_fraction == 0.4 and 'static=2' in repr(r)


# ---------------------------------------------------------------- the motion step on the reference geometry
def test_a_yaw_of_two_degrees_keeps_most_of_the_978_triangle_view():
    '''the geometry alone: the kept view and the motion of the yawed one in f64, through the resample step.  A turn about the
    centre of projection has no parallax, so only what enters at the film's edge is new'''
    from ptina_amd import scenes
    import visibility_ref as vr
    nx = ny = 64
    pos = vr.positions(scenes.scene_s978()[0])
    kept_cam = np.asarray(scenes.BENCH_CAMERA, np.float64)
    new_cam = rr.yawed(kept_cam, 2.0)
    assert np.allclose(rr.eye_of(kept_cam), rr.eye_of(new_cam))
    face, obj, depth = rr.gbuffer(kept_cam, pos, nx, ny)
    mo = rr.motion(kept_cam, new_cam, pos, pos, nx, ny)
    assert (face >= 0).all()                                    # the room is closed around the kept camera's view ...
    assert (mo['face'] >= 0).mean() > 0.95 and mo['placed'][mo['face'] >= 0].all()   # ... the turned one looks past the open side's edge
    shift = np.median(mo['fx'] - np.arange(nx)[:, None])
    assert 1.0 < abs(shift) < 3.5, shift                        # 2 degrees of a 60 degree view, 64 pixels wide
    F = np.ones((nx * ny, 4), f32) * f32(64)
    out, n = rr.resample(F, face, obj, depth, rr.motion_records(mo, nx, ny), nx, ny)
    share = n['kept'] / (nx * ny)
    print(f'yaw 2 degrees, s978 64x64: kept {share:.4f}, disoccluded {n["disoccluded"]}, offscreen {n["offscreen"]}')
    assert share > 0.9 and n['static'] == 0 and n['background_kept'] == 0
    assert np.abs(out[out[:, 3] > 0, 3] - 32).max() < 1e-4      # 64 samples a tap, capped to the default max_history
    # the same camera: every pixel looks at itself
    same = rr.motion(kept_cam, kept_cam, pos, pos, nx, ny)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    assert np.abs(same['fx'] - i).max() < 1e-9 and np.abs(same['fy'] - j).max() < 1e-9 and np.abs(same['d_exp'] - same['t']).max() < 1e-9

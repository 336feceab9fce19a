'''
CPU tests of the scatter's pure pieces: mpt_scatter_rule -- selection and placement on the host from
ptina_amd/csrc/scatter_rule.h -- against tests/scatter_ref.py bit for bit, the binary search's edge cases, the distribution of the
restatement itself, the frames of the matrices, the refusals that need no device, and tools/scatter_rule_check.cpp built with the
host sanitizers and run.  No GPU.
'''

import os
import shutil
import subprocess

import numpy as np
import pytest

import displace_ref as dr
import scatter_ref as sc
import subdiv_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64 = np.uint64
COUNTS = (1, 64, 257)
SHEAR = np.array([[1.7, 0.4, -0.2, 0.3], [0.1, 0.6, 0.5, -1.0], [-0.3, 0.2, 2.2, 0.5], [0, 0, 0, 1.0]])   # non-uniform and sheared


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(u64)


def _same_points(a, b):
    return a.shape == b.shape and all(np.array_equal(a[k].view(u64) if a[k].dtype == np.float64 else a[k], b[k].view(u64) if b[k].dtype == np.float64 else b[k])
                                      for k in ('face', 'b1', 'b2', 'scale', 'cy', 'sy'))


def _same_worlds(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a)[~(np.isnan(a) & np.isnan(b))], _bits(b)[~(np.isnan(a) & np.isnan(b))]) and \
        np.array_equal(np.isnan(a), np.isnan(b))


def quad():
    '''two faces over the unit square; face 0 has every corner uv at (0, 0), face 1 at (1, 1)'''
    verts = np.float32([(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)])
    p = verts[[[0, 2, 1], [0, 3, 2]]]
    rec = np.zeros((6, 8), np.float32)
    rec[:, :3], rec[:, 4] = p.reshape(6, 3), 1.0
    rec[3:, 6:] = 1.0
    return rec


QUAD_IMAGE = np.float32([[[0, 0, 0, 0], [0.5] * 4], [[0.5] * 4, [2.0, 2.0, 2.0, 2.0]]])    # a zero texel and a texel above 1


def surfaces():
    '''(name, records, world, density image or None)'''
    return [('octahedron', sr.fixture('octahedron'), np.eye(4), None),
            ('quad, one face without density', quad(), np.eye(4), QUAD_IMAGE),
            ('octahedron under a sheared matrix', sr.fixture('octahedron'), SHEAR, None)]


# ---------------------------------------------------------------- A: the rule against the restatement
def test_draws_of_the_array_restatement_equal_python_integers():
    key = sc.mix_int(sc.SEED)
    for i in (0, 1, 255, 2 ** 31, 2 ** 40 + 3):
        for k in (0, 3, 19):
            assert int(sc.draw(sc.SEED, np.array([i], u64), k)[0]) == sc.mix_int((key + 16 * i + k) & sc.M64)
    assert sc.mix_int(0) == 0xE220A8397B1DCDAF                            # SplitMix64's first output for the seed 0
    assert sc.unit(np.array([0, 2 ** 64 - 1], u64)).tolist() == [2.0 ** -54, 1.0]


@pytest.mark.parametrize('count', COUNTS)
def test_rule_equals_the_restatement_bit_for_bit(count):
    from ptina_amd import _lib
    for name, rec, world, image in surfaces():
        P = sc.world_corners(rec, world)
        dens = None if image is None else sc.density(rec, image, dr.R)
        q, _ = sc.shares(sc.weights(P, dens))
        if image is not None:
            assert dens.tolist() == [0.0, 1.0] and q.tolist() == [0, 1 << 24]
        for align, up, yaw, scale in ((sc.NORMAL, (0, 1, 0), True, (0.5, 1.5)), (sc.UP, (0.3, 2.0, -0.4), False, (2.0, 2.0)), (sc.UP, (0, 0, -3.0), True, (1.0, 1.25))):
            want_p, want_w, _ = sc.scatter(rec, world, sc.SEED + count, count, scale, align, up, yaw, q=q)
            rc, got_p, got_w = _lib.scatter_rule(P, q, sc.SEED + count, count, scale=scale, align=_lib.SCATTER_ALIGNS[align], up=up, random_yaw=yaw)
            assert rc == 0 and _same_points(got_p, want_p), (name, align, count)
            assert _same_worlds(got_w, want_w), (name, align, count)
            if image is not None:
                assert (got_p['face'] == 1).all()                         # the face without density is never chosen
            # instances first .. first + count - 1 are the same instances whatever the call's window
            rc, tail_p, tail_w = _lib.scatter_rule(P, q, sc.SEED + count, count - count // 2, first=count // 2, scale=scale, align=_lib.SCATTER_ALIGNS[align],
                                                   up=up, random_yaw=yaw)
            assert rc == 0 and _same_points(tail_p, want_p[count // 2:]) and _same_worlds(tail_w, want_w[count // 2:])


# ---------------------------------------------------------------- B: the binary search
def _t_of(seed, T, count):
    return (sc.draw(seed, np.arange(count, dtype=u64), 0) % u64(T)).astype(np.int64)


def test_binary_search_edge_cases():
    '''shares with runs of q = 0 at the beginning, in the middle and at the end: a face without a share is never chosen, and t = 0,
    t = T - 1 and every t equal to a cdf entry fall on the face the definition names.  With T = 12 and 4096 instances every t occurs'''
    from ptina_amd import _lib
    q = np.array([0, 0, 3, 1, 0, 0, 0, 2, 5, 1, 0, 0], np.uint32)
    cdf = sc.scan(q)
    T = int(cdf[-1])
    assert T == 12 and cdf.tolist() == [0, 0, 0, 3, 4, 4, 4, 4, 6, 11, 12, 12, 12]
    P = np.random.default_rng(3).normal(size=(q.size, 3, 3))
    count = 4096
    rc, got, _ = _lib.scatter_rule(P, q, 7, count)
    want = sc.select(cdf, 7, count)
    assert rc == 0 and _same_points(got, want)
    t = _t_of(7, T, count)
    assert set(t.tolist()) == set(range(T))                               # t = 0, t = T - 1, every cdf entry
    by_hand = np.array([2, 2, 2, 3, 7, 7, 8, 8, 8, 8, 8, 9])              # face of t = 0 .. 11
    assert np.array_equal(got['face'], by_hand[t])
    assert (q[got['face']] > 0).all()
    # one face; and a single share of 1 at either end of a table
    for qq, face in (([5], 0), ([1, 0, 0, 0], 0), ([0, 0, 0, 1], 3)):
        rc, got, _ = _lib.scatter_rule(P[:len(qq)], np.array(qq, np.uint32), 1, 64)
        assert rc == 0 and (got['face'] == face).all()
    assert _lib.scatter_rule(P, np.zeros(q.size, np.uint32), 1, 4)[0] == 2    # no share at all
    # T near 2^45: 2^21 - 1 faces of the full share
    big = np.full(2 ** 21 - 1, 1 << 24, np.uint32)
    cdf = sc.scan(big)
    assert int(cdf[-1]) == (2 ** 21 - 1) << 24
    want = sc.select(cdf, 11, 64)
    Pb = np.zeros((big.size, 3, 3))
    rc, got, _ = _lib.scatter_rule(Pb, big, 11, 64)
    assert rc == 0 and _same_points(got, want) and got['face'].max() > 2 ** 20


# ---------------------------------------------------------------- C: the distribution, on the restatement alone
def test_distribution_of_the_restatement():
    N = 8192
    sig = np.sqrt(N / 8 * 7 / 8)
    pts = sc.select(sc.scan(np.full(8, 1 << 24, np.uint32)), sc.SEED, N)
    counts = np.bincount(pts['face'], minlength=8)
    assert (np.abs(counts - N / 8) <= 5 * sig).all(), counts
    # faces of areas 1 : 3
    pts13 = sc.select(sc.scan(np.array([(1 << 24) // 3, 1 << 24], np.uint32)), sc.SEED, N)
    n0 = int((pts13['face'] == 0).sum())
    p0 = ((1 << 24) // 3) / ((1 << 24) // 3 + (1 << 24))
    assert abs(n0 - N * p0) <= 5 * np.sqrt(N * p0 * (1 - p0)), n0
    # inside a face: the barycentric mean (each coordinate of a uniform point has variance 1 / 18) and the mean yaw vector (1 / 2)
    b = np.stack([(1.0 - pts['b1']) - pts['b2'], pts['b1'], pts['b2']], axis=1)
    assert N >= 2048 and (b >= 0).all() and (b <= 1).all()
    assert (np.abs(b.mean(axis=0) - 1 / 3) <= 5 * np.sqrt(1 / 18 / N)).all(), b.mean(axis=0)
    yaw = np.stack([pts['cy'], pts['sy']], axis=1)
    assert np.allclose((yaw ** 2).sum(axis=1), 1.0, atol=1e-15)
    assert (np.abs(yaw.mean(axis=0)) <= 5 * np.sqrt(0.5 / N)).all(), yaw.mean(axis=0)
    # scales fill their range
    s = sc.select(sc.scan(np.full(8, 1 << 24, np.uint32)), sc.SEED, N, 0.5, 1.5)['scale']
    assert s.min() >= 0.5 and s.max() <= 1.5 and abs(s.mean() - 1.0) <= 5 * np.sqrt(1 / 12 / N)


# ---------------------------------------------------------------- D: the frames
def test_every_matrix_is_scale_times_a_right_handed_orthonormal_frame():
    for name, rec, world, image in surfaces():
        for align, up in ((sc.NORMAL, (0, 1, 0)), (sc.UP, (0.3, 2.0, -0.4)), (sc.UP, (0, 0, -1.0)), (sc.UP, (1.0, 0, 0)), (sc.UP, (0, -1.0, 0))):
            pts, W, _ = sc.scatter(rec, world, sc.SEED, 257, (0.25, 3.0), align, up, True, image=image, channel=dr.R)
            R = W[:, :3, :3] / pts['scale'][:, None, None]
            assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 1e-14, (name, align, up)
            assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-14
            assert (W[:, 3] == [0, 0, 0, 1]).all()
            P = sc.world_corners(rec, world)
            n = sc.unit_vector(sc.cross(P))[pts['face']] if align == sc.NORMAL else sc.unit_vector(up)
            assert np.abs(R[:, :, 1] - n).max() <= 1e-15                  # local +Y is the normal
            # the point lies on its face
            f = pts['face']
            d = ((W[:, :3, 3] - P[f, 0]) * sc.unit_vector(sc.cross(P))[f]).sum(axis=1)
            assert np.abs(d).max() <= 1e-14


def test_a_collapsed_face_gives_nan_as_the_restatement_does():
    from ptina_amd import _lib
    P = np.zeros((1, 3, 3))
    P[0, 1] = P[0, 2] = [1.0, 2.0, 3.0]                                  # two corners on one point
    q = np.array([5], np.uint32)
    rc, pts, W = _lib.scatter_rule(P, q, 3, 8)
    want = sc.place(P, sc.select(sc.scan(q), 3, 8))
    assert rc == 0 and np.isnan(W[:, :3, :3]).all() and np.isfinite(W[:, :3, 3]).all() and _same_worlds(W, want)
    rc, pts, W = _lib.scatter_rule(P, q, 3, 8, align='up')                # `up` does not ask for the normal
    assert rc == 0 and np.isfinite(W).all()


# ---------------------------------------------------------------- E: refusals that need no device
def test_rule_refusals():
    from ptina_amd import _lib
    P, q = np.zeros((2, 3, 3)), np.array([1, 1], np.uint32)
    assert _lib.scatter_rule(P, q, 0, 4)[0] == 0
    for bad in (dict(scale=(2.0, 1.0)), dict(scale=(float('nan'), 1.0)), dict(scale=(0.0, float('inf'))), dict(up=(0, 0, 0)), dict(up=(float('nan'), 1, 0)),
                dict(up=(float('inf'), 1, 0))):
        assert _lib.scatter_rule(P, q, 0, 4, **bad)[0] == 1, bad
    assert _lib.scatter_rule(P, q, 0, -1)[0] == 1 and _lib.scatter_rule(P, q, 0, 1, first=-1)[0] == 1
    with pytest.raises(ValueError, match='align'):
        _lib.scatter_params(align='tangent')
    with pytest.raises(ValueError, match='channel'):
        _lib.scatter_params(channel='luma')
    with pytest.raises(ValueError, match='negative'):
        _lib.scatter_params(density=-2)
    with pytest.raises(ValueError, match='3 components'):
        _lib.scatter_params(up=(0, 1))
    with pytest.raises(ValueError, match='shares'):
        _lib.scatter_rule(P, q[:1], 0, 1)


def test_restatement_flags_shares_near_a_boundary():
    x = np.array([3.0, 3.0 + 4 * np.spacing(3.0), 2.5, 1e6 - 1e-10, 1e6 - 1e-3])
    assert sc.near_boundary(x).tolist() == [True, True, False, True, False]
    # an affine matrix leaves the opposite faces of the octahedron with equal areas: the second largest share is flagged ...
    w = sc.weights(sc.world_corners(sr.fixture('octahedron'), SHEAR))
    assert (sc.near_boundary(sc.shares(w)[1]) & (w != w.max())).any()
    # ... and under scatter_ref.BENT the surfaces of the GPU tests show no such face but the largest itself, whose share is 2^24
    # by any evaluation (w / w = 1)
    for name, L in (('octahedron', 0), ('icosahedron', 1), ('fan7', 3), ('grid', 2)):
        rec = sr.fixture(name) if L == 0 else sr.fixture_subdivided(name, L)
        w = sc.weights(sc.world_corners(rec, sc.BENT))
        _, xs = sc.shares(w)
        assert not (sc.near_boundary(xs) & (w != w.max())).any(), name


# ---------------------------------------------------------------- F: the rule under the host sanitizers
def test_rule_check_program_builds_and_passes(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'scatter_rule_check')
    subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'scatter_rule_check.cpp'),
                    '-o', exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr[-2000:]

'''
CPU tests of mesh deformation: the numpy restatement the GPU tests hold the kernel to (tests/deform_ref.py),
the pure functions of the host runtime (mpt_deform_plan, mpt_skin_check: no context, no GPU) and tools.skin.joint_matrices.
'''

import os

import numpy as np
import pytest

import compose_ref
import deform_ref

u32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def mesh():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_compose.npz'))
    sizes = [g['mesh%d_p' % i].shape[0] for i in range(int(g['nmeshes']))]
    i = int(np.argmax(sizes))
    return deform_ref.records(g['mesh%d_p' % i], g['mesh%d_n' % i], g['mesh%d_t' % i])


def test_rest_pose_returns_the_positions_bits(mesh):
    '''zero weights and identity joints: the positions' bits come back, and the uvs'; the normals are normalised again'''
    g = np.random.default_rng(5)
    k = mesh.shape[0] // 3
    dp, dn, jt, wt = deform_ref.random_rig(g, k, T=3, nj=5)
    deltas = np.concatenate([dp.reshape(3, k * 3, 3), dn.reshape(3, k * 3, 3)], axis=2)
    wt = wt.reshape(k * 3, 4).copy()
    wt[:, 3] = 0
    wt[:, :3] = [0.5, 0.25, 0.25]                                          # sums to 1 exactly, in any order
    out = deform_ref.deform(mesh, deltas, np.zeros(3), jt.reshape(k * 3, 4), wt, np.tile(np.eye(4), (5, 1, 1)))
    assert out.dtype == np.float32 and out.shape == mesh.shape
    assert np.array_equal(out[:, [0, 1, 2, 6, 7]].view(u32), mesh[:, [0, 1, 2, 6, 7]].view(u32))
    assert np.allclose(np.linalg.norm(out[:, 3:6], axis=1), 1, atol=1e-6)
    plain = deform_ref.deform(mesh)
    assert np.array_equal(out.view(u32), plain.view(u32))


def test_one_joint_skin_agrees_with_the_world_matrix(mesh):
    '''a one-joint skin with weight 1 and matrix J, then world W, against the unskinned mesh under W . J: within the a-priori error
    bounds of the two f64 evaluations (compose_ref.error_bound) plus the f32 rounding of the deformed copy in between'''
    from ptina_amd.multimesh import compose_multiple_meshes
    g = np.random.default_rng(11)
    m = mesh.shape[0]
    J = deform_ref.random_joints(g, 1, amount=0.8)[0]
    W = compose_ref.grid_world(g, 1, 2)
    copy = deform_ref.deform(mesh, None, None, np.zeros((m, 4), np.int64), np.tile(np.float32([1, 0, 0, 0]), (m, 1)), J[None])
    pa, na, ta = deform_ref.split(copy)
    a, _ = compose_multiple_meshes([(pa, na, ta, W, 0)])
    pb, nb, tb = deform_ref.split(mesh)
    b, _ = compose_multiple_meshes([(pb, nb, tb, W @ J, 0)])
    # the first road: the f64 evaluation under J (bound e1), its rounding to f32 (half an ulp), both carried through W, and the f64
    # evaluation under W (bound e2); the second road: one f64 evaluation under W . J (bound e3; W . J itself: 4 roundings per entry)
    e1p, e1n = compose_ref.error_bound(mesh[:, :3], mesh[:, 3:6], J)
    e2p, e2n = compose_ref.error_bound(copy[:, :3], copy[:, 3:6], W)
    e3p, e3n = compose_ref.error_bound(mesh[:, :3], mesh[:, 3:6], W @ J)
    half_ulp = lambda x: 0.5 * np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)   # noqa: E731
    aW = np.abs(W[:3, :3])
    carried_p = (e1p + half_ulp(copy[:, :3])) @ aW.T
    eWJ = 4 * compose_ref.U * (np.abs(W) @ np.abs(J))
    carried_wj = np.abs(np.concatenate([mesh[:, :3].astype(np.float64), np.ones((m, 1))], axis=1)) @ eWJ[:3].T
    bound_p = carried_p + e2p + e3p + carried_wj
    assert np.all(np.abs(a[:, :3] - b[:, :3]) <= bound_p), float((np.abs(a[:, :3] - b[:, :3]) / bound_p).max())
    # normals: unit vectors; the in-between rounding moves a component by half an f32 ulp of 1 at most, which a 3x3 matrix and the
    # division by the length carry to at most 2 |W| |W^-1| times as much per component.  Both bounds are FIRST-ORDER in the
    # roundings (products of two errors are dropped, as compose_ref.error_bound drops them), not rigorous enclosures: with errors
    # of 2^-24 and 2^-53 the dropped terms are 2^-48 of the kept ones
    cond = np.linalg.norm(W[:3, :3], 2) * np.linalg.norm(np.linalg.inv(W[:3, :3]), 2)
    bound_n = 2 * cond * 3 * (2.0 ** -24 + e1n.max()) + e2n + e3n + 2 * cond * 3 * eWJ[:3, :3].max() / np.abs(W @ J)[:3, :3].max()
    assert np.all(np.abs(a[:, 3:6] - b[:, 3:6]) <= bound_n), float((np.abs(a[:, 3:6] - b[:, 3:6]) / bound_n).max())
    assert np.array_equal(a[:, 6:], b[:, 6:])


def test_deform_plan_against_its_restatement():
    from ptina_amd import _lib
    C = _lib.DEFORM_CHUNK
    assert C == 1024
    cases = [([], None), ([0], None), ([0, 0, 5], None), ([C], None), ([C, C + 1, 0, C - 1, 3 * C], None),      # runs that end on a chunk boundary
             ([C, 2 * C, 7], [0, 1, 1]), ([3, 4, 5], [0, 0, 0]), ([900, 0, 63], [1, 1, 0])]
    g = np.random.default_rng(3)
    for _ in range(200):
        n = int(g.integers(1, 12))
        k = g.choice([0, 1, 3, 63, 255, 256, C - 3, C, C + 3, 2 * C, 5 * C + 21], size=n)
        cases.append((k.tolist(), None if g.random() < 0.3 else g.integers(0, 2, size=n).tolist()))
    for corners, dirty in cases:
        got = _lib.deform_plan(corners, dirty)
        want = deform_ref.plan(corners, dirty, C)
        assert got == want, (corners, dirty, got, want)
        runs, blocks = got
        ends = [b + -(-corners[o] // C) for o, b in runs]
        assert [b for _, b in runs] == ([0] + ends[:-1] if runs else []) and blocks == (ends[-1] if runs else 0)
    with pytest.raises(ValueError):
        _lib.deform_plan([3, -1])
    with pytest.raises(ValueError):
        _lib.deform_plan([3, 3], [1])


def test_skin_check_accepts_and_refuses():
    from ptina_amd import _lib
    j = np.array([[0, 1, 2, 3], [4, 4, 4, 4]], np.uint16)
    w = np.array([[0.25, 0.25, 0.25, 0.25], [1, 0, 0, 0]], np.float32)
    assert _lib.skin_check(j, w, 5) == (0, '')
    assert _lib.skin_check(j, w, 256)[0] == 0
    assert _lib.skin_check(np.zeros((0, 4), np.uint16), np.zeros((0, 4), np.float32), 1) == (0, '')
    for nj in (0, -1, 257):
        rc, why = _lib.skin_check(j, w, nj)
        assert rc == 2 and 'njoints %d outside [1, 256]' % nj in why
    rc, why = _lib.skin_check(j, w, 4)
    assert rc == 3 and 'joints[1][0] names joint 4' in why
    for bad in (np.nan, np.inf, -np.inf):
        w2 = w.copy()
        w2[0, 2] = bad
        rc, why = _lib.skin_check(j, w2, 5)
        assert rc == 4 and 'weights[0][2] is not finite' in why
    w2 = w.copy()
    w2[1, 3] = -1e-30
    rc, why = _lib.skin_check(j, w2, 5)
    assert rc == 5 and 'weights[1][3] is negative' in why
    w2[1, 3] = -0.0                                                        # minus zero is zero
    assert _lib.skin_check(j, w2, 5)[0] == 0


def test_joint_matrices_of_a_three_joint_chain():
    from ptina_amd.tools.skin import joint_matrices

    def T(x, y, z):
        m = np.eye(4)
        m[:3, 3] = [x, y, z]
        return m

    def Rz90():
        m = np.eye(4)
        m[:2, :2] = [[0, -1], [1, 0]]
        return m
    # a chain along y with bones of length 1; the rest pose is unrotated, so inverse bind j is the shift by -j along y
    parents = [-1, 0, 1]
    local = np.stack([T(0, 0, 0), T(0, 1, 0) @ Rz90(), T(0, 1, 0)])
    inv_bind = np.stack([T(0, 0, 0), T(0, -1, 0), T(0, -2, 0)])
    pal = joint_matrices(parents, local, inv_bind)
    assert pal.shape == (3, 4, 4) and pal.dtype == np.float64
    assert np.array_equal(pal[0], np.eye(4))
    # joint 1 turns about (0, 1, 0): (x, y) -> (-(y - 1), 1 + x)
    assert np.array_equal(pal[1], np.array([[0, -1, 0, 1], [1, 0, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1.0]]))
    # joint 2 hangs one bone further along the turned axis: its rest origin (0, 2, 0) lands at (-1, 1, 0)
    assert np.array_equal(pal[2], pal[1])
    assert np.array_equal(pal[2] @ np.array([0, 2, 0, 1.0]), [-1, 1, 0, 1])
    assert np.array_equal(pal[:, 3], np.tile([0, 0, 0, 1.0], (3, 1)))
    with pytest.raises(ValueError, match='parents must come before'):
        joint_matrices([1, -1, 0], local, inv_bind)
    with pytest.raises(ValueError, match='parents must come before'):
        joint_matrices([0, 0, 1], local, inv_bind)
    with pytest.raises(ValueError):
        joint_matrices(parents, local[:2], inv_bind)
    assert joint_matrices(np.zeros(0, np.int64), np.zeros((0, 4, 4)), np.zeros((0, 4, 4))).shape == (0, 4, 4)

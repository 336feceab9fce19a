'''what the composition tests share (tests/test_compose_cpu.py, tests/test_compose_gpu.py, tests/golden/make_reference_compose_golden.py):
the margin that makes bit equality with an f64 evaluation in another order a fair demand, and the fixture's primitives.

An f64 evaluation of multimesh.py:58-65 in another summation order, or with FMA, differs from numpy's by a few f64 roundings of the
terms' magnitude.  Rounded to f32 the two can differ only where the value sits that close to an f32 rounding boundary (the midpoint
of two neighbouring f32 numbers).  margin() returns, per position and normal component, distance to the nearest boundary / a-priori
bound of the f64 evaluation error; the tests demand more than MARGIN everywhere.'''

import numpy as np

U = 2.0 ** -53
MARGIN = 64.0


def f32_boundary_distance(x):
    '''|x - nearest midpoint of two neighbouring f32 numbers|, x f64'''
    x = np.asarray(x, np.float64)
    r = x.astype(np.float32)
    other = np.where(r.astype(np.float64) > x, np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf)))
    mid = 0.5 * (r.astype(np.float64) + other.astype(np.float64))
    return np.abs(x - mid)


def error_bound(p, n, w):
    '''a-priori bounds of the f64 rounding error of pos [m,3] and nrm [m,3] (first order in U = 2^-53) for object-space p, n [m,3]
    and the world matrix w: a sum of k terms is off by at most k U (sum of |terms|) in any order, with or without FMA; a divide or
    square root adds one rounding'''
    p, n, w = np.asarray(p, np.float64), np.asarray(n, np.float64), np.asarray(w, np.float64)
    ph = np.concatenate([p, np.ones((p.shape[0], 1))], axis=1)
    num = ph @ w.T
    e_num = 4 * U * (np.abs(ph) @ np.abs(w).T)                       # [m,4]
    pos = num[:, :3] / num[:, 3:4]
    e_pos = np.abs(pos) * (e_num[:, :3] / np.maximum(np.abs(num[:, :3]), 1e-300) + e_num[:, 3:4] / np.abs(num[:, 3:4]) + U)
    e_pos = np.where(num[:, :3] == 0, e_num[:, :3] / np.abs(num[:, 3:4]), e_pos)
    nh = n @ w[:3, :3].T
    e_nh = 3 * U * (np.abs(n) @ np.abs(w[:3, :3]).T)
    l2 = (nh * nh).sum(axis=1, keepdims=True)
    e_l2 = (2 * np.abs(nh) * e_nh).sum(axis=1, keepdims=True) + 3 * U * l2
    ln = np.sqrt(l2)
    e_ln = e_l2 / (2 * ln) + U * ln
    nrm = nh / ln
    e_nrm = e_nh / ln + np.abs(nrm) * (e_ln / ln + U)
    return e_pos, e_nrm


def margin(primitives, out):
    '''min over every position and normal component of (distance of the f64 output to the nearest f32 rounding boundary) / (error
    bound), the smallest distance in f32 ulps, and the number of values; out [3n,8] f64 is the composition of the primitives'''
    at, worst, closest, count = 0, np.inf, np.inf, 0
    for p, n, t, w, m in primitives:
        k = np.asarray(p).shape[0] * 3
        if k == 0:
            continue
        e_pos, e_nrm = error_bound(np.asarray(p).reshape(k, 3), np.asarray(n).reshape(k, 3), w)
        val = out[at:at + k, :6]
        d = f32_boundary_distance(val)
        worst = min(worst, float((d / np.concatenate([e_pos, e_nrm], axis=1)).min()))
        closest = min(closest, float((d / np.spacing(np.abs(val).astype(np.float32)).astype(np.float64)).min()))
        count += val.size
        at += k
    return worst, closest, count


def fixture_primitives(g):
    '''the (p, n, t, w, m) tuples of tests/golden/reference_compose.npz; objects of one mesh share its array objects'''
    meshes = [(g['mesh%d_p' % i], g['mesh%d_n' % i], g['mesh%d_t' % i]) for i in range(int(g['nmeshes']))]
    prims = []
    for o, mesh in enumerate(g['obj_mesh']):
        p, n, t = meshes[int(mesh)]
        prims.append((p, n, t, g['obj_world'][o], None if g['obj_mtl_none'][o] else int(g['obj_mtl'][o])))
    return prims


# ---- the scene above the host tree passes' limit: a 96 x 96 height-field grid, 18 432 faces, as nine objects of three meshes
GRID_SEED = 1            # (chosen on the CPU: grid_scene(GRID_SEED) and its edit pass margin(); test_compose_gpu re-asserts it)


def grid_patch(kind, cells=32):
    '''one 32 x 32-cell patch of a height field over [0,1]^2, object space: p, n [2 cells^2, 3, 3] and t [.., 3, 2], f32'''
    lin = np.linspace(0.0, 1.0, cells + 1)
    u, v = np.meshgrid(lin, lin, indexing='ij')
    h = 0.12 * np.sin((3 + kind) * u + 0.3 * kind) * np.cos((2 + kind) * v) + 0.05 * kind * u * v
    q = np.stack([u, h, v], axis=-1)
    du, dv = np.gradient(h, lin, lin)
    nrm = np.stack([-du, np.ones_like(h), -dv], axis=-1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    uv = np.stack([u, v], axis=-1)

    def tris(a):
        c = a[:-1, :-1], a[1:, :-1], a[1:, 1:], a[:-1, 1:]
        return np.concatenate([np.stack([c[0], c[2], c[1]], axis=-2).reshape(-1, 3, a.shape[-1]),
                               np.stack([c[0], c[3], c[2]], axis=-2).reshape(-1, 3, a.shape[-1])])
    return tris(q).astype(np.float32), tris(nrm).astype(np.float32), tris(uv).astype(np.float32)


def grid_world(g, bx, bz):
    '''block (bx, bz) of the 3 x 3 grid over [-2,2]^2 at height ~1: a small rotation, a non-uniform scale, the translation'''
    ax = g.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = g.uniform(-0.08, 0.08)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    w = np.eye(4)
    w[:3, :3] = R @ np.diag(4.0 / 3.0 * g.uniform(0.97, 1.03, 3))
    w[:3, 3] = [-2 + 4.0 / 3.0 * bx + g.uniform(-0.01, 0.01), 0.8 + g.uniform(-0.2, 0.2), -2 + 4.0 / 3.0 * bz + g.uniform(-0.01, 0.01)]
    return w


def grid_scene(seed=GRID_SEED):
    '''(primitives, the edit (object, its new world)): nine objects, object o of mesh o % 3, material o % 3'''
    g = np.random.default_rng(seed)
    meshes = [grid_patch(k) for k in range(3)]
    prims = [(*meshes[o % 3], grid_world(g, o // 3, o % 3), o % 3) for o in range(9)]
    return prims, (4, grid_world(g, 1, 1))

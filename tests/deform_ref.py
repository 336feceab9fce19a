'''what the deformation tests share (tests/test_deform_cpu.py, tests/test_deform_gpu.py): a numpy restatement of the expressions
of ptina_amd/csrc/deform.hip, elementwise in f64 in exactly the written order -- no `@`, no einsum, no
sum() on the value path -- rounded to f32 once at the end.  Every operation is a correctly rounded IEEE + * / sqrt on both sides,
so the kernel is held to it bit for bit, with no margin rule.'''

import numpy as np


def deform(rec, deltas=None, w=None, joints=None, weights=None, mats=None):
    '''the deformed copy [m,8] f32 of the mesh records rec [m,8] f32 (pos3 nrm3 uv2 per corner):
    deltas [T,m,6] f32 (dp3 dn3) with the morph weights w [T] f64, or None;
    joints [m,4] integers and weights [m,4] f32 with the joint matrices mats [nj,4,4] f64, or None'''
    rec = np.asarray(rec)
    assert rec.dtype == np.float32 and rec.ndim == 2 and rec.shape[1] == 8
    q = [rec[:, k].astype(np.float64) for k in range(3)]
    m = [rec[:, 3 + k].astype(np.float64) for k in range(3)]
    if deltas is not None:
        deltas, w = np.asarray(deltas), np.asarray(w, np.float64)
        assert deltas.dtype == np.float32 and deltas.shape == (w.shape[0], rec.shape[0], 6)
        for t in range(w.shape[0]):
            if w[t] == 0.0:
                continue
            for k in range(3):
                q[k] = q[k] + w[t] * deltas[t, :, k].astype(np.float64)
                m[k] = m[k] + w[t] * deltas[t, :, 3 + k].astype(np.float64)
    if joints is not None:
        joints, weights, mats = np.asarray(joints), np.asarray(weights), np.asarray(mats, np.float64)
        assert weights.dtype == np.float32 and joints.shape == weights.shape == (rec.shape[0], 4) and mats.shape[1:] == (4, 4)
        a = [weights[:, i].astype(np.float64) for i in range(4)]
        j = [joints[:, i].astype(np.int64) for i in range(4)]
        qs, ms = [], []
        for r in range(3):
            M = [((a[0] * mats[j[0], r, c] + a[1] * mats[j[1], r, c]) + a[2] * mats[j[2], r, c]) + a[3] * mats[j[3], r, c] for c in range(4)]
            qs.append(((M[0] * q[0] + M[1] * q[1]) + M[2] * q[2]) + M[3])
            ms.append((M[0] * m[0] + M[1] * m[1]) + M[2] * m[2])
        q, m = qs, ms
    with np.errstate(invalid='ignore', divide='ignore'):
        ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        out = np.stack([q[0], q[1], q[2], m[0] / ln, m[1] / ln, m[2] / ln], axis=1).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([out, rec[:, 6:8]], axis=1))


def records(p, n, t=None):
    '''[3k,8] f32 mesh records of positions p [k,3,3], normals n [k,3,3] and texcoords t [k,3,2] (None: zeros): ModelPool.add_mesh's'''
    p, n = np.asarray(p), np.asarray(n)
    k = p.shape[0]
    t = np.zeros((k, 3, 2), np.float32) if t is None else np.asarray(t)
    return np.ascontiguousarray(np.concatenate([p.reshape(k * 3, 3), n.reshape(k * 3, 3), t.reshape(k * 3, 2)], axis=1), np.float32)


def split(rec):
    '''(p, n, t) as ModelPool.add_mesh / load_meshes take them, of records [3k,8]'''
    k = rec.shape[0] // 3
    return rec[:, 0:3].reshape(k, 3, 3).copy(), rec[:, 3:6].reshape(k, 3, 3).copy(), rec[:, 6:8].reshape(k, 3, 2).copy()


def plan(corners, dirty=None, chunk=1024):
    '''mpt_deform_plan restated (csrc/run_table.h's rule; subdiv_ref.plan passes its chunk): ([(object, first block), ...], blocks)'''
    runs, at = [], 0
    for o, k in enumerate(corners):
        if k == 0 or (dirty is not None and not dirty[o]):
            continue
        runs.append((o, at))
        at += -(-int(k) // chunk)
    return runs, at


def random_rig(g, k, T=0, nj=0):
    '''deltas [T,k,3,3] x 2 (f32), joints [k,3,4] (int64) and weights [k,3,4] (f32) for a mesh of k faces; None where T / nj is 0.
    Weights are positive and sum to about 1, not exactly: they are used as given'''
    dp = dn = jt = wt = None
    if T:
        dp = g.normal(scale=0.05, size=(T, k, 3, 3)).astype(np.float32)
        dn = g.normal(scale=0.2, size=(T, k, 3, 3)).astype(np.float32)
    if nj:
        jt = g.integers(0, nj, size=(k, 3, 4))
        wt = g.uniform(0.05, 1.0, size=(k, 3, 4))
        wt = (wt / wt.sum(axis=2, keepdims=True)).astype(np.float32)
    return dp, dn, jt, wt


def random_joints(g, nj, amount=0.3):
    '''[nj,4,4] f64 affine matrices: a rotation by up to `amount` radians about a random axis, a scale near 1, a small shift'''
    out = np.zeros((nj, 4, 4))
    for j in range(nj):
        ax = g.normal(size=3)
        ax /= np.linalg.norm(ax)
        th = g.uniform(-amount, amount)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        out[j, :3, :3] = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)) @ np.diag(g.uniform(0.9, 1.1, 3))
        out[j, :3, 3] = g.uniform(-0.1, 0.1, 3)
        out[j, 3, 3] = 1.0
    return out

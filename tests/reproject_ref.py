'''
The film's reprojection (FilmTable.keep_history / reproject; csrc/history_rule.h, history_kernel.hip, history.hip; DESIGN.md
section 3.18) restated in numpy, with nothing of ptina_amd.

resample()   the resample step in float32, operation for operation as include/miptina.h states it (numpy rounds every f32
             operation once, as the kernels do without contraction): the new accumulators and the counts, bit for bit.
motion()     the motion step in float64 from the model's positions and the two world-to-clip matrices alone: an exhaustive
             Moller-Trumbore over all triangles for every pixel's centre ray in the new view, and the hit point's place in the kept
             view.  The kernels round the camera's inverse, the ray and the hit to f32 on the way; the tests grant them the
             allowances the project already grants those roundings (visibility_ref.MARGIN in pixels, the query tolerance in depth).
'''

import numpy as np

MOTION_DTYPE = np.dtype([('cur_id', np.int32), ('fx', np.float32), ('fy', np.float32), ('d_exp', np.float32), ('flags', np.int32)])
NONE, STATIC, BACKGROUND = 0, 1, 2
COUNTS = ('kept', 'static', 'background_kept', 'disoccluded', 'offscreen', 'background_reset')
f32 = np.float32


def records(nx, ny, cur_id=-1, fx=np.nan, fy=np.nan, d_exp=np.nan, flags=NONE):
    '''motion records [nx * ny] from scalars or [nx, ny] arrays'''
    m = np.empty(nx * ny, MOTION_DTYPE)
    for key, value in (('cur_id', cur_id), ('fx', fx), ('fy', fy), ('d_exp', d_exp), ('flags', flags)):
        m[key] = np.broadcast_to(np.asarray(value), (nx, ny)).reshape(-1)
    return m


def identity_records(nx, ny, cur_id, d_exp, flags=STATIC):
    '''every pixel looks at its own place: fx = i, fy = j'''
    i, j = np.meshgrid(np.arange(nx, dtype=f32), np.arange(ny, dtype=f32), indexing='ij')
    return records(nx, ny, cur_id, i, j, d_exp, flags)


def resample(f_old, face, id_, depth, motion, nx, ny, max_history=32.0, depth_tol=0.02, own=None):
    '''-> (f_new [nx * ny, 4] f32, counts: a dict of COUNTS).  f_old [nx * ny, 4]; face, id_, depth [nx * ny] the kept G-buffer;
    motion MOTION_DTYPE [nx * ny]; own: [nx] bool, the columns of the context's share (None: all)'''
    F = np.ascontiguousarray(f_old, f32).reshape(nx, ny, 4)
    face = np.asarray(face, np.int32).reshape(nx, ny)
    id_ = np.asarray(id_, np.int32).reshape(nx, ny)
    depth = np.asarray(depth, f32).reshape(nx, ny)
    m = np.asarray(motion, MOTION_DTYPE).reshape(nx, ny)
    cur, fx, fy, dexp, flags = m['cur_id'], m['fx'], m['fy'], m['d_exp'], m['flags']
    mine = np.ones((nx, ny), bool) if own is None else np.broadcast_to(np.asarray(own, bool)[:, None], (nx, ny))
    cap, tolf = f32(max_history), f32(depth_tol)
    out = np.zeros((nx, ny, 4), f32)

    def capped(R):
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            s = cap / R[..., 3]
            return np.where((R[..., 3] > cap)[..., None], R * s[..., None], R)

    miss = cur < 0
    bg_kept = mine & miss & (flags == BACKGROUND) & (face == -1) & (F[..., 3] > 0)
    out[bg_kept] = capped(F)[bg_kept]
    hit = mine & ~miss
    with np.errstate(invalid='ignore'):
        onscreen = hit & (fx > f32(-1)) & (fx < f32(nx)) & (fy > f32(-1)) & (fy < f32(ny))
    gx, gy = np.where(onscreen, fx, f32(0)), np.where(onscreen, fy, f32(0))
    x0f, y0f = np.floor(gx), np.floor(gy)
    tx, ty = gx - x0f, gy - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    with np.errstate(invalid='ignore'):
        tol = tolf * dexp
    A = np.full((nx, ny, 4), -0.0, f32)
    B = np.full((nx, ny), -0.0, f32)
    for a in (0, 1):
        for b in (0, 1):
            bw = (tx if a else f32(1) - tx) * (ty if b else f32(1) - ty)
            qx, qy = x0 + a, y0 + b
            inside = (qx >= 0) & (qx < nx) & (qy >= 0) & (qy < ny)
            cx, cy = np.clip(qx, 0, nx - 1), np.clip(qy, 0, ny - 1)
            with np.errstate(invalid='ignore'):
                used = (onscreen & (bw > 0) & inside & (id_[cx, cy] == cur) & (np.abs(depth[cx, cy] - dexp) <= tol) & (F[cx, cy, 3] > 0))
            A = np.where(used[..., None], A + bw[..., None] * F[cx, cy], A)
            B = np.where(used, B + bw, B)
    kept = onscreen & (B > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        R = capped(A / B[..., None])
    out[kept] = R[kept]
    counts = dict(kept=int(kept.sum()), static=int((kept & (flags == STATIC)).sum()), background_kept=int(bg_kept.sum()),
                  disoccluded=int((onscreen & ~kept).sum()), offscreen=int((hit & ~onscreen).sum()),
                  background_reset=int((mine & miss & ~bg_kept).sum()))
    return out.reshape(nx * ny, 4), counts


# ---------------------------------------------------------------- the motion step, float64
def eye_of(pers):
    '''the centre of projection of a world-to-clip matrix: the point whose clip x, y and w vanish'''
    pers = np.asarray(pers, np.float64)
    rows = pers[[0, 1, 3]]
    return np.linalg.solve(rows[:, :3], -rows[:, 3])


def yawed(pers, degrees):
    '''the camera of `pers` turned about the world's y axis through its own centre of projection'''
    th = np.radians(degrees)
    R = np.eye(4)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
    c = eye_of(pers)
    T, Tinv = np.eye(4), np.eye(4)
    T[:3, 3], Tinv[:3, 3] = c, -c
    return np.asarray(pers, np.float64) @ T @ R @ Tinv


def centre_rays(pers, nx, ny):
    '''-> (o, d) [nx, ny, 3]: camera_generate of every pixel's centre, in f64 from the f64 inverse'''
    inv = np.linalg.inv(np.asarray(pers, np.float64))
    x, y = np.meshgrid((np.arange(nx) + 0.5) / nx * 2 - 1, (np.arange(ny) + 0.5) / ny * 2 - 1, indexing='ij')
    near = np.stack([x, y, -np.ones_like(x), np.ones_like(x)], axis=-1) @ inv.T
    far = np.stack([x, y, np.ones_like(x), np.ones_like(x)], axis=-1) @ inv.T
    o = near[..., :3] / near[..., 3:]
    d = far[..., :3] / far[..., 3:] - o
    return o, d / np.linalg.norm(d, axis=-1, keepdims=True)


def closest(pos, o, d):
    '''exhaustive Moller-Trumbore: pos [n, 3, 3], rays o, d [..., 3] -> (face (-1: none), t, u, v), each [...]'''
    pos = np.asarray(pos, np.float64)
    shape = o.shape[:-1]
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    best_t = np.full(o.shape[0], np.inf)
    best = np.full(o.shape[0], -1, np.int64)
    bu, bv = np.zeros(o.shape[0]), np.zeros(o.shape[0])
    for f in range(pos.shape[0]):
        e1, e2 = pos[f, 1] - pos[f, 0], pos[f, 2] - pos[f, 0]
        p = np.cross(d, e2)
        det = p @ e1
        with np.errstate(divide='ignore', invalid='ignore'):
            inv = 1.0 / det
            s = o - pos[f, 0]
            u = (s * p).sum(axis=1) * inv
            q = np.cross(s, e1)
            v = (d * q).sum(axis=1) * inv
            t = (q @ e2) * inv
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < best_t)
        best_t[ok], best[ok], bu[ok], bv[ok] = t[ok], f, u[ok], v[ok]
    return best.reshape(shape), best_t.reshape(shape), bu.reshape(shape), bv.reshape(shape)


def motion(pers_kept, pers_new, pos_kept, pos_new, nx, ny):
    '''-> dict of [nx, ny] arrays: face (-1: the centre ray of the new view hits nothing), t (its distance), u, v, and where the hit
    point lay in the kept view: fx, fy (pixel q's centre is q), d_exp (its distance from the kept camera's ray origin), placed
    (clip.w > 0)'''
    pos_kept, pos_new = np.asarray(pos_kept, np.float64), np.asarray(pos_new, np.float64)
    o, d = centre_rays(pers_new, nx, ny)
    face, t, u, v = closest(pos_new, o, d)
    tri = pos_kept[np.maximum(face, 0)]
    P = (1 - u - v)[..., None] * tri[..., 0, :] + u[..., None] * tri[..., 1, :] + v[..., None] * tri[..., 2, :]
    pk = np.asarray(pers_kept, np.float64)
    clip = P @ pk[:, :3].T + pk[:, 3]
    placed = (face >= 0) & (clip[..., 3] > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        x, y = clip[..., 0] / clip[..., 3], clip[..., 1] / clip[..., 3]
        near = np.stack([x, y, -np.ones_like(x), np.ones_like(x)], axis=-1) @ np.linalg.inv(pk).T
        origin = near[..., :3] / near[..., 3:]
    return dict(face=face, t=t, u=u, v=v, fx=(x + 1) * 0.5 * nx - 0.5, fy=(y + 1) * 0.5 * ny - 0.5,
                d_exp=np.linalg.norm(P - origin, axis=-1), placed=placed)


def gbuffer(pers, pos, nx, ny, first=None):
    '''the kept view in f64 -> (face, id, depth) [nx * ny]: id from the objects' first faces (None: 0 on every hit)'''
    o, d = centre_rays(pers, nx, ny)
    face, t, _, _ = closest(pos, o, d)
    hit = face >= 0
    obj = np.zeros_like(face) if first is None else np.searchsorted(np.asarray(first), face, side='right') - 1
    return (face.astype(np.int32).reshape(-1), np.where(hit, obj, -1).astype(np.int32).reshape(-1),
            np.where(hit, t, 1e6).astype(f32).reshape(-1))


def motion_records(mo, nx, ny, first=None):
    '''motion()'s answer as the records the resample step takes (no static and no background-kept pixel: a changed view)'''
    face = mo['face']
    obj = np.zeros_like(face) if first is None else np.searchsorted(np.asarray(first), face, side='right') - 1
    ok = mo['placed']
    return records(nx, ny, np.where(face >= 0, obj, -1), np.where(ok, mo['fx'], np.nan), np.where(ok, mo['fy'], np.nan),
                   np.where(ok, mo['d_exp'], np.nan), NONE)

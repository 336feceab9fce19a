'''
Which pixels of a film see a triangle with every one of their camera rays, and which with none: an exhaustive search over
all triangles in float64 numpy, with no tree, no sampler and nothing of ptina_amd.  Kernels and oracle alike are held to
it by rendering a scene in which a sample's radiance says exactly whether its camera ray hit (tests/test_visibility_gpu.py,
tests/test_visibility_ref_cpu.py).

Two arguments carry it.

EXACTNESS.  With every material `basecolor = 0, transmission = 1`, no lights and a constant world light W, a path that
hits anything ends with radiance exactly 0: lights_sample returns colour 0; clearcoat = 0 never takes the coat lobe;
transmission = 1 makes the specular rate 1, so the specular branch and in it the transmission choice are always taken, and
both of its outcomes multiply basecolor = 0 by finite factors over a positive pdf; the diffuse lobe carries
(1 - transmission) = 0.  The bounce's colour is exactly 0 in either build and the loop head ends the path.  A path that
hits nothing returns exactly W.  With W = (1, 1/2, 1/4) and F <= 8 frames every film sum is exact in f32: a raw pixel is
bit for bit (0, 0, 0, F) if all F camera rays hit and (F, F/2, F/4, F) if none did.

CONVEXITY.  camera_generate(x, y) is the preimage of the clip point (x, y) under the world-to-clip matrix: a world point
with clip coordinates (X, Y, Z, w), w > 0, Z / w > -1, lies on the ray of (X / w, Y / w), beyond the near plane where the
ray starts.  Every jittered ray of pixel (i, j) has x in [2 i / nx - 1, 2 (i + 1) / nx - 1] and y likewise: in pixel units
((x + 1) / 2 * nx) the rays of a pixel are the unit square at (i, j), and a triangle wholly beyond the near plane is its
projected 2-D triangle.  Both are convex, so corners decide:

  full hit    all four corners of the square lie at least `margin` inside all three edges of ONE triangle: every ray of
              the pixel hits that triangle
  full miss   for EVERY triangle, the square is separated from it by at least `margin`: by the triangle's bounding box or
              by one of its three edge lines (all four corners at least `margin` outside)
  left out    every other pixel.  A triangle whose projected area is below 1e-12 px^2 covers nothing and leaves out its
              whole bounding box

The margin (in pixels) absorbs what the renderers round: the f32 inverse of the camera matrix, the division in the pixel
coordinate, the triangle test's own rounding.

NEAREST MATERIAL.  w is the depth along the view axis and grows along every ray; a hit on a triangle has a w between the
smallest and the largest w of its vertices.  Among the triangles that fully cover a pixel take the one with the smallest
far bound (largest vertex w).  Its material is the nearest hit's material for every ray of the pixel if that far bound
times (1 + 1e-3) lies below the near bound (smallest vertex w) of every triangle of ANOTHER material that the pixel does
not fully miss.  A pixel where such another triangle exists is `contested`: there the walk had to order hits to be right.
'''

import numpy as np

MARGIN = 0.05
TINY_AREA = 1e-12          # px^2
DEPTH_GAP = 1e-3           # relative

_cache = {}


def positions(vertices):
    '''[3n][8] vertex rows (pos3 nrm3 uv2) -> [n][3][3] positions, f64 of the f32 values the renderers get'''
    v = np.asarray(vertices, np.float32)
    return v.reshape(-1, 3, v.shape[-1])[:, :, :3].astype(np.float64)


def project(pers, pos, nx, ny):
    '''-> (xy [n][3][2] in pixel units, w [n][3]); raises unless every vertex lies beyond the near plane'''
    pers = np.asarray(pers, np.float64)
    pos = np.asarray(pos, np.float64).reshape(-1, 3, 3)
    clip = pos @ pers[:, :3].T + pers[:, 3]
    w = clip[..., 3]
    if not (np.all(w > 0) and np.all(clip[..., 2] > -w)):
        bad = np.flatnonzero(~((w > 0) & (clip[..., 2] > -w)).all(axis=1))
        raise ValueError(f'{bad.size} triangles reach behind the near plane (first: {bad[0]}): a projected triangle is not their footprint')
    xy = np.empty(pos.shape[:2] + (2,))
    xy[..., 0] = (clip[..., 0] / w + 1.0) * 0.5 * nx
    xy[..., 1] = (clip[..., 1] / w + 1.0) * 0.5 * ny
    return xy, w


def _scan(pers, pos, mtlids, nx, ny, margin):
    xy, w = project(pers, pos, nx, ny)
    n = xy.shape[0]
    m = float(margin)
    cover = np.full((nx, ny), -1, np.int64)            # the fully covering triangle with the smallest far bound
    cover_far = np.full((nx, ny), np.inf)
    touched = np.zeros((nx, ny), bool)                 # some triangle is not separated from the pixel
    near = None
    if mtlids is not None:
        mtlids = np.asarray(mtlids, np.int64)
        near = np.full((nx, ny, int(mtlids.max()) + 1 if n else 1), np.inf)   # smallest near bound of the triangles of a material the pixel does not fully miss
    lo, hi = xy.min(axis=1), xy.max(axis=1)
    wfar, wnear = w.max(axis=1), w.min(axis=1)
    a, b = xy, np.roll(xy, -1, axis=1)
    e = b - a                                          # edge k: from vertex k to vertex k + 1
    area2 = e[:, 0, 0] * e[:, 1, 1] - e[:, 0, 1] * e[:, 1, 0]
    sign = np.where(area2 >= 0, 1.0, -1.0)
    length = np.sqrt((e ** 2).sum(axis=2))
    with np.errstate(divide='ignore', invalid='ignore'):
        # inward unit normal of every edge: distance(p) = nrm . p + off, positive inside
        nrm = np.stack([-e[..., 1], e[..., 0]], axis=2) * (sign[:, None] / length)[..., None]
    off = -(nrm * a).sum(axis=2)
    tiny = ~(np.abs(area2) * 0.5 >= TINY_AREA) | ~np.isfinite(nrm).all(axis=(1, 2))
    i0s = np.clip(np.floor(lo[:, 0] - m).astype(np.int64) - 1, 0, nx)
    i1s = np.clip(np.ceil(hi[:, 0] + m).astype(np.int64) + 1, 0, nx)
    j0s = np.clip(np.floor(lo[:, 1] - m).astype(np.int64) - 1, 0, ny)
    j1s = np.clip(np.ceil(hi[:, 1] + m).astype(np.int64) + 1, 0, ny)
    gi, gj = np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64)
    for t in range(n):
        i0, i1, j0, j1 = i0s[t], i1s[t], j0s[t], j1s[t]
        if i0 >= i1 or j0 >= j1:
            continue
        ci, cj = gi[i0:i1 + 1], gj[j0:j1 + 1]          # pixel corners
        # the bounding box separates the square [i, i + 1] x [j, j + 1] when it ends `m` before the box or starts `m` after it
        in_i = (ci[1:] > lo[t, 0] - m) & (ci[:-1] < hi[t, 0] + m)
        in_j = (cj[1:] > lo[t, 1] - m) & (cj[:-1] < hi[t, 1] + m)
        apart = ~(in_i[:, None] & in_j[None, :])
        if tiny[t]:
            full = None
        else:
            full = np.ones((i1 - i0, j1 - j0), bool)
            for k in range(3):
                d = (nrm[t, k, 0] * ci + off[t, k])[:, None] + (nrm[t, k, 1] * cj)[None, :]      # at the corners
                dmin = np.minimum(np.minimum(d[:-1, :-1], d[1:, :-1]), np.minimum(d[:-1, 1:], d[1:, 1:]))
                dmax = np.maximum(np.maximum(d[:-1, :-1], d[1:, :-1]), np.maximum(d[:-1, 1:], d[1:, 1:]))
                full &= dmin >= m
                apart |= dmax <= -m
        hitme = ~apart
        touched[i0:i1, j0:j1] |= hitme
        if near is not None:
            s = near[i0:i1, j0:j1, mtlids[t]]
            np.minimum(s, np.where(hitme, wnear[t], np.inf), out=s)
        if full is not None and full.any():
            cf, cv = cover_far[i0:i1, j0:j1], cover[i0:i1, j0:j1]
            better = full & (wfar[t] < cf)
            cf[better] = wfar[t]
            cv[better] = t
    return dict(cover=cover, cover_far=cover_far, touched=touched, near=near)


def _key(pers, pos, mtlids, nx, ny, margin):
    import hashlib
    h = hashlib.sha1()
    for a in (np.asarray(pers, np.float64), np.asarray(pos, np.float64), np.asarray(-1 if mtlids is None else mtlids, np.int64)):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest(), nx, ny, float(margin)


def _cached(pers, pos, mtlids, nx, ny, margin):
    key = _key(pers, pos, mtlids, nx, ny, margin)
    if key not in _cache:
        _cache[key] = _scan(pers, pos, mtlids, nx, ny, margin)
    return _cache[key]


def classify(pers, pos, nx, ny, margin=MARGIN):
    '''-> (full_hit, full_miss), [nx][ny] bool each.  pers: the 4 x 4 world-to-clip matrix, pos: [n][3][3]'''
    s = _cached(pers, pos, None, nx, ny, margin)
    return s['cover'] >= 0, ~s['touched']


def covering(pers, pos, nx, ny, margin=MARGIN):
    '''[nx][ny]: a triangle that fully covers the pixel (the one with the smallest far bound), -1 where none does'''
    return _cached(pers, pos, None, nx, ny, margin)['cover']


def nearest_material(pers, pos, mtlids, nx, ny, margin=MARGIN):
    '''-> (material [nx][ny] int, -1 where it is not known; contested [nx][ny] bool: known although a triangle of another
    material reaches into the pixel)'''
    s = _cached(pers, pos, mtlids, nx, ny, margin)
    mtlids = np.asarray(mtlids, np.int64)
    cover, far, near = s['cover'], s['cover_far'], s['near']
    covered = cover >= 0
    k = np.where(covered, mtlids[np.maximum(cover, 0)], 0)
    other = near.copy()
    np.put_along_axis(other, k[..., None], np.inf, axis=2)
    other = other.min(axis=2)
    known = covered & (far * (1.0 + DEPTH_GAP) < other)
    return np.where(known, k, -1), known & np.isfinite(other)

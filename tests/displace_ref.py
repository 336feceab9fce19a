'''what the displacement tests share (tests/test_displace_cpu.py, tests/test_displace_gpu.py): an independent numpy restatement of
texture displacement of a subdivided mesh as include/miptina.h defines it, written from the definition,
not from the kernel.  The parts section 3.19 already defines are subdiv_ref's (topology, refine, normals, refine_uv); added here
are the first-corner table (a plain loop), the bilinear sample and the two modes.  Every value is computed in f64 with one
correctly rounded IEEE + - * / sqrt floor per written operation, in the written order, and rounded to f32 once, so the kernel is
held to it bit for bit.

The definition, in short.  A last-level vertex takes the face-varying uv of its first corner: the lowest index 3 g + c into the
last level's faces that names it.  The image [nx][ny] is sampled at px = u (nx - 1), py = v (ny - 1): fx = floor(px), x0 = px - fx,
y0 = 1 - x0 (and fy, x1, y1 of py), texels wrapped by Python's modulo,
t = (((t11 x0) x1 + (t10 x0) y1) + (t00 y0) y1) + (t01 y0) x1.  Channel 0..3 is r, g, b, a; 4 is ((r + g) + b) / 3.  Mode 'normal':
p' = p + (strength (h - midlevel)) n with n the unrounded smooth normal of the undisplaced level; mode 'vector':
p' = p + strength ((r, g, b) - midlevel).  The normals of the result are subdiv_ref.normals of p'.'''

import numpy as np

import subdiv_ref as sr

NORMAL, VECTOR = 0, 1
R, G, B, A, MEAN = 0, 1, 2, 3, 4
MAX_UV = 2.0 ** 20


def first_corners(faces, nverts):
    '''per vertex the lowest index 3 g + c with faces[g][c] == vertex; ValueError for an id out of range or an untouched vertex'''
    corner = [None] * nverts
    for s, v in enumerate(np.asarray(faces).reshape(-1).tolist()):
        if not 0 <= v < nverts:
            raise ValueError('corner %d names vertex %d of %d' % (s, v, nverts))
        if corner[v] is None:
            corner[v] = s
    for v, s in enumerate(corner):
        if s is None:
            raise ValueError('no face touches vertex %d' % v)
    return np.array(corner, np.int64).reshape(nverts)


def sample(image, u, v):
    '''the bilinear sample [n,4] f64 of image [nx,ny,4] f32 at u, v [n] f64'''
    image = np.asarray(image)
    assert image.dtype == np.float32 and image.ndim == 3 and image.shape[2] == 4
    nx, ny = image.shape[:2]
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    px, py = u * float(nx - 1), v * float(ny - 1)
    fx, fy = np.floor(px), np.floor(py)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1 = px - fx, py - fy
    y0, y1 = 1.0 - x0, 1.0 - x1
    texel = image.astype(np.float64)

    def at(x, y):
        return texel[x % nx, y % ny]                                      # (numpy's % on integers is Python's: the sign of the divisor)
    t11, t10, t00, t01 = at(ix + 1, iy + 1), at(ix + 1, iy), at(ix, iy), at(ix, iy + 1)
    x0, x1, y0, y1 = x0[:, None], x1[:, None], y0[:, None], y1[:, None]
    return (((t11 * x0) * x1 + (t10 * x0) * y1) + (t00 * y0) * y1) + (t01 * y0) * x1


def height(rgba, channel):
    if channel == MEAN:
        return ((rgba[:, 0] + rgba[:, 1]) + rgba[:, 2]) / 3.0
    return rgba[:, channel]


def vertex_uv(src, topo, levels):
    '''[V_L,2] f64: the uv of every last-level vertex's first corner'''
    uv = np.asarray(src)[:, 6:8].astype(np.float64).reshape(-1, 3, 2)
    for _ in range(levels):
        uv = sr.refine_uv(uv)
    corner = first_corners(topo['faces'], len(topo['rings']))
    return uv.reshape(-1, 2)[corner]


def displace(rec, levels, image, mode, channel, strength, midlevel, control=None, topo=None):
    '''the displaced subdivided copy [3 k 4^levels, 8] f32 of the mesh records rec [3k,8] f32.  `control`: the records the positions
    and uvs are read from (an object's deformed copy), where the topology is rec's'''
    rec = np.asarray(rec)
    assert rec.dtype == np.float32 and rec.ndim == 2 and rec.shape[1] == 8
    topo = sr.topology(rec, levels) if topo is None else topo
    src = rec if control is None else np.asarray(control)
    assert src.shape == rec.shape and src.dtype == np.float32
    strength, midlevel = float(strength), float(midlevel)
    P = src[topo['first_corner'], :3].astype(np.float64)
    for l in range(1, levels + 1):
        P = sr.refine(P, topo['rules'][l])
    uv = vertex_uv(src, topo, levels)
    rgba = sample(image, uv[:, 0], uv[:, 1])
    with np.errstate(invalid='ignore', divide='ignore'):
        if mode == NORMAL:
            n = sr.normals(P, topo['rings'])
            s = strength * (height(rgba, channel) - midlevel)
            Pd = P + s[:, None] * n
        else:
            assert mode == VECTOR
            Pd = P + strength * (rgba[:, :3] - midlevel)
    N = sr.normals(Pd, topo['rings'])
    fuv = src[:, 6:8].astype(np.float64).reshape(-1, 3, 2)
    for _ in range(levels):
        fuv = sr.refine_uv(fuv)
    ids = topo['faces'].reshape(-1)
    out = np.concatenate([Pd[ids], N[ids], fuv.reshape(-1, 2)], axis=1).astype(np.float32)
    return np.ascontiguousarray(out)


def scaled_uv(rec):
    '''the records with their uvs taken to 3 uv - 1.25 (in f32): negative and above 1, so that the sample wraps on both sides'''
    out = np.array(rec, np.float32)
    out[:, 6:8] = np.float32(3.0) * out[:, 6:8] - np.float32(1.25)
    return out


def random_image(seed, nx, ny):
    '''[nx,ny,4] f32 in [0, 1)'''
    return np.random.default_rng(seed).random((nx, ny, 4), dtype=np.float32)

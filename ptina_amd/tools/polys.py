'''polygon cages for ModelPool.add_subdivision(scheme='catmull-clark'): the pool holds triangles, and a
polygon of n corners is n - 2 consecutive triangles, a fan about its first corner'''

import numpy as np


def fan(polygons, p, n=None, t=None):
    '''the fan-ordered mesh of the polygons -- lists of 3 to 64 indices into the vertices p [V,3] (normals n [V,3] or None: unit z, the
    subdivision does not read them; texcoords t [V,2] per vertex, or a list with one [n_j,2] array per polygon for face-varying
    texcoords, or None: zeros): (records [3k,8] f32, polys [m] int32).  Triangle i of polygon (c_0 .. c_n-1) is
    (c_0, c_i+1, c_i+2) -- not readobj's split of a quad, (0, 1, 2), (2, 3, 0).  records.reshape(k, 3, 8) splits into what
    ModelPool.add_mesh takes'''
    p = np.asarray(p, np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError('positions must be [V,3], got %s' % (p.shape,))
    n = np.tile(np.float32([0, 0, 1]), (p.shape[0], 1)) if n is None else np.asarray(n, np.float32)
    if n.shape != p.shape:
        raise ValueError('normals must be %s, got %s' % (p.shape, n.shape))
    per_vertex = t is None or not isinstance(t, (list, tuple))
    if per_vertex:
        t = np.zeros((p.shape[0], 2), np.float32) if t is None else np.asarray(t, np.float32)
        if t.shape != (p.shape[0], 2):
            raise ValueError('texcoords must be [%d,2] or one [n,2] array per polygon, got %s' % (p.shape[0], t.shape))
    elif len(t) != len(polygons):
        raise ValueError('%d arrays of texcoords for %d polygons' % (len(t), len(polygons)))
    out, polys = [], []
    for j, poly in enumerate(polygons):
        c = [int(v) for v in poly]
        if not 3 <= len(c) <= 64:
            raise ValueError('polygon %d has %d corners, outside [3, 64]' % (j, len(c)))
        if min(c) < 0 or max(c) >= p.shape[0]:
            raise ValueError('polygon %d names a vertex outside [0, %d)' % (j, p.shape[0]))
        uv = t[c] if per_vertex else np.asarray(t[j], np.float32)
        if uv.shape != (len(c), 2):
            raise ValueError('the texcoords of polygon %d must be [%d,2], got %s' % (j, len(c), uv.shape))
        corner = np.concatenate([p[c], n[c], uv], axis=1)
        for i in range(len(c) - 2):
            out += [corner[0], corner[i + 1], corner[i + 2]]
        polys.append(len(c))
    rec = np.ascontiguousarray(np.array(out, np.float32).reshape(-1, 8))
    return rec, np.array(polys, np.int32)

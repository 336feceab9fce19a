'''what the subdivision tests share (tests/test_subdiv_cpu.py, tests/test_subdiv_gpu.py): an independent numpy restatement of Loop
subdivision as include/miptina.h defines it -- its own weld, edges, rings and level-by-level refinement,
written from the definition with dictionaries and sets, not from the C++ -- and the procedural fixtures.  Every value is computed
in f64 with one correctly rounded IEEE + - * / sqrt per written operation, in the written order (no `@`, no sum(), no cross()), and
rounded to f32 once, so the kernels are held to it bit for bit.

The definition, in short.  Corners with equal positions (-0 equals +0) are one control vertex, numbered by first appearance, whose
position is its first corner's.  Level l -> l + 1: even vertices keep their ids, the vertex of edge e is V_l + e with the edges in
lexicographic order of (lower id, higher id), face (v0, v1, v2) becomes (v0, e01, e20), (v1, e12, e01), (v2, e20, e12),
(e01, e12, e20).  A vertex's ring follows the faces' winding; interior: from the lowest id; boundary: from the neighbour that
begins the fan.  Interior edge 0.375 (a + b) + 0.125 (c + d), boundary edge 0.5 (a + b), interior vertex (1 - n beta) v + beta s
with beta = 3/16 for n = 3, else 3 / (8 n), boundary vertex 0.75 v + 0.125 (p + q).  Normals: the sum of cross(a - v, b - v) over
the vertex's faces in ring order, from 0, normalised.  Texcoords face-varying, midpoints 0.5 (u_i + u_j).'''

import functools

import numpy as np

import deform_ref

VERT_INT, VERT_BND, EDGE_INT, EDGE_BND = 0, 1, 2, 3
CHUNK = 256


class Refusal(Exception):
    '''what the topology refuses: .kind is one of 'finite', 'degenerate', 'edge_faces', 'edge_direction', 'fan' '''
    def __init__(self, kind, what):
        Exception.__init__(self, '%s: %s' % (kind, what))
        self.kind = kind


# ---------------------------------------------------------------- topology
def weld(rec):
    '''(faces [k,3] of control vertex ids, first corner of every control vertex)'''
    pos = np.asarray(rec)[:, :3]
    if not np.isfinite(pos).all():
        bad = int(np.flatnonzero(~np.isfinite(pos).all(axis=1))[0])
        raise Refusal('finite', 'corner %d of face %d' % (bad % 3, bad // 3))
    ids, first, out = {}, [], []
    for s in range(pos.shape[0]):
        key = tuple(float(x) + 0.0 for x in pos[s])                      # (-0.0 + 0.0 is +0.0)
        if key not in ids:
            ids[key] = len(first)
            first.append(s)
        out.append(ids[key])
    faces = np.array(out, np.int64).reshape(-1, 3)
    for f, (a, b, c) in enumerate(faces):
        if a == b or b == c or c == a:
            raise Refusal('degenerate', 'face %d' % f)
    return faces, np.array(first, np.int64)


def level_topology(faces, V):
    '''of one level's faces [F,3]: (edges -- sorted list of (a, b, c, d), d None on a boundary --, {(a, b): edge id},
    rings -- per vertex (kind, [neighbours]))'''
    directed, count = {}, {}
    for f, (v0, v1, v2) in enumerate(faces.tolist()):
        for p, q, r in ((v0, v1, v2), (v1, v2, v0), (v2, v0, v1)):
            key = (min(p, q), max(p, q))
            count[key] = count.get(key, 0) + 1
            if count[key] > 2:
                raise Refusal('edge_faces', 'face %d on edge %s' % (f, key))
    for f, (v0, v1, v2) in enumerate(faces.tolist()):
        for p, q, r in ((v0, v1, v2), (v1, v2, v0), (v2, v0, v1)):
            if (p, q) in directed:
                raise Refusal('edge_direction', 'face %d runs %d -> %d again' % (f, p, q))
            directed[(p, q)] = r
    keys = sorted(count)
    edge_id = {key: e for e, key in enumerate(keys)}
    edges = []
    for a, b in keys:
        if count[(a, b)] == 2:
            edges.append((a, b, directed[(a, b)], directed[(b, a)]))
        else:
            edges.append((a, b, None, None))
    follows = [dict() for _ in range(V)]                                 # per vertex v: a -> b for its faces (v, a, b)
    for v0, v1, v2 in faces.tolist():
        follows[v0][v1] = v2
        follows[v1][v2] = v0
        follows[v2][v0] = v1
    rings = []
    for v in range(V):
        nxt = follows[v]
        entered = set(nxt.values())
        starts = [a for a in nxt if a not in entered]
        if len(starts) > 1:
            raise Refusal('fan', 'vertex %d' % v)
        cur = starts[0] if starts else min(nxt)
        ring, left = [cur], dict(nxt)
        while cur in left:
            cur = left.pop(cur)
            ring.append(cur)
        if left:
            raise Refusal('fan', 'vertex %d' % v)
        if starts:
            rings.append((VERT_BND, ring))
        else:
            assert ring[-1] == ring[0]
            rings.append((VERT_INT, ring[:-1]))
    return edges, edge_id, rings


def split_faces(faces, V, edge_id):
    out = []
    for v0, v1, v2 in faces.tolist():
        e01, e12, e20 = (V + edge_id[(min(p, q), max(p, q))] for p, q in ((v0, v1), (v1, v2), (v2, v0)))
        out += [(v0, e01, e20), (v1, e12, e01), (v2, e20, e12), (e01, e12, e20)]
    return np.array(out, np.int64).reshape(-1, 3)


def topology(rec, levels):
    '''the tables in the form _lib.subdiv_topology returns them: counts [levels+1,3], first_corner, rules {l: [(kind, ids)]},
    rings [(kind, ids)] of the last level, faces [F_L,3]'''
    faces, first = weld(rec)
    V = int(first.size)
    counts, rules = [], {}
    for l in range(levels + 1):
        edges, edge_id, rings = level_topology(faces, V)
        counts.append((V, len(edges), faces.shape[0]))
        if l == levels:
            break
        rules[l + 1] = [(k, list(r)) for k, r in rings] + [(EDGE_INT, [a, b, c, d]) if d is not None else (EDGE_BND, [a, b]) for a, b, c, d in edges]
        faces = split_faces(faces, V, edge_id)
        V += len(edges)
    return dict(counts=np.array(counts, np.int64).reshape(levels + 1, 3), first_corner=first, rules=rules,
                rings=[(k, list(r)) for k, r in rings], faces=faces)


# ---------------------------------------------------------------- values
def refine(P, rules):
    '''positions [V_l+1,3] f64 of the next level from P [V_l,3] f64'''
    out = np.empty((len(rules), 3), np.float64)
    for i, (kind, ids) in enumerate(rules):
        if kind == EDGE_INT:
            a, b, c, d = ids
            out[i] = 0.375 * (P[a] + P[b]) + 0.125 * (P[c] + P[d])
        elif kind == EDGE_BND:
            out[i] = 0.5 * (P[ids[0]] + P[ids[1]])
        elif kind == VERT_BND:
            out[i] = 0.75 * P[i] + 0.125 * (P[ids[0]] + P[ids[-1]])
        else:
            n = len(ids)
            s = P[ids[0]]
            for r in ids[1:]:
                s = s + P[r]
            beta = 0.1875 if n == 3 else 3.0 / (8.0 * n)
            out[i] = (1.0 - n * beta) * P[i] + beta * s
    return out


def normals(P, rings):
    out = np.empty((len(rings), 3), np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        for v, (kind, ids) in enumerate(rings):
            pairs = list(zip(ids, ids[1:])) + ([(ids[-1], ids[0])] if kind == VERT_INT else [])
            N = np.zeros(3)
            for a, b in pairs:
                A, B = P[a] - P[v], P[b] - P[v]
                N = N + np.array([A[1] * B[2] - A[2] * B[1], A[2] * B[0] - A[0] * B[2], A[0] * B[1] - A[1] * B[0]])
            out[v] = N / np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
    return out


def refine_uv(uv):
    '''[F,3,2] f64 -> [4F,3,2]'''
    u0, u1, u2 = uv[:, 0], uv[:, 1], uv[:, 2]
    m01, m12, m20 = 0.5 * (u0 + u1), 0.5 * (u1 + u2), 0.5 * (u2 + u0)
    kids = np.stack([np.stack([u0, m01, m20], 1), np.stack([u1, m12, m01], 1), np.stack([u2, m20, m12], 1), np.stack([m01, m12, m20], 1)], 1)
    return kids.reshape(-1, 3, 2)


def subdivide(rec, levels, topo=None, control=None):
    '''the subdivided copy [3 k 4^levels, 8] f32 of the mesh records rec [3k,8] f32.  `control`: the records the positions and uvs
    are read from (an object's deformed copy), where the topology is rec's'''
    rec = np.asarray(rec)
    assert rec.dtype == np.float32 and rec.ndim == 2 and rec.shape[1] == 8
    topo = topology(rec, levels) if topo is None else topo
    src = rec if control is None else np.asarray(control)
    assert src.shape == rec.shape and src.dtype == np.float32
    P = src[topo['first_corner'], :3].astype(np.float64)
    for l in range(1, levels + 1):
        P = refine(P, topo['rules'][l])
    N = normals(P, topo['rings'])
    uv = src[:, 6:8].astype(np.float64).reshape(-1, 3, 2)
    for l in range(levels):
        uv = refine_uv(uv)
    ids = topo['faces'].reshape(-1)
    out = np.concatenate([P[ids], N[ids], uv.reshape(-1, 2)], axis=1).astype(np.float32)
    return np.ascontiguousarray(out)


def plan(items, dirty=None, chunk=CHUNK):
    '''mpt_subdiv_plan restated: ([(job, first block), ...], blocks) -- deform_ref.plan's rule with this chunk'''
    return deform_ref.plan(items, dirty, chunk)


# ---------------------------------------------------------------- fixtures
def mesh_records(verts, faces, seam=3):
    '''[3k,8] f32 records of an indexed mesh: positions verts[faces] as f32 (shared vertices get equal bits), unit-z normals (not
    used), and texcoords from the x and y of the position -- shifted on every `seam`-th face, so that the edges of those faces are uv
    seams and the face-varying rule is exercised'''
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    k = faces.shape[0]
    p = verts[faces]                                                     # [k,3,3]
    n = np.tile(np.float32([0, 0, 1]), (k, 3, 1))
    t = (0.25 * p[:, :, :2] + 0.5).astype(np.float32)
    t[::seam] += np.float32([0.125, 0.0625])
    return np.ascontiguousarray(np.concatenate([p.reshape(-1, 3), n.reshape(-1, 3), t.reshape(-1, 2)], axis=1), np.float32)


def bipyramid(n):
    '''a closed fan of n faces around each apex: apexes of valence n over an equator of valence 4'''
    ang = 2 * np.pi * np.arange(n) / n
    verts = [(0, 0, 1.0), (0, 0, -0.8)] + [(np.cos(a), np.sin(a), 0.1 * np.cos(3 * a)) for a in ang]
    faces = []
    for i in range(n):
        a, b = 2 + i, 2 + (i + 1) % n
        faces += [(0, a, b), (1, b, a)]
    return verts, faces


def grid(nx=5, ny=5, bump=0.15):
    '''an open grid of nx x ny quads split in two along one diagonal: boundary, two corners of valence 2, a regular interior'''
    verts = [(x - nx / 2, y - ny / 2, bump * np.sin(1.3 * x + 0.7 * y)) for y in range(ny + 1) for x in range(nx + 1)]
    faces = []
    for y in range(ny):
        for x in range(nx):
            a = y * (nx + 1) + x
            b, c, d = a + 1, a + nx + 2, a + nx + 1
            faces += [(a, b, c), (a, c, d)]
    return verts, faces


def cylinder(n=8, rings=3):
    verts = [(np.cos(2 * np.pi * i / n), np.sin(2 * np.pi * i / n), 0.7 * r) for r in range(rings) for i in range(n)]
    faces = []
    for r in range(rings - 1):
        for i in range(n):
            a, b = r * n + i, r * n + (i + 1) % n
            faces += [(a, b, b + n), (a, b + n, a + n)]
    return verts, faces


def icosahedron():
    t = (1 + 5 ** 0.5) / 2
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    return verts, faces


def octahedron():
    verts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    faces = []
    for sx in (0, 1):
        for sy in (0, 1):
            for sz in (0, 1):
                x, y, z = sx, 2 + sy, 4 + sz
                faces.append((x, y, z) if (sx + sy + sz) % 2 == 0 else (x, z, y))
    return verts, faces


CLOSED = ('tetrahedron', 'octahedron', 'icosahedron', 'fan7', 'fan12')
NAMES = ('triangle', 'pair') + CLOSED + ('grid', 'cylinder')


@functools.lru_cache(maxsize=None)
def fixture(name):
    '''the records [3k,8] f32 of a fixture mesh (read-only: shared among the tests)'''
    if name == 'triangle':
        rec = mesh_records([(0, 0, 0), (1, 0, 0.25), (0.25, 1, 0)], [(0, 1, 2)], seam=1)
    elif name == 'pair':
        rec = mesh_records([(0, 0, 0), (1, 0, 0.25), (1, 1, 0), (-0.0, 1, 0.5)], [(0, 1, 2), (0, 2, 3)], seam=2)
    elif name == 'tetrahedron':
        rec = mesh_records([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)])
    elif name == 'octahedron':
        rec = mesh_records(*octahedron())
    elif name == 'icosahedron':
        rec = mesh_records(*icosahedron())
    elif name == 'fan7':
        rec = mesh_records(*bipyramid(7))
    elif name == 'fan12':
        rec = mesh_records(*bipyramid(12))
    elif name == 'grid':
        rec = mesh_records(*grid())
    elif name == 'cylinder':
        rec = mesh_records(*cylinder())
    else:
        raise KeyError(name)
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def fixture_topology(name, levels):
    return topology(fixture(name), levels)


@functools.lru_cache(maxsize=None)
def fixture_subdivided(name, levels):
    out = subdivide(fixture(name), levels, fixture_topology(name, levels))
    out.setflags(write=False)
    return out

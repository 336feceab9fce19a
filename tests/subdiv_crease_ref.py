'''what the crease tests share (tests/test_subdiv_crease_cpu.py, tests/test_subdiv_crease_gpu.py): a numpy restatement of Loop
subdivision with semi-sharp creases, corners and hard edges as include/miptina.h defines it, written
from the definition.  The weld, a level's edges and rings, the face split and the uv rule are subdiv_ref's; everything a crease
adds is restated here with dictionaries and lists.  Every value is computed in f64 with one correctly rounded IEEE operation per
written operation, in the written order, and rounded to f32 once, so the kernels are held to it bit for bit.

The definition, in short.  An edge of cage sharpness s0 has at level l s0 - l where that is positive, else 0 (inf stays inf); the
halves of a split edge inherit, the edges new inside a face have 0, a boundary edge counts as inf; the larger of what the two
faces on an edge state holds.  Edge point: E for s == 0, H = 0.5 (a + b) for s >= 1, else ((1 - s) E) + (s H).  Vertex point: a
flagged corner stays; S the sharpnesses > 0 around it in ring order, k their number; k <= 1: M; k == 2: C = 0.75 v + 0.125 (p + q)
with f = 0.5 (s1 + s2), C if f >= 1, else ((1 - f) M) + (f C); k >= 3: f = ((s1 + s2) + s3 ...) / k, v if f >= 1, else
((1 - f) M) + (f v).  Normals: the edges of sharpness > 0 at the last level (and the boundary) cut a vertex's fan into sectors; a
corner takes the normal sum over its own sector, from the sector's first hard edge.

The tables are in the form _lib.subdiv_topology_creased decodes the block to: a rule is (kind, variant, ids, parameter).'''

import functools
import math

import numpy as np

import subdiv_ref
from subdiv_ref import VERT_INT, VERT_BND, EDGE_INT, EDGE_BND, Refusal

PLAIN, BLEND_CREASE, BLEND_CORNER, FIXED = 0, 1, 2, 3
BLEND_EDGE = 1
INF = float('inf')


# ---------------------------------------------------------------- topology
def stated(rec, creases, corners):
    '''creases [k,3] as f64 of the f32 values and corners [k,3] as booleans, with the refusals'''
    k = np.asarray(rec).shape[0] // 3
    cr = np.zeros((k, 3), np.float32) if creases is None else np.asarray(creases, np.float32).reshape(k, 3)
    co = np.zeros((k, 3), bool) if corners is None else (np.asarray(corners).reshape(k, 3) != 0)
    for f in range(k):
        for j in range(3):
            if math.isnan(cr[f, j]):
                raise Refusal('crease', 'the crease of edge %d of face %d is not a number' % (j, f))
            if cr[f, j] < 0:
                raise Refusal('crease', 'the crease of edge %d of face %d is negative' % (j, f))
    return cr.astype(np.float64), co


def topology(rec, levels, creases=None, corners=None):
    '''counts [levels+1,3], first_corner, rules {l: [(kind, variant, ids, parameter)]}, rings [(kind, ids)] of the last level's
    vertices, records [(vertex, kind, ids)] of the last level, faces [F_L,3] of record ids'''
    cr, co = stated(rec, creases, corners)
    faces, first = subdiv_ref.weld(rec)
    V = int(first.size)
    creased = bool((cr > 0).any() or co.any())
    flagged = set(int(v) for v in faces[co])
    counts, rules = [], {}
    cage, V_below = None, 0
    for l in range(levels + 1):
        edges, edge_id, rings = subdiv_ref.level_topology(faces, V)
        counts.append((V, len(edges), faces.shape[0]))
        if l == 0:
            cage = [0.0] * len(edges)
            for f, (v0, v1, v2) in enumerate(faces.tolist()):
                for j, (p, q) in enumerate(((v0, v1), (v1, v2), (v2, v0))):
                    e = edge_id[(min(p, q), max(p, q))]
                    cage[e] = max(cage[e], float(cr[f, j]))
        else:
            cage = [cage[b - V_below] if a < V_below else 0.0 for a, b, _, _ in edges]

        def sharp(p, q):
            e = edge_id[(min(p, q), max(p, q))]
            if edges[e][3] is None:
                return INF
            s = cage[e] - float(l)
            return s if s > 0.0 else 0.0
        if l == levels:
            break
        out = []
        for v, (kind, ring) in enumerate(rings):
            S = [(sharp(v, r), r) for r in ring]
            S = [(s, r) for s, r in S if s > 0.0]
            if not creased:
                out.append((kind, PLAIN, list(ring), None))
            elif v in flagged:
                out.append((VERT_INT, FIXED, [], None))
            elif len(S) <= 1 or (kind == VERT_BND and len(S) == 2):
                out.append((kind, PLAIN, list(ring), None))
            elif len(S) == 2:
                f = 0.5 * (S[0][0] + S[1][0])
                if f >= 1.0:
                    out.append((VERT_BND, PLAIN, [S[0][1], S[1][1]], None))
                else:
                    out.append((VERT_INT, BLEND_CREASE, list(ring) + [S[0][1], S[1][1]], f))
            else:
                f = S[0][0] + S[1][0]
                for s, _ in S[2:]:
                    f = f + s
                f = f / float(len(S))
                out.append((VERT_INT, FIXED, [], None) if f >= 1.0 else (VERT_INT, BLEND_CORNER, list(ring), f))
        for a, b, c, d in edges:
            s = sharp(a, b) if creased else 0.0
            if d is None or s >= 1.0:
                out.append((EDGE_BND, PLAIN, [a, b], None))
            elif s == 0.0:
                out.append((EDGE_INT, PLAIN, [a, b, c, d], None))
            else:
                out.append((EDGE_INT, BLEND_EDGE, [a, b, c, d], s))
        rules[l + 1] = out
        faces = subdiv_ref.split_faces(faces, V, edge_id)
        V_below = V
        V += len(edges)
    # the last level: the sectors of every vertex, then the faces by record
    rings = [(k, list(r)) for k, r in rings]
    records = [None] * V
    sector_of = {}                                                       # (v, a) for the face (v, a, b) -> record
    for v, (kind, ring) in enumerate(rings):
        n = len(ring)
        if kind == VERT_BND:
            pairs = list(zip(ring, ring[1:]))
            cut = [0] + [i for i in range(1, n - 1) if sharp(v, ring[i]) > 0.0] + [n - 1]
            sectors = [ring[a:b + 1] for a, b in zip(cut, cut[1:])] if creased else [ring]
        else:
            pairs = list(zip(ring, ring[1:] + ring[:1]))
            cut = [i for i in range(n) if sharp(v, ring[i]) > 0.0] if creased else []
            turned = [ring[i:] + ring[:i] for i in cut]
            spans = [(b - a) % n or n for a, b in zip(cut, cut[1:] + cut[:1])]
            sectors = [t[:s] + [(t + t)[s]] for t, s in zip(turned, spans)]
        if len(sectors) <= 1 and (kind == VERT_BND or not sectors):
            records[v] = (v, kind, ring)
            for a, _ in pairs:
                sector_of[(v, a)] = v
            continue
        for j, sec in enumerate(sectors):
            r = v if j == 0 else len(records)
            if j == 0:
                records[v] = (v, VERT_BND, sec)
            else:
                records.append((v, VERT_BND, sec))
            for a in sec[:-1]:
                sector_of[(v, a)] = r
    rfaces = np.array([[sector_of[(v0, v1)], sector_of[(v1, v2)], sector_of[(v2, v0)]] for v0, v1, v2 in faces.tolist()], np.int64).reshape(-1, 3)
    return dict(counts=np.array(counts, np.int64).reshape(levels + 1, 3), first_corner=first, rules=rules, rings=rings, records=records,
                faces=rfaces, vfaces=faces)


# ---------------------------------------------------------------- values
def refine(P, rules):
    '''positions [V_l+1,3] f64 of the next level from P [V_l,3] f64'''
    out = np.empty((len(rules), 3), np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for i, (kind, variant, ids, par) in enumerate(rules):
            if kind == EDGE_INT:
                a, b, c, d = ids
                E = 0.375 * (P[a] + P[b]) + 0.125 * (P[c] + P[d])
                out[i] = E if variant == PLAIN else ((1.0 - par) * E) + (par * (0.5 * (P[a] + P[b])))
            elif kind == EDGE_BND:
                out[i] = 0.5 * (P[ids[0]] + P[ids[1]])
            elif kind == VERT_BND:
                out[i] = 0.75 * P[i] + 0.125 * (P[ids[0]] + P[ids[-1]])
            elif variant == FIXED:
                out[i] = P[i]
            else:
                ring = ids[:-2] if variant == BLEND_CREASE else ids
                n = len(ring)
                s = P[ring[0]]
                for r in ring[1:]:
                    s = s + P[r]
                beta = 0.1875 if n == 3 else 3.0 / (8.0 * n)
                M = (1.0 - n * beta) * P[i] + beta * s
                if variant == BLEND_CREASE:
                    C = 0.75 * P[i] + 0.125 * (P[ids[-2]] + P[ids[-1]])
                    M = ((1.0 - par) * M) + (par * C)
                elif variant == BLEND_CORNER:
                    M = ((1.0 - par) * M) + (par * P[i])
                out[i] = M
    return out


def normals(P, records):
    '''[R,3] f64: the normal of every record (vertex, kind, ids) on the positions P'''
    out = np.empty((len(records), 3), np.float64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for r, (v, kind, ids) in enumerate(records):
            pairs = list(zip(ids, ids[1:])) + ([(ids[-1], ids[0])] if kind == VERT_INT else [])
            N = np.zeros(3)
            for a, b in pairs:
                A, B = P[a] - P[v], P[b] - P[v]
                N = N + np.array([A[1] * B[2] - A[2] * B[1], A[2] * B[0] - A[0] * B[2], A[0] * B[1] - A[1] * B[0]])
            out[r] = N / np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
    return out


def positions(rec, topo, control=None, levels=None):
    '''the f64 positions of every level 0..L: a list of [V_l,3]'''
    src = np.asarray(rec if control is None else control)
    P = [src[topo['first_corner'], :3].astype(np.float64)]
    for l in sorted(topo['rules']):
        P.append(refine(P[-1], topo['rules'][l]))
    return P


def records_of(rec, topo, P_last, control=None):
    '''the subdivided copy [3 F_L, 8] f32 from the last level's (perhaps displaced) positions'''
    src = np.asarray(rec if control is None else control)
    levels = topo['counts'].shape[0] - 1
    N = normals(P_last, topo['records'])
    uv = src[:, 6:8].astype(np.float64).reshape(-1, 3, 2)
    for l in range(levels):
        uv = subdiv_ref.refine_uv(uv)
    ids = topo['faces'].reshape(-1)
    vert = np.array([r[0] for r in topo['records']], np.int64)
    out = np.concatenate([P_last[vert[ids]], N[ids], uv.reshape(-1, 2)], axis=1).astype(np.float32)
    return np.ascontiguousarray(out)


def subdivide(rec, levels, creases=None, corners=None, topo=None, control=None):
    '''the subdivided copy [3 k 4^levels, 8] f32 of the mesh records rec [3k,8] f32 (`control`: as subdiv_ref.subdivide)'''
    rec = np.asarray(rec)
    assert rec.dtype == np.float32 and rec.ndim == 2 and rec.shape[1] == 8
    topo = topology(rec, levels, creases, corners) if topo is None else topo
    return records_of(rec, topo, positions(rec, topo, control)[-1], control)


# ---------------------------------------------------------------- fixtures
def cube():
    '''12 triangles, vertices at +-1, outward winding'''
    verts = [(x, y, z) for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)]
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    faces = []
    for a, b, c, d in quads:
        faces += [(a, b, c), (a, c, d)]
    return verts, faces


def edge_creases(faces, pairs, default=0.0):
    '''[k,3] f32: the sharpness of {(p, q): s} on the face edges that run between indexed vertices p and q (either direction)'''
    out = np.full((len(faces), 3), default, np.float32)
    for f, (v0, v1, v2) in enumerate(faces):
        for j, (p, q) in enumerate(((v0, v1), (v1, v2), (v2, v0))):
            for key in ((p, q), (q, p)):
                if key in pairs:
                    out[f, j] = pairs[key]
    return out


def _cube_edges(verts, faces):
    '''the 12 edges of the cube among the 18 of its triangles: the two ends differ in one coordinate'''
    out = {}
    for v0, v1, v2 in faces:
        for p, q in ((v0, v1), (v1, v2), (v2, v0)):
            if sum(a != b for a, b in zip(verts[p], verts[q])) == 1:
                out[(p, q)] = True
    return out


NAMES = ('cube_inf', 'cube_1p5', 'octa_dart', 'fan7_spokes', 'grid_line', 'grid_corners', 'octa_two')


@functools.lru_cache(maxsize=None)
def fixture(name):
    '''(records [3k,8] f32, creases [k,3] f32 or None, corners [k,3] bool or None), read-only'''
    corners = None
    if name in ('cube_inf', 'cube_1p5'):
        verts, faces = cube()
        s = INF if name == 'cube_inf' else 1.5
        creases = edge_creases(faces, {e: s for e in _cube_edges(verts, faces)})
    elif name == 'octa_dart':                                             # one sharp edge: both its ends are dart ends and stay smooth
        verts, faces = subdiv_ref.octahedron()
        creases = edge_creases(faces, {(0, 2): INF})
    elif name == 'octa_two':                                              # the two faces on an edge state 0.25 and 2: the edge has 2
        verts, faces = subdiv_ref.octahedron()
        creases = edge_creases(faces, {(0, 2): 2.0, (2, 1): 2.0, (1, 3): 2.0, (3, 0): 2.0})
        f = [i for i, face in enumerate(faces) if 0 in face and 2 in face][0]
        j = [j for j in range(3) if {faces[f][j], faces[f][(j + 1) % 3]} == {0, 2}][0]
        creases[f, j] = 0.25
    elif name == 'fan7_spokes':                                           # three spokes of the valence-7 apex at 0.5, 1 and 2.5
        verts, faces = subdiv_ref.bipyramid(7)
        creases = edge_creases(faces, {(0, 3): 0.5, (0, 5): 1.0, (0, 8): 2.5})
    elif name in ('grid_line', 'grid_corners'):                           # a crease line x = 2 from boundary to boundary
        verts, faces = subdiv_ref.grid()
        line = {(y * 6 + 2, (y + 1) * 6 + 2): INF for y in range(5)}
        creases = edge_creases(faces, line)
        if name == 'grid_corners':
            flag = {0, 5, 30, 35}
            corners = np.array([[v in flag for v in face] for face in faces], bool)
            corners.setflags(write=False)
    else:
        raise KeyError(name)
    rec = subdiv_ref.mesh_records(verts, faces)
    rec.setflags(write=False)
    creases.setflags(write=False)
    return rec, creases, corners


@functools.lru_cache(maxsize=None)
def fixture_topology(name, levels):
    return topology(*((fixture(name)[0], levels) + fixture(name)[1:]))


@functools.lru_cache(maxsize=None)
def fixture_positions(name, levels):
    return positions(fixture(name)[0], fixture_topology(name, levels))


@functools.lru_cache(maxsize=None)
def fixture_subdivided(name, levels):
    out = records_of(fixture(name)[0], fixture_topology(name, levels), fixture_positions(name, levels)[-1])
    out.setflags(write=False)
    return out

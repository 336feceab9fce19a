'''what the Catmull-Clark tests share (tests/test_subdiv_cc_cpu.py, tests/test_subdiv_cc_gpu.py): an independent numpy restatement of
Catmull-Clark subdivision of a polygon cage with semi-sharp creases, corners and hard edges as include/miptina.h defines it
 -- its own polygon tables, edges, rings and level-by-level refinement, written from the definition with
dictionaries and lists, not from the C++; the weld alone is subdiv_ref's -- and the procedural fixtures.  Every value is computed in
f64 with one correctly rounded IEEE operation per written operation, in the written order, and rounded to f32 once, so the kernels
are held to it bit for bit.

The definition, in short.  Polygon j of n_j corners is n_j - 2 triangles of the mesh, a fan (c_0, c_i+1, c_i+2).  Level l -> l + 1:
even vertices keep their ids, the point of edge e is V_l + e (edges in lexicographic order of (lower id, higher id)), the point of
face j is V_l + E_l + j; face (c_0 .. c_n-1) becomes the quads (c_i, e(c_i, c_i+1), f, e(c_i-1, c_i)).  Face point
(((c_0 + c_1) + c_2) + ...) / n; interior edge 0.25 ((a + b) + (F1 + F2)), F1 the face that runs a -> b; boundary edge 0.5 (a + b);
interior vertex ((n - 2) / n) v + (1 / (n n)) (S_r + S_f); boundary vertex 0.75 v + 0.125 (p + q).  Creases as subdiv_crease_ref
states them.  Normals: the sum of cross(r_i - v, r_i+1 - v) over the ring of edge neighbours, by sectors.  The last level's quad
(v0, v1, v2, v3) is emitted as (v0, v1, v2), (v0, v2, v3).

The tables are in the form _lib.subdiv_topology_cc decodes the block to: a rule is (kind, variant, ids, parameter).'''

import functools

import numpy as np

import subdiv_ref
from subdiv_ref import VERT_INT, VERT_BND, EDGE_INT, EDGE_BND

PLAIN, BLEND_CREASE, BLEND_CORNER, FIXED, BLEND_EDGE, CC = 0, 1, 2, 3, 1, 4
INF = float('inf')


# ---------------------------------------------------------------- topology
def cage(rec, polys):
    '''(polygons: lists of control vertex ids, first corner of every control vertex, first triangle of every polygon)'''
    tris, first = subdiv_ref.weld(rec)
    polys = [3] * tris.shape[0] if polys is None else [int(n) for n in polys]
    assert sum(n - 2 for n in polys) == tris.shape[0]
    out, tri0, t = [], [], 0
    for n in polys:
        c = [int(tris[t][0]), int(tris[t][1])]
        for i in range(n - 2):
            assert int(tris[t + i][0]) == c[0] and int(tris[t + i][1]) == c[-1]
            c.append(int(tris[t + i][2]))
        assert len(set(c)) == n
        out.append(c)
        tri0.append(t)
        t += n - 2
    return out, first, tri0


def level_topology(faces, V):
    '''of one level's faces (corner lists): (edges -- sorted list of (a, b, f1, f2), f1 the face that runs a -> b and f2 the other, a
    boundary edge (a, b, its face, None) --, {(a, b): edge id}, rings -- per vertex (kind, [edge neighbours], [the face between r_i
    and r_i+1]))'''
    runs = {}
    for f, c in enumerate(faces):
        for i in range(len(c)):
            key = (c[i], c[(i + 1) % len(c)])
            assert key not in runs
            runs[key] = f
    keys = sorted(set((min(p, q), max(p, q)) for p, q in runs))
    edge_id = {key: e for e, key in enumerate(keys)}
    edges = []
    for a, b in keys:
        if (a, b) in runs and (b, a) in runs:
            edges.append((a, b, runs[(a, b)], runs[(b, a)]))
        else:
            edges.append((a, b, runs.get((a, b), runs.get((b, a))), None))
    follows = [dict() for _ in range(V)]                                 # per vertex v: a -> (b, f) for its faces f = (v, a, ..., b)
    for f, c in enumerate(faces):
        n = len(c)
        for i in range(n):
            follows[c[i]][c[(i + 1) % n]] = (c[(i - 1) % n], f)
    rings = []
    for v in range(V):
        nxt = follows[v]
        entered = set(b for b, _ in nxt.values())
        starts = [a for a in nxt if a not in entered]
        assert len(starts) <= 1
        cur = starts[0] if starts else min(nxt)
        ring, rfaces, left = [cur], [], dict(nxt)
        while cur in left:
            cur, f = left.pop(cur)
            ring.append(cur)
            rfaces.append(f)
        assert not left
        if starts:
            rings.append((VERT_BND, ring, rfaces))
        else:
            assert ring[-1] == ring[0]
            rings.append((VERT_INT, ring[:-1], rfaces))
    return edges, edge_id, rings


def topology(rec, levels, polys=None, creases=None, corners=None):
    '''counts [levels+1,3], first_corner, rules {l: [(kind, variant, ids, parameter)]}, rings [(kind, ids)] of the last level's
    vertices, records [(vertex, kind, ids)], quads1 [Q_1,2], faces [2 Q_L,3] of record ids, quads [Q_L,4] of vertex ids'''
    faces, first, tri0 = cage(rec, polys)
    ncorners = sum(len(c) for c in faces)
    cr = np.zeros(ncorners, np.float32) if creases is None else np.asarray(creases, np.float32).reshape(ncorners)
    co = np.zeros(ncorners, bool) if corners is None else (np.asarray(corners).reshape(ncorners) != 0)
    assert not np.isnan(cr).any() and not (cr < 0).any()
    cr = cr.astype(np.float64)
    V = int(first.size)
    creased = bool((cr > 0).any() or co.any())
    flat = [v for c in faces for v in c]
    flagged = set(v for v, flag in zip(flat, co) if flag)
    quads1 = [(tri0[j], len(c) | i << 8) for j, c in enumerate(faces) for i in range(len(c))]
    counts, rules = [], {}
    sharpness, V_below = None, 0
    for l in range(levels + 1):
        edges, edge_id, rings = level_topology(faces, V)
        E, F = len(edges), len(faces)
        counts.append((V, E, F))
        if l == 0:
            sharpness, s = [0.0] * E, 0
            for c in faces:
                for i in range(len(c)):
                    p, q = c[i], c[(i + 1) % len(c)]
                    e = edge_id[(min(p, q), max(p, q))]
                    sharpness[e] = max(sharpness[e], float(cr[s]))
                    s += 1
        else:
            sharpness = [sharpness[b - V_below] if a < V_below else 0.0 for a, b, _, _ in edges]

        def sharp(p, q):
            e = edge_id[(min(p, q), max(p, q))]
            if edges[e][3] is None:
                return INF
            s = sharpness[e] - float(l)
            return s if s > 0.0 else 0.0
        if l == levels:
            break
        fp = V + E

        def smooth(kind, ring, rfaces, blend, tail, par):
            if kind == VERT_BND:
                return (VERT_BND, PLAIN, list(ring), None)
            return (VERT_INT, CC | blend, list(ring) + [fp + f for f in rfaces] + tail, par)
        out = []
        for v, (kind, ring, rfaces) in enumerate(rings):
            S = [(sharp(v, r), r) for r in ring]
            S = [(s, r) for s, r in S if s > 0.0]
            if not creased:
                out.append(smooth(kind, ring, rfaces, PLAIN, [], None))
            elif v in flagged:
                out.append((VERT_INT, FIXED, [], None))
            elif len(S) <= 1 or (kind == VERT_BND and len(S) == 2):
                out.append(smooth(kind, ring, rfaces, PLAIN, [], None))
            elif len(S) == 2:
                f = 0.5 * (S[0][0] + S[1][0])
                if f >= 1.0:
                    out.append((VERT_BND, PLAIN, [S[0][1], S[1][1]], None))
                else:
                    out.append(smooth(kind, ring, rfaces, BLEND_CREASE, [S[0][1], S[1][1]], f))
            else:
                f = S[0][0] + S[1][0]
                for s, _ in S[2:]:
                    f = f + s
                f = f / float(len(S))
                out.append((VERT_INT, FIXED, [], None) if f >= 1.0 else smooth(kind, ring, rfaces, BLEND_CORNER, [], f))
        for a, b, f1, f2 in edges:
            s = sharp(a, b) if creased else 0.0
            if f2 is None or s >= 1.0:
                out.append((EDGE_BND, PLAIN, [a, b], None))
            elif s == 0.0:
                out.append((EDGE_INT, CC, [a, b, fp + f1, fp + f2], None))
            else:
                out.append((EDGE_INT, CC | BLEND_EDGE, [a, b, fp + f1, fp + f2], s))
        for c in faces:
            out.append((EDGE_BND, CC, list(c), None))
        rules[l + 1] = out
        nxt = []
        for j, c in enumerate(faces):
            n = len(c)
            for i in range(n):
                p, q, r = c[(i - 1) % n], c[i], c[(i + 1) % n]
                nxt.append([q, V + edge_id[(min(q, r), max(q, r))], fp + j, V + edge_id[(min(p, q), max(p, q))]])
        faces = nxt
        V_below = V
        V += E + F
    # the last level: the sectors of every vertex, then the quads by record
    records = [None] * V
    sector_of = {}                                                       # (v, a) for the quad (v, a, .., b) -> record
    for v, (kind, ring, _) in enumerate(rings):
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
            records[v] = (v, kind, list(ring))
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
    tris = []
    for q in faces:
        r = [sector_of[(q[i], q[(i + 1) % 4])] for i in range(4)]
        tris += [(r[0], r[1], r[2]), (r[0], r[2], r[3])]
    return dict(counts=np.array(counts, np.int64).reshape(levels + 1, 3), first_corner=first, rules=rules,
                rings=[(k, list(r)) for k, r, _ in rings], records=records, quads1=np.array(quads1, np.int64).reshape(-1, 2),
                faces=np.array(tris, np.int64).reshape(-1, 3), quads=np.array(faces, np.int64).reshape(-1, 4), polygons=cage(rec, polys)[0])


# ---------------------------------------------------------------- values
def face_point(P, rule):
    ids = rule[2]
    s = P[ids[0]] + P[ids[1]]
    for c in ids[2:]:
        s = s + P[c]
    return s / float(len(ids))


def refine(P, rules):
    '''positions [V_l+1,3] f64 of the next level from P [V_l,3] f64'''
    out = np.empty((len(rules), 3), np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for i, (kind, variant, ids, par) in enumerate(rules):
            blend = variant & 3
            if variant & CC and kind == EDGE_BND:
                out[i] = face_point(P, rules[i])
            elif variant & CC and kind == EDGE_INT:
                a, b, f1, f2 = ids
                E = 0.25 * ((P[a] + P[b]) + (face_point(P, rules[f1]) + face_point(P, rules[f2])))
                out[i] = E if blend == PLAIN else ((1.0 - par) * E) + (par * (0.5 * (P[a] + P[b])))
            elif variant & CC:
                n = (len(ids) - (2 if blend == BLEND_CREASE else 0)) // 2
                ring, rfaces = ids[:n], ids[n:2 * n]
                sr, sf = P[ring[0]], face_point(P, rules[rfaces[0]])
                for r in ring[1:]:
                    sr = sr + P[r]
                for f in rfaces[1:]:
                    sf = sf + face_point(P, rules[f])
                nd = float(n)
                M = (((nd - 2.0) / nd) * P[i]) + ((1.0 / (nd * nd)) * (sr + sf))
                if blend == BLEND_CREASE:
                    C = 0.75 * P[i] + 0.125 * (P[ids[-2]] + P[ids[-1]])
                    M = ((1.0 - par) * M) + (par * C)
                elif blend == BLEND_CORNER:
                    M = ((1.0 - par) * M) + (par * P[i])
                out[i] = M
            elif kind == EDGE_BND:
                out[i] = 0.5 * (P[ids[0]] + P[ids[1]])
            elif kind == VERT_BND:
                out[i] = 0.75 * P[i] + 0.125 * (P[ids[0]] + P[ids[-1]])
            else:
                assert kind == VERT_INT and variant == FIXED
                out[i] = P[i]
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


def positions(rec, topo, control=None):
    '''the f64 positions of every level 0..L: a list of [V_l,3]'''
    src = np.asarray(rec if control is None else control)
    P = [src[topo['first_corner'], :3].astype(np.float64)]
    for l in sorted(topo['rules']):
        P.append(refine(P[-1], topo['rules'][l]))
    return P


def split_uv(c):
    '''the uvs [n,2] of a face's corners -> those of its n quads, [n,4,2]'''
    n = len(c)
    s = c[0] + c[1]
    for u in c[2:]:
        s = s + u
    f = s / float(n)
    return [np.stack([c[i], 0.5 * (c[i] + c[(i + 1) % n]), f, 0.5 * (c[(i - 1) % n] + c[i])]) for i in range(n)]


def face_uvs(src, topo):
    '''[2 Q_L,3,2] f64: the face-varying uvs of the emitted triangles'''
    levels = topo['counts'].shape[0] - 1
    uv = np.asarray(src)[:, 6:8].astype(np.float64)
    quads, tri = [], 0
    for c in topo['polygons']:
        n = len(c)
        corner = [uv[3 * tri], uv[3 * tri + 1]] + [uv[3 * (tri + i) + 2] for i in range(n - 2)]
        quads += split_uv(corner)
        tri += n - 2
    for l in range(1, levels):
        quads = [k for q in quads for k in split_uv(list(q))]
    out = []
    for q in quads:
        out += [np.stack([q[0], q[1], q[2]]), np.stack([q[0], q[2], q[3]])]
    return np.array(out, np.float64).reshape(-1, 3, 2)


def records_of(rec, topo, P_last, control=None):
    '''the subdivided copy [3 F, 8] f32 from the last level's (perhaps displaced) positions'''
    src = np.asarray(rec if control is None else control)
    N = normals(P_last, topo['records'])
    uv = face_uvs(src, topo)
    ids = topo['faces'].reshape(-1)
    vert = np.array([r[0] for r in topo['records']], np.int64)
    out = np.concatenate([P_last[vert[ids]], N[ids], uv.reshape(-1, 2)], axis=1).astype(np.float32)
    return np.ascontiguousarray(out)


def subdivide(rec, levels, polys=None, creases=None, corners=None, topo=None, control=None):
    '''the subdivided copy [3 * 2 (sum n_j) 4^(levels - 1), 8] f32 of the mesh records rec [3k,8] f32 (`control`: the records the
    positions and uvs are read from, an object's deformed copy, where the topology is rec's)'''
    rec = np.asarray(rec)
    assert rec.dtype == np.float32 and rec.ndim == 2 and rec.shape[1] == 8
    topo = topology(rec, levels, polys, creases, corners) if topo is None else topo
    return records_of(rec, topo, positions(rec, topo, control)[-1], control)


# ---------------------------------------------------------------- fixtures
def fan_records(verts, polygons, seam=3):
    '''(records [3k,8] f32, polys [m] int32) of an indexed polygon mesh, fan by fan: unit-z normals (not used) and texcoords from the x
    and y of the position, shifted on every `seam`-th polygon, so that the edges of those polygons are uv seams'''
    verts = np.asarray(verts, np.float32)
    out = []
    for j, c in enumerate(polygons):
        p = verts[list(c)]
        t = (0.25 * p[:, :2] + 0.5).astype(np.float32)
        if j % seam == 0:
            t += np.float32([0.125, 0.0625])
        corner = np.concatenate([p, np.tile(np.float32([0, 0, 1]), (len(c), 1)), t], axis=1)
        for i in range(len(c) - 2):
            out += [corner[0], corner[i + 1], corner[i + 2]]
    return np.ascontiguousarray(np.array(out, np.float32).reshape(-1, 8)), np.array([len(c) for c in polygons], np.int32)


def cube():
    verts = [(x, y, z) for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)]
    return verts, [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]


def pyramid():
    '''a square pyramid: four triangles about an apex of valence 4, and a quad'''
    verts = [(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0), (0.1, 0, 1.5)]
    return verts, [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4), (3, 2, 1, 0)]


def cap5():
    '''closed: five quads about a vertex of valence 5, five quads below them, and a pentagon'''
    ang = 2 * np.pi * np.arange(5) / 5
    verts = [(0, 0, 1.0)] + [(np.cos(a), np.sin(a), 0.6) for a in ang] + [(1.2 * np.cos(a + 0.6), 1.2 * np.sin(a + 0.6), 0.3) for a in ang] \
        + [(0.9 * np.cos(a + 0.6), 0.9 * np.sin(a + 0.6), -0.5) for a in ang]
    polygons = []
    for i in range(5):
        j = (i + 1) % 5
        polygons.append((0, 1 + i, 6 + i, 1 + j))
        polygons.append((1 + j, 6 + i, 11 + i, 11 + j))
        polygons.append((1 + j, 11 + j, 6 + j))
    polygons.append((15, 14, 13, 12, 11))
    return verts, polygons


def grid(nx=5, ny=5, bump=0.15):
    verts = [(x - nx / 2, y - ny / 2, bump * np.sin(1.3 * x + 0.7 * y)) for y in range(ny + 1) for x in range(nx + 1)]
    polygons = []
    for y in range(ny):
        for x in range(nx):
            a = y * (nx + 1) + x
            polygons.append((a, a + 1, a + nx + 2, a + nx + 1))
    return verts, polygons


def cylinder(n=8, rings=3):
    verts = [(np.cos(2 * np.pi * i / n), np.sin(2 * np.pi * i / n), 0.7 * r) for r in range(rings) for i in range(n)]
    polygons = []
    for r in range(rings - 1):
        for i in range(n):
            a, b = r * n + i, r * n + (i + 1) % n
            polygons.append((a, b, b + n, a + n))
    return verts, polygons


def indexed(name):
    if name == 'quad':
        return [(0, 0, 0), (1, 0, 0.25), (1, 1, 0), (-0.0, 1, 0.5)], [(0, 1, 2, 3)]
    if name == 'triangle':
        return [(0, 0, 0), (1, 0, 0.25), (0.25, 1, 0)], [(0, 1, 2)]
    if name == 'pentagon':
        return [(np.cos(a), np.sin(a), 0.1 * np.cos(2 * a)) for a in 2 * np.pi * np.arange(5) / 5], [(0, 1, 2, 3, 4)]
    return dict(cube=cube, pyramid=pyramid, cap5=cap5, grid=grid, cylinder=cylinder)[name]()


def edge_creases(polygons, pairs):
    '''flat [sum n_j] f32: the sharpness of {(p, q): s} on the polygon edges that run between indexed vertices p and q (either
    direction)'''
    out = []
    for c in polygons:
        for i in range(len(c)):
            p, q = c[i], c[(i + 1) % len(c)]
            out.append(pairs.get((p, q), pairs.get((q, p), 0.0)))
    return np.array(out, np.float32)


NAMES = ('quad', 'triangle', 'pentagon', 'cube', 'pyramid', 'cap5', 'grid', 'cylinder')
CREASED = ('cube_inf', 'cube_1p5', 'grid_line', 'grid_corners', 'cube_two')


@functools.lru_cache(maxsize=None)
def fixture(name):
    '''(records [3k,8] f32, polys [m] int32, creases [sum n_j] f32 or None, corners [sum n_j] bool or None), read-only'''
    creases = corners = None
    if name in NAMES:
        verts, polygons = indexed(name)
    elif name in ('cube_inf', 'cube_1p5'):
        verts, polygons = cube()
        s = INF if name == 'cube_inf' else 1.5
        creases = np.full(24, s, np.float32)
    elif name == 'cube_two':                                              # the two faces on an edge state 0.25 and 2: the edge has 2
        verts, polygons = cube()
        creases = edge_creases(polygons, {(0, 2): 2.0, (2, 3): 2.0, (3, 1): 2.0, (1, 0): 2.0})
        creases[0] = 0.25                                                 # (edge 0 -> 2 as polygon 0 states it; polygon 4 states 2)
    elif name in ('grid_line', 'grid_corners'):                           # a crease line x = 2 from boundary to boundary
        verts, polygons = grid()
        creases = edge_creases(polygons, {(y * 6 + 2, (y + 1) * 6 + 2): INF for y in range(5)})
        if name == 'grid_corners':
            corners = np.array([v in (0, 5, 30, 35) for c in polygons for v in c], bool)
            corners.setflags(write=False)
    else:
        raise KeyError(name)
    rec, polys = fan_records(verts, polygons)
    for a in (rec, polys, creases):
        if a is not None:
            a.setflags(write=False)
    return rec, polys, creases, corners


@functools.lru_cache(maxsize=None)
def fixture_topology(name, levels):
    rec, polys, creases, corners = fixture(name)
    return topology(rec, levels, polys, creases, corners)


@functools.lru_cache(maxsize=None)
def fixture_positions(name, levels):
    return positions(fixture(name)[0], fixture_topology(name, levels))


@functools.lru_cache(maxsize=None)
def fixture_subdivided(name, levels):
    out = records_of(fixture(name)[0], fixture_topology(name, levels), fixture_positions(name, levels)[-1])
    out.setflags(write=False)
    return out

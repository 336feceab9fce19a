// subdiv_rule.h -- the pure piece of subdivision's host side (scene_subdiv.cpp; DESIGN.md sections 3.19 to 3.19.2): the topology of a
// cage and of its refinements, the tables subdiv.hip gathers through (the run tables of its launches are run_table.h's).  Plain
// C++17 with nothing of HIP and no context (as deform_rule.h), so that a stand-alone program can run it under a sanitizer
// (tools/subdiv_rule_check.cpp).  Two schemes: Loop over a mesh's triangles (mpt_subdiv_topology and, with creases and corners,
// mpt_subdiv_topology_creased in the C ABI) and Catmull-Clark over a cage of polygons (mpt_subdiv_topology_cc).  The definitions
// they follow are stated in include/miptina.h and at the top of subdiv.hip.
//
// Both schemes build every level from corner lists with ONE builder (build_level: a triangle is a polygon of 3 corners), decide
// every vertex and edge by ONE set of crease rules (decide_vertex, decide_edge) and write rules with one writer (Rules, put_vertices,
// put_edges).  What a scheme states for itself: which ids its smooth vertex rule and its interior edge rule read beside the
// neighbours and the endpoints, its face points, how a face splits, and the tail of the block.
//
// THE BLOCK.  The topology function hands back per level 0..levels the counts, and one block of 32-bit words, the layout the
// device reads (offsets in words from the block's start):
//   [0, V_0)                      first corner of every control vertex
//   rule_at[l], l = 1..levels     the rules (two words each) of the vertices of level l, then their ids
//   nrule_at                      V_L rules of the rings of the last level (for the normals), then the rings
//   srule_at                      (a creased mesh) R rules of the last level's RECORDS, then R vertex ids, then the rings of the sectors
//   quad_at                       (Catmull-Clark) the table of level-1 quads
//   face_at                       the last level's triangles, [.][3] record ids
// A rule is { kind | n << 2 | variant << 28, ring }: `ring` is the offset of its ids, vertex ids of the level below (nrule, srule:
// of the last level).  The ids of a launch's rules lie behind its rules in the rules' order.  Variant 0, the plain rules:
//   MPT_SUBDIV_VERT_INT   the n neighbours of an interior vertex in winding order, from the lowest id
//   MPT_SUBDIV_VERT_BND   the n neighbours of a boundary vertex, from the boundary neighbour that begins the fan to the one that ends it
//   MPT_SUBDIV_EDGE_INT   a b c d of an interior edge          MPT_SUBDIV_EDGE_BND   a b of a boundary edge
// A CREASED mesh (a sharpness above zero or a flagged corner; section 3.19.1) has beside them
//   MPT_SUBDIV_VERT_INT | MPT_SUBDIV_BLEND_CREASE   the n neighbours, then p q, the far ends of the vertex's two sharp edges, then the
//                                                   f64 f (low word first):  ((1 - f) * M) + (f * C)
//   MPT_SUBDIV_VERT_INT | MPT_SUBDIV_BLEND_CORNER   the n neighbours, then the f64 f:  ((1 - f) * M) + (f * v)
//   MPT_SUBDIV_VERT_INT | MPT_SUBDIV_FIXED          n = 0: the vertex stays (a flagged corner; three or more sharp edges with f >= 1)
//   MPT_SUBDIV_EDGE_INT | MPT_SUBDIV_BLEND_EDGE     a b c d, then the f64 s:  ((1 - s) * E) + (s * H)
// A vertex of two sharp edges with f >= 1 is a plain MPT_SUBDIV_VERT_BND of n = 2, p q; an interior edge with s >= 1 a plain
// MPT_SUBDIV_EDGE_BND: the crease rules are the boundary's.
// The hard edges of the last level cut a vertex's fan into sectors.  Record v < V_L is vertex v's first sector (from the ring's
// start), or its whole ring where no interior edge of it is hard -- then its rule is the nrule's, ring and all; a further sector is
// a record from V_L on, in the order of the vertices and then of the ring.  A sector's rule is a MPT_SUBDIV_VERT_BND of the
// neighbours from its first hard edge to its last (an interior vertex with one hard edge: n + 1 of them, the first again at the
// end).  The whole rings at nrule_at stay: the displacement's direction is taken of them.  An uncreased mesh has nrec = V_L,
// srule_at = 0, no records in the block and a face table of vertex ids.
//
// LOOP.  The mesh verts [3k][8] (pos3 nrm3 uv2, f32; only the positions are read); crease [k][3] (edge j of face f runs from corner
// j to corner (j + 1) % 3; null: all zero) and the corner flags corner [k][3] (null: none).  Vertex ids of level l + 1: the V_l even
// vertices, then the E_l edge points; rule_at[l + 1] has V_l + E_l rules.  c d of an interior edge are the opposite corners of the
// face that runs a -> b and of the other.  Face (v0, v1, v2) becomes (v0, e01, e20), (v1, e12, e01), (v2, e20, e12), (e01, e12,
// e20); face_at is [F_L][3]; quad_at is 0.
//
// CATMULL-CLARK (section 3.19.2).  The mesh holds polygon j, of polys[j] corners, as polys[j] - 2 consecutive triangles, a fan about
// its first corner: triangle i is (c_0, c_i+1, c_i+2) (polys null: every triangle is a polygon).  crease and corner are flat [sum
// polys]: entry i of polygon j is the edge from its corner i to corner (i + 1) % n, respectively its corner i.  Level 0 has the
// polygons for faces, every later level quads: polygon or quad j of corners c_0 .. c_n-1 becomes the quads (c_i, e(c_i, c_i+1),
// f_j, e(c_i-1, c_i)), at level 1 from the sum of the n before it, later 4 j + i.  Vertex ids of level l + 1: V_l even vertices,
// then the E_l edge points, then the F_l face points; rule_at[l + 1] has V_l + E_l + F_l rules, the vertices, the edges, then the
// FACES.  A boundary vertex, a boundary edge (and an edge of sharpness >= 1), a vertex that stays and the rings and sectors of the
// last level have the heads of above.  The rules that are Catmull-Clark's carry MPT_SUBDIV_CC in the variant:
//   MPT_SUBDIV_EDGE_BND | MPT_SUBDIV_CC          a FACE POINT: the n corners of the face in its own order
//   MPT_SUBDIV_EDGE_INT | MPT_SUBDIV_CC          n = 4: a b, then the ids at level l + 1 of the face points of the face that runs a -> b
//                                                and of the other (a face point's rule is rule `id` of the same launch: the lane
//                                                evaluates it again);  | MPT_SUBDIV_BLEND_EDGE: then the f64 s
//   MPT_SUBDIV_VERT_INT | MPT_SUBDIV_CC          the n neighbours, then n face point ids, the i-th the face between r_i and r_i+1;
//                                                | MPT_SUBDIV_BLEND_CREASE: then p q and the f64 f;  | MPT_SUBDIV_BLEND_CORNER: then the f64 f
//   quad_at                       [Q_1][2] per quad of level 1: the first triangle of its polygon in the mesh, n | i << 8
//   face_at                       [2 Q_L][3]: quad q = (v0, v1, v2, v3) of the last level is faces 2q (v0, v1, v2), 2q + 1 (v0, v2, v3)
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <unordered_map>
#include <vector>
#include "mpt_types.h"          // MPT_SUBDIV_* (plain structures and constants)

enum MptSubdivVerdict {
    MPT_SUBDIV_OK = 0, MPT_SUBDIV_ARGS, MPT_SUBDIV_LEVELS, MPT_SUBDIV_TOO_MANY, MPT_SUBDIV_NOT_FINITE, MPT_SUBDIV_DEGENERATE,
    MPT_SUBDIV_EDGE_FACES, MPT_SUBDIV_EDGE_DIRECTION, MPT_SUBDIV_FAN, MPT_SUBDIV_CREASE,
    MPT_SUBDIV_POLYS                            // (Catmull-Clark: polygons that are not the mesh's triangles, or not fans)
};

// The block's header: what a reader needs beside the words (a mesh's row keeps it: mpt_ctx::MptSubdivMesh)
struct MptSubdivHead {
    int levels = 0;
    int64_t nv[MPT_SUBDIV_MAX_LEVELS + 1] = {}, ne[MPT_SUBDIV_MAX_LEVELS + 1] = {}, nf[MPT_SUBDIV_MAX_LEVELS + 1] = {}, nrec = 0;
    int32_t rule_at[MPT_SUBDIV_MAX_LEVELS + 1] = {}, nrule_at = 0, face_at = 0, srule_at = 0;
    int32_t quad_at = 0; int64_t nquads1 = 0;   // (Catmull-Clark; 0 of a Loop mesh)
};
struct MptSubdivTopo : MptSubdivHead { std::vector<int32_t> words; };
using MptSubdivTopoCC = MptSubdivTopo;

namespace mpt_subdiv_detail {

struct Say {
    char *why; size_t size;
    MptSubdivVerdict operator()(MptSubdivVerdict v, const char *fmt, long long a = 0, long long b = 0, long long c = 0) const {
        if (why && size) snprintf(why, size, fmt, a, b, c);
        return v;
    }
};

// faces as corner lists: face f's corners are face[at[f]] .. face[at[f + 1] - 1].  F faces of n corners each:
inline std::vector<int32_t> corners_at(int64_t F, int32_t n) {
    std::vector<int32_t> at((size_t)F + 1);
    for (int64_t f = 0; f <= F; f++) at[(size_t)f] = (int32_t)(n * f);
    return at;
}

struct Level {                                  // one level's edges and rings, from its faces alone
    std::vector<int32_t> edge;                  // [E][4]: a b h1 h2 -- the corner slots the half-edges on it start from: h1 of the face that runs a -> b, h2 of the other; a boundary edge: h1 of its face, h2 -1
    std::vector<int32_t> face_edge;             // per corner slot: the edge of corners j -> j + 1
    std::vector<int32_t> slot_face;             // per corner slot: its face
    std::vector<int32_t> ring_kind, ring_n, ring_at, ring, ring_face;   // ring_face: beside ring, the face between r_i and r_i+1 (-1 behind a boundary ring's last)
};

struct HalfEdge {                               // ends: lo << 32 | hi
    uint64_t ends; int32_t slot, fwd;
    int32_t lo() const { return (int32_t)(ends >> 32); }
    int32_t hi() const { return (int32_t)(ends & 0xffffffffu); }
};

inline MptSubdivVerdict build_level(const std::vector<int32_t> &at, const std::vector<int32_t> &face, int64_t V, Level &out, const Say &say) {
    const int64_t F = (int64_t)at.size() - 1, S = (int64_t)face.size();
    std::vector<HalfEdge> he((size_t)S);
    out.slot_face.resize((size_t)S);
    for (int64_t f = 0; f < F; f++) {
        const int32_t a0 = at[(size_t)f], n = at[(size_t)f + 1] - a0;
        for (int32_t j = 0; j < n; j++) {
            const int32_t p = face[(size_t)(a0 + j)], q = face[(size_t)(a0 + (j + 1 == n ? 0 : j + 1))];
            he[(size_t)(a0 + j)] = { (uint64_t)std::min(p, q) << 32 | (uint64_t)std::max(p, q), a0 + j, p < q ? 1 : 0 };
            out.slot_face[(size_t)(a0 + j)] = (int32_t)f;
        }
    }
    std::sort(he.begin(), he.end(), [](const HalfEdge &x, const HalfEdge &y) {        // (by slot: by face, then by corner)
        return x.ends != y.ends ? x.ends < y.ends : x.slot < y.slot;
    });
    const auto face_of = [&](const HalfEdge &h) { return (long long)out.slot_face[(size_t)h.slot]; };
    out.edge.clear(); out.face_edge.assign((size_t)S, -1);
    for (size_t i = 0; i < he.size();) {
        size_t j = i + 1;
        while (j < he.size() && he[j].ends == he[i].ends) j++;
        if (j - i > 2) return say(MPT_SUBDIV_EDGE_FACES, "subdivision: face %lld is the third on the edge of vertices %lld and %lld", face_of(he[i + 2]), he[i].lo(), he[i].hi());
        if (j - i == 2 && he[i].fwd == he[i + 1].fwd)
            return say(MPT_SUBDIV_EDGE_DIRECTION, "subdivision: faces %lld and %lld run their shared edge in the same direction (vertex %lld first)", face_of(he[i]),
                       face_of(he[i + 1]), he[i].fwd ? he[i].lo() : he[i].hi());
        const int32_t e = (int32_t)(out.edge.size() / 4);
        int32_t h1 = -1, h2 = -1;
        for (size_t h = i; h < j; h++) {
            if (j - i == 1 || he[h].fwd) h1 = he[h].slot; else h2 = he[h].slot;
            out.face_edge[(size_t)he[h].slot] = e;
        }
        out.edge.insert(out.edge.end(), { he[i].lo(), he[i].hi(), h1, h2 });
        i = j;
    }
    // the corner slots of every vertex (counting sort), then its ring of edge neighbours
    std::vector<int64_t> first((size_t)V + 1, 0);
    for (int32_t v : face) first[(size_t)v + 1]++;
    for (int64_t v = 0; v < V; v++) first[(size_t)v + 1] += first[(size_t)v];
    std::vector<int32_t> slot((size_t)S);
    {
        std::vector<int64_t> put(first.begin(), first.end() - 1);
        for (int64_t s = 0; s < S; s++) slot[(size_t)put[(size_t)face[(size_t)s]]++] = (int32_t)s;
    }
    out.ring_kind.assign((size_t)V, 0); out.ring_n.assign((size_t)V, 0); out.ring_at.assign((size_t)V, 0); out.ring.clear(); out.ring_face.clear();
    out.ring.reserve((size_t)(S + V)); out.ring_face.reserve((size_t)(S + V));    // (a ring entry per corner slot, one more of a boundary vertex)
    std::vector<int32_t> src, dst, fc; std::vector<char> used;
    for (int64_t v = 0; v < V; v++) {
        const int64_t n = first[(size_t)v + 1] - first[(size_t)v];
        src.resize((size_t)n); dst.resize((size_t)n); fc.resize((size_t)n); used.assign((size_t)n, 0);
        for (int64_t i = 0; i < n; i++) {               // in face (v, a, ..., b), a comes before b
            const int32_t s = slot[(size_t)(first[(size_t)v] + i)], f = out.slot_face[(size_t)s], a0 = at[(size_t)f], m = at[(size_t)f + 1] - a0, j = s - a0;
            src[(size_t)i] = face[(size_t)(a0 + (j + 1 == m ? 0 : j + 1))]; dst[(size_t)i] = face[(size_t)(a0 + (j ? j - 1 : m - 1))]; fc[(size_t)i] = f;
        }
        if (n == 0) return say(MPT_SUBDIV_ARGS, "subdivision: vertex %lld has no face", v);
        int32_t start = -1, starts = 0, lowest = src[0];
        for (int64_t i = 0; i < n; i++) {
            lowest = std::min(lowest, src[(size_t)i]);
            bool entered = false;
            for (int64_t k = 0; k < n && !entered; k++) entered = dst[(size_t)k] == src[(size_t)i];
            if (!entered) { start = src[(size_t)i]; starts++; }
        }
        const char *fan = "subdivision: the %lld faces of vertex %lld are not one fan (a bow-tie)";
        if (starts > 1) return say(MPT_SUBDIV_FAN, fan, n, v);
        const bool boundary = starts == 1;
        int32_t cur = boundary ? start : lowest;
        out.ring_at[(size_t)v] = (int32_t)out.ring.size();
        out.ring.push_back(cur);
        for (int64_t step = 0; step < n; step++) {
            int64_t hit = -1;
            for (int64_t i = 0; i < n && hit < 0; i++)
                if (!used[(size_t)i] && src[(size_t)i] == cur) hit = i;
            if (hit < 0) return say(MPT_SUBDIV_FAN, fan, n, v);
            used[(size_t)hit] = 1; cur = dst[(size_t)hit];
            out.ring_face.push_back(fc[(size_t)hit]);
            out.ring.push_back(cur);
        }
        if (!boundary) {
            if (cur != lowest) return say(MPT_SUBDIV_FAN, fan, n, v);
            out.ring.pop_back();
        } else out.ring_face.push_back(-1);
        out.ring_kind[(size_t)v] = boundary ? MPT_SUBDIV_VERT_BND : MPT_SUBDIV_VERT_INT;
        out.ring_n[(size_t)v] = (int32_t)(boundary ? n + 1 : n);
    }
    return MPT_SUBDIV_OK;
}

// the edge of vertices p and q of a level (its edges are sorted by (lower id, higher id))
inline int64_t edge_of(const Level &lv, int32_t p, int32_t q) {
    const int32_t lo = std::min(p, q), hi = std::max(p, q);
    int64_t a = 0, b = (int64_t)lv.edge.size() / 4;
    while (a < b) {
        const int64_t m = (a + b) / 2;
        const int32_t *e = &lv.edge[(size_t)m * 4];
        if (e[0] < lo || (e[0] == lo && e[1] < hi)) a = m + 1; else b = m;
    }
    return a;
}

struct KeyHash {
    size_t operator()(const uint64_t &k) const { return (size_t)(k * 0x9E3779B97F4A7C15ull >> 17); }
};

// control vertices: corners whose positions are equal as values (-0 is +0), numbered by first appearance in corner order.  corner [3k]:
// the vertex of every corner; first_corner [V]: the first corner of every vertex
inline MptSubdivVerdict weld(const float *verts, int k, std::vector<int32_t> &corner, std::vector<int32_t> &first_corner, const Say &say) {
    struct Key { uint32_t x, y, z; bool operator==(const Key &o) const { return x == o.x && y == o.y && z == o.z; } };
    struct Hash { size_t operator()(const Key &q) const { return KeyHash()(((uint64_t)q.x << 32 | q.y) ^ (uint64_t)q.z * 0xD6E8FEB86659FD93ull); } };
    std::unordered_map<Key, int32_t, Hash> ids;
    ids.reserve((size_t)k * 2);
    corner.assign((size_t)k * 3, 0); first_corner.clear();
    for (int64_t s = 0; s < (int64_t)k * 3; s++) {
        Key key;
        uint32_t *w[3] = { &key.x, &key.y, &key.z };
        for (int a = 0; a < 3; a++) {
            const float p = verts[(size_t)s * 8 + (size_t)a];
            if (!std::isfinite(p)) return say(MPT_SUBDIV_NOT_FINITE, "subdivision: the position of corner %lld of face %lld is not finite", s % 3, s / 3);
            const float q = p == 0.0f ? 0.0f : p;
            memcpy(w[a], &q, 4);
        }
        auto it = ids.find(key);
        if (it == ids.end()) { it = ids.emplace(key, (int32_t)first_corner.size()).first; first_corner.push_back((int32_t)s); }
        corner[(size_t)s] = it->second;
    }
    return MPT_SUBDIV_OK;
}

// ---------------------------------------------------------------- the steps both schemes take
inline MptSubdivVerdict check_args(const float *verts, int k, int levels, const Say &say) {
    if (say.why && say.size) say.why[0] = 0;
    if (k < 0 || (k > 0 && !verts)) return say(MPT_SUBDIV_ARGS, "subdivision: verts must hold [%lld][8] values", 3LL * k);
    if (levels < 1 || levels > MPT_SUBDIV_MAX_LEVELS) return say(MPT_SUBDIV_LEVELS, "subdivision: levels %lld outside [1, %lld]", levels, MPT_SUBDIV_MAX_LEVELS);
    return MPT_SUBDIV_OK;
}

inline MptSubdivVerdict check_faces(long long last_faces, int levels, const Say &say) {      // the triangles of the last level
    if (last_faces > MPT_SUBDIV_MAX_FACES) return say(MPT_SUBDIV_TOO_MANY, "subdivision: too many faces: %lld at level %lld, at most %lld", last_faces, levels, MPT_SUBDIV_MAX_FACES);
    return MPT_SUBDIV_OK;
}

// crease and corner, one entry per corner slot of the cage's faces (either null).  A refusal names the `unit` ("face", "polygon")
// and the entry in it.  creased: a sharpness is above zero or a corner is flagged
inline MptSubdivVerdict check_creases(const float *crease, const uint8_t *corner, const std::vector<int32_t> &at, const char *unit, bool &creased, const Say &say) {
    const int64_t S = at.back();
    creased = false;
    for (int64_t s = 0; crease && s < S; s++) {
        const float x = crease[(size_t)s];
        if (std::isnan(x) || x < 0.0f) {
            const int64_t f = (int64_t)(std::upper_bound(at.begin(), at.end(), (int32_t)s) - at.begin()) - 1;
            char fmt[96];
            snprintf(fmt, sizeof fmt, "subdivision: the crease of edge %%lld of %s %%lld is %s", unit, std::isnan(x) ? "not a number" : "negative");
            return say(MPT_SUBDIV_CREASE, fmt, s - at[(size_t)f], f);
        }
        creased = creased || x > 0.0f;
    }
    for (int64_t s = 0; corner && s < S; s++) creased = creased || corner[(size_t)s] != 0;
    return MPT_SUBDIV_OK;
}

// a control vertex is a corner if any of its welded corners is flagged; the flags pass to even vertices only (their ids stay)
inline std::vector<char> flags_of(const uint8_t *corner, const std::vector<int32_t> &face, int64_t V) {
    std::vector<char> flagged((size_t)V, 0);
    for (size_t s = 0; corner && s < face.size(); s++)
        if (corner[s]) flagged[(size_t)face[s]] = 1;
    return flagged;
}

// The sharpness of a level's edges.  cage: per edge the CAGE sharpness it inherits (0: an edge new inside a face)
struct Sharpness {
    const Level *lv = nullptr;
    int l = 0;
    std::vector<double> cage, below;
    // level l's edges, once its Level is built; V_below: the vertices of level l - 1
    void inherit(const Level &level, int at_level, const float *crease, bool creased, int64_t V_below) {
        lv = &level; l = at_level;
        const int64_t E = (int64_t)level.edge.size() / 4;
        below.swap(cage);
        cage.assign((size_t)E, 0.0);
        if (l == 0) {                           // the two faces on an edge may state different values: the edge takes the larger
            for (size_t s = 0; crease && s < level.face_edge.size(); s++) {
                double &c = cage[(size_t)level.face_edge[s]];
                c = std::max(c, (double)crease[s]);
            }
        } else if (creased) {                   // both halves of a split edge inherit (an even vertex's edges all end in edge points); the others are new
            for (int64_t e = 0; e < E; e++) {
                const int32_t lo = level.edge[(size_t)e * 4], hi = level.edge[(size_t)e * 4 + 1];
                if (lo < V_below) cage[(size_t)e] = below[(size_t)(hi - V_below)];
            }
        }
    }
    // the sharpness of edge e at this level: s0 - l where that is positive, else 0; a boundary edge counts as inf
    double operator()(int64_t e) const {
        if (lv->edge[(size_t)e * 4 + 3] < 0) return std::numeric_limits<double>::infinity();
        const double s = cage[(size_t)e] - (double)l;
        return s > 0.0 ? s : 0.0;
    }
};

// The rules of one launch.  A rule's ids (and the f64 parameter some variants end with, low word first) are collected in `ids`
// and appended by put, in the rules' order
struct Rules {
    std::vector<int32_t> &W;
    size_t at = 0;
    std::vector<int32_t> ids;
    explicit Rules(std::vector<int32_t> &words) : W(words) {}
    void begin(MptSubdivHead &out, int l, int64_t n) {          // n rules: of level l + 1's vertices, or (the last level) of its rings
        at = W.size();
        (l == out.levels ? out.nrule_at : out.rule_at[l + 1]) = (int32_t)at;
        W.resize(at + (size_t)n * 2);
    }
    void put(int64_t i, int kind, int variant, int64_t n) {
        W[at + (size_t)i * 2] = (int32_t)(kind | n << 2 | variant << MPT_SUBDIV_VARIANT_SHIFT);
        W[at + (size_t)i * 2 + 1] = (int32_t)W.size();
        W.insert(W.end(), ids.begin(), ids.end());
    }
    void push_f64(double x) { int32_t w[2]; memcpy(w, &x, 8); ids.push_back(w[0]); ids.push_back(w[1]); }
};

// What the crease rules decide of a vertex: it stays; its scheme's smooth rule; the crease rule of p q; a blend of the smooth rule
// with the crease rule of p q, or with the vertex itself, by f
struct VertexRule {
    enum What { SMOOTH, STAY, CREASE, BLEND_CREASE, BLEND_CORNER } what = SMOOTH;
    int32_t p = 0, q = 0;
    double f = 0.0;
};
struct Spoke { double s; int32_t far; };         // a sharp edge of a vertex: its sharpness at the level, its far end

inline VertexRule decide_vertex(const Level &lv, int64_t v, bool flagged, const Sharpness &sharp, std::vector<Spoke> &S) {
    if (flagged) return { VertexRule::STAY };
    const int32_t *ring = &lv.ring[(size_t)lv.ring_at[(size_t)v]];
    S.clear();
    for (int64_t i = 0; i < lv.ring_n[(size_t)v]; i++) {
        const double s = sharp(edge_of(lv, (int32_t)v, ring[i]));
        if (s > 0.0) S.push_back({ s, ring[i] });
    }
    const size_t ks = S.size();
    if (ks <= 1 || (ks == 2 && lv.ring_kind[(size_t)v] == MPT_SUBDIV_VERT_BND)) return { VertexRule::SMOOTH };   // (a boundary vertex's two boundary edges: the boundary rule)
    if (ks == 2) {
        const double f = 0.5 * (S[0].s + S[1].s);
        return { f >= 1.0 ? VertexRule::CREASE : VertexRule::BLEND_CREASE, S[0].far, S[1].far, f };
    }
    double f = S[0].s + S[1].s;
    for (size_t i = 2; i < ks; i++) f = f + S[i].s;
    f = f / (double)ks;
    return { f >= 1.0 ? VertexRule::STAY : VertexRule::BLEND_CORNER, 0, 0, f };      // (a blend: an interior vertex -- a boundary vertex's S holds an inf)
}

// The rules of level l's V vertices: rule v of the launch.  The last level's are its plain rings.  more(v, ids), the scheme's
// hook, appends what its smooth rule reads behind the n neighbours and returns the bit its variants carry
template <class More>
inline void put_vertices(Rules &R, const Level &lv, int64_t V, bool last, bool creased, const std::vector<char> &flagged, const Sharpness &sharp, const More &more) {
    std::vector<Spoke> S;
    std::vector<int32_t> &ids = R.ids;
    for (int64_t v = 0; v < V; v++) {
        const int32_t *ring = &lv.ring[(size_t)lv.ring_at[(size_t)v]];
        const int64_t n = lv.ring_n[(size_t)v];
        const int kind = lv.ring_kind[(size_t)v];
        ids.assign(ring, ring + n);
        if (last) { R.put(v, kind, MPT_SUBDIV_PLAIN, n); continue; }
        const VertexRule d = creased ? decide_vertex(lv, v, v < (int64_t)flagged.size() && flagged[(size_t)v], sharp, S) : VertexRule{};
        if (d.what == VertexRule::STAY) { ids.clear(); R.put(v, MPT_SUBDIV_VERT_INT, MPT_SUBDIV_FIXED, 0); continue; }
        if (d.what == VertexRule::CREASE) { ids = { d.p, d.q }; R.put(v, MPT_SUBDIV_VERT_BND, MPT_SUBDIV_PLAIN, 2); continue; }
        const int scheme = more(v, ids);
        if (d.what == VertexRule::SMOOTH) { R.put(v, kind, MPT_SUBDIV_PLAIN | scheme, n); continue; }
        if (d.what == VertexRule::BLEND_CREASE) { ids.push_back(d.p); ids.push_back(d.q); }
        R.push_f64(d.f);
        R.put(v, MPT_SUBDIV_VERT_INT, (d.what == VertexRule::BLEND_CREASE ? MPT_SUBDIV_BLEND_CREASE : MPT_SUBDIV_BLEND_CORNER) | scheme, n);
    }
}

// What the crease rules decide of an edge: half -- its point is 0.5 * (a + b): a boundary edge, and an edge that is sharp at this
// level --, else its scheme's interior rule, blended with the half rule by s where s > 0
struct EdgeRule { bool half; double s; };

inline EdgeRule decide_edge(const Level &lv, int64_t e, bool creased, const Sharpness &sharp) {
    const bool inner = lv.edge[(size_t)e * 4 + 3] >= 0;
    const double s = creased ? sharp(e) : 0.0;
    return { !inner || s >= 1.0, s };
}

// The rules of level l's edges: rules V + e of the launch.  side(h), the scheme's hook, is the id its interior rule reads of the
// half-edge h beside the endpoints; scheme: the bit its variants carry
template <class Side>
inline void put_edges(Rules &R, const Level &lv, int64_t V, bool creased, const Sharpness &sharp, int scheme, const Side &side) {
    const int64_t E = (int64_t)lv.edge.size() / 4;
    for (int64_t e = 0; e < E; e++) {
        const int32_t *ed = &lv.edge[(size_t)e * 4];
        const EdgeRule d = decide_edge(lv, e, creased, sharp);
        if (d.half) { R.ids = { ed[0], ed[1], 0, 0 }; R.put(V + e, MPT_SUBDIV_EDGE_BND, MPT_SUBDIV_PLAIN, 2); continue; }
        R.ids = { ed[0], ed[1], side(ed[2]), side(ed[3]) };
        if (d.s == 0.0) R.put(V + e, MPT_SUBDIV_EDGE_INT, MPT_SUBDIV_PLAIN | scheme, 4);
        else { R.push_f64(d.s); R.put(V + e, MPT_SUBDIV_EDGE_INT, MPT_SUBDIV_BLEND_EDGE | scheme, 4); }
    }
}

// The records of a creased mesh's last level, appended to the block: the hard edges (sharpness > 0 at this level, or a boundary) cut
// a vertex's fan into sectors, each an open ring from one hard edge to the next.  Record v is vertex v's first sector -- its whole
// ring where no interior edge of it is hard -- and the others follow V_L in the vertices' order.  face [F][corners]: the last
// level's faces (Loop's triangles, Catmull-Clark's quads) by vertex on entry, by record on return
inline void append_records(const Level &lv, int64_t V, int corners, const Sharpness &sharp, MptSubdivTopo &out, std::vector<int32_t> &face) {
    std::vector<int32_t> &W = out.words;
    std::vector<int32_t> cut;
    const size_t srules = W.size();
    std::vector<int32_t> sector_of(lv.ring.size(), -1);        // per ring slot i of a vertex: the record of its face (v, r_i, r_i+1)
    std::vector<int32_t> svert, shead, sring;                  // per record: its vertex, its rule's head, its ring's word (-1: appended below)
    std::vector<std::vector<int32_t>> extra;
    svert.resize((size_t)V); shead.resize((size_t)V); sring.resize((size_t)V);
    for (int64_t v = 0; v < V; v++) {
        const size_t at = (size_t)lv.ring_at[(size_t)v];
        const int32_t *ring = &lv.ring[at];
        const int64_t n = lv.ring_n[(size_t)v];
        const bool bnd = lv.ring_kind[(size_t)v] == MPT_SUBDIV_VERT_BND;
        const int64_t nfaces = bnd ? n - 1 : n;
        cut.clear();
        for (int64_t i = bnd ? 1 : 0; i < (bnd ? n - 1 : n); i++)
            if (sharp(edge_of(lv, (int32_t)v, ring[i])) > 0.0) cut.push_back((int32_t)i);
        svert[(size_t)v] = (int32_t)v;
        if (cut.empty()) {
            shead[(size_t)v] = W[(size_t)out.nrule_at + (size_t)v * 2]; sring[(size_t)v] = W[(size_t)out.nrule_at + (size_t)v * 2 + 1];
            for (int64_t i = 0; i < nfaces; i++) sector_of[at + (size_t)i] = (int32_t)v;
            continue;
        }
        if (bnd) { cut.insert(cut.begin(), 0); cut.push_back((int32_t)(n - 1)); }
        const size_t nsectors = bnd ? cut.size() - 1 : cut.size();
        for (size_t j = 0; j < nsectors; j++) {
            const int64_t from = cut[j];
            int64_t span = bnd || j + 1 < cut.size() ? cut[j + 1] - from : cut[0] + n - from;
            std::vector<int32_t> open;
            for (int64_t i = 0; i <= span; i++) open.push_back(ring[(size_t)((from + i) % n)]);
            int32_t rec = (int32_t)v;
            if (j > 0) { rec = (int32_t)svert.size(); svert.push_back((int32_t)v); shead.push_back(0); sring.push_back(0); }
            shead[(size_t)rec] = (int32_t)(MPT_SUBDIV_VERT_BND | (span + 1) << 2);
            sring[(size_t)rec] = -1 - (int32_t)extra.size();
            extra.push_back(std::move(open));
            for (int64_t i = 0; i < span; i++) sector_of[at + (size_t)((from + i) % n)] = rec;
        }
    }
    const size_t R = svert.size();
    out.srule_at = (int32_t)srules; out.nrec = (int64_t)R;
    W.resize(srules + R * 2);
    W.insert(W.end(), svert.begin(), svert.end());
    for (size_t r = 0; r < R; r++) {
        W[srules + r * 2] = shead[r];
        if (sring[r] >= 0) { W[srules + r * 2 + 1] = sring[r]; continue; }
        W[srules + r * 2 + 1] = (int32_t)W.size();
        const std::vector<int32_t> &open = extra[(size_t)(-1 - sring[r])];
        W.insert(W.end(), open.begin(), open.end());
    }
    // the face table of a creased mesh indexes records: corner j of a face is the record of its vertex's sector that holds the face
    std::vector<int32_t> by_record(face.size());
    for (int64_t s = 0; s < (int64_t)face.size(); s++) {
        const int32_t v = face[(size_t)s], a = face[(size_t)(s - s % corners + (s + 1) % corners)];
        const size_t at = (size_t)lv.ring_at[(size_t)v];
        const int64_t n = lv.ring_n[(size_t)v];
        int64_t i = 0;
        while (i < n && lv.ring[at + (size_t)i] != a) i++;
        by_record[(size_t)s] = sector_of[at + (size_t)i];
    }
    face.swap(by_record);
}

// the last level's records: one per vertex, or -- then the face table indexes them -- a creased mesh's sectors
inline void put_records(const Level &lv, int64_t V, int corners, bool creased, const Sharpness &sharp, MptSubdivTopo &out, std::vector<int32_t> &face) {
    out.nrec = V; out.srule_at = 0;
    if (creased) append_records(lv, V, corners, sharp, out, face);
}

}  // namespace mpt_subdiv_detail

// The topology of a mesh and of `levels` Loop refinements of it.  A refusal writes its words, which name the face and the edge or
// the vertex, to `why` (always terminated) and leaves `out` unspecified.
inline MptSubdivVerdict mpt_subdiv_topology_creased_of(const float *verts, int k, int levels, const float *crease, const uint8_t *corner, MptSubdivTopo &out,
                                                       char *why, size_t why_size) {
    using namespace mpt_subdiv_detail;
    const Say say{ why, why_size };
    if (const MptSubdivVerdict v = check_args(verts, k, levels, say)) return v;
    if (const MptSubdivVerdict v = check_faces((long long)k << (2 * levels), levels, say)) return v;
    bool creased = false;
    if (const MptSubdivVerdict v = check_creases(crease, corner, corners_at(k, 3), "face", creased, say)) return v;
    std::vector<int32_t> face, first_corner;
    if (const MptSubdivVerdict v = weld(verts, k, face, first_corner, say)) return v;
    for (int64_t f = 0; f < k; f++) {
        const int32_t *v = &face[(size_t)f * 3];
        if (v[0] == v[1] || v[1] == v[2] || v[2] == v[0]) return say(MPT_SUBDIV_DEGENERATE, "subdivision: face %lld has two corners on one vertex (vertex %lld)", f, v[0] == v[1] || v[0] == v[2] ? v[0] : v[1]);
    }
    out = MptSubdivTopo{};
    out.levels = levels;
    std::vector<int32_t> &W = out.words;
    W.assign(first_corner.begin(), first_corner.end());
    int64_t V = (int64_t)first_corner.size();
    const std::vector<char> flagged = flags_of(corner, face, V);
    Sharpness sharp;
    Rules R(W);
    Level lv;
    for (int l = 0; l <= levels; l++) {
        const int64_t F = (int64_t)face.size() / 3;
        if (const MptSubdivVerdict v = build_level(corners_at(F, 3), face, V, lv, say)) return v;
        const int64_t E = (int64_t)lv.edge.size() / 4;
        out.nv[l] = V; out.ne[l] = E; out.nf[l] = F;
        sharp.inherit(lv, l, crease, creased, l ? out.nv[l - 1] : 0);
        const bool last = l == levels;
        R.begin(out, l, last ? V : V + E);
        put_vertices(R, lv, V, last, creased, flagged, sharp, [](int64_t, std::vector<int32_t> &) { return 0; });
        if (last) { put_records(lv, V, 3, creased, sharp, out, face); break; }
        // c d of an edge: the corners opposite to it in the faces of its half-edges
        put_edges(R, lv, V, creased, sharp, 0, [&](int32_t h) { return face[(size_t)(h - h % 3 + (h + 2) % 3)]; });
        // face f = (v0, v1, v2) becomes (v0, e01, e20), (v1, e12, e01), (v2, e20, e12), (e01, e12, e20)
        std::vector<int32_t> next((size_t)F * 12);
        for (int64_t f = 0; f < F; f++) {
            const int32_t v0 = face[(size_t)f * 3], v1 = face[(size_t)f * 3 + 1], v2 = face[(size_t)f * 3 + 2];
            const int32_t e01 = (int32_t)V + lv.face_edge[(size_t)f * 3], e12 = (int32_t)V + lv.face_edge[(size_t)f * 3 + 1],
                          e20 = (int32_t)V + lv.face_edge[(size_t)f * 3 + 2];
            const int32_t child[12] = { v0, e01, e20, v1, e12, e01, v2, e20, e12, e01, e12, e20 };
            std::copy(child, child + 12, next.begin() + (std::ptrdiff_t)f * 12);
        }
        face.swap(next);
        V += E;
    }
    out.face_at = (int32_t)W.size();
    W.insert(W.end(), face.begin(), face.end());
    return MPT_SUBDIV_OK;
}

// The topology of an uncreased mesh: no sharpness, no corner
inline MptSubdivVerdict mpt_subdiv_topology_of(const float *verts, int k, int levels, MptSubdivTopo &out, char *why, size_t why_size) {
    return mpt_subdiv_topology_creased_of(verts, k, levels, nullptr, nullptr, out, why, why_size);
}

// The topology of a cage of m polygons and of `levels` Catmull-Clark refinements of it.  A refusal writes its words, which name the
// face, the polygon, the edge or the vertex, to `why` (always terminated) and leaves `out` unspecified
inline MptSubdivVerdict mpt_subdiv_topology_cc_of(const float *verts, int k, int levels, const int32_t *polys, int m, const float *crease, const uint8_t *corner,
                                                  MptSubdivTopoCC &out, char *why, size_t why_size) {
    using namespace mpt_subdiv_detail;
    const Say say{ why, why_size };
    if (const MptSubdivVerdict v = check_args(verts, k, levels, say)) return v;
    if (!polys) m = k;
    if (m < 0) return say(MPT_SUBDIV_ARGS, "subdivision: polys must hold [%lld] values", m);
    // the polygons: their corner counts sum to the triangles, each within [3, MPT_SUBDIV_MAX_CORNERS]
    std::vector<int32_t> at((size_t)m + 1, 0), tri0((size_t)m, 0);
    {
        int64_t tris = 0;
        for (int j = 0; j < m; j++) {
            const int32_t n = polys ? polys[j] : 3;
            if (n < 3 || n > MPT_SUBDIV_MAX_CORNERS) return say(MPT_SUBDIV_POLYS, "subdivision: polygon %lld has %lld corners, outside [3, %lld]", j, n, MPT_SUBDIV_MAX_CORNERS);
            tri0[(size_t)j] = (int32_t)std::min<int64_t>(tris, k);
            tris += n - 2;
            at[(size_t)j + 1] = at[(size_t)j] + n;
        }
        if (tris != k) return say(MPT_SUBDIV_POLYS, "subdivision: the polygons hold %lld triangles, the mesh has %lld", tris, k);
    }
    const int64_t S0 = at[(size_t)m];
    if (const MptSubdivVerdict v = check_faces((long long)(2 * S0) << (2 * (levels - 1)), levels, say)) return v;
    bool creased = false;
    if (const MptSubdivVerdict v = check_creases(crease, corner, at, "polygon", creased, say)) return v;
    std::vector<int32_t> tri, first_corner;
    if (const MptSubdivVerdict v = weld(verts, k, tri, first_corner, say)) return v;
    // the polygons' corners off their fans: triangle i of polygon j is (c_0, c_i+1, c_i+2)
    std::vector<int32_t> face((size_t)S0);
    for (int j = 0; j < m; j++) {
        const int32_t n = at[(size_t)j + 1] - at[(size_t)j];
        int32_t *c = &face[(size_t)at[(size_t)j]];
        const int32_t *t = &tri[(size_t)tri0[(size_t)j] * 3];
        c[0] = t[0]; c[1] = t[1];
        for (int32_t i = 0; i < n - 2; i++) {
            if (t[3 * i] != c[0] || t[3 * i + 1] != c[i + 1])
                return say(MPT_SUBDIV_POLYS, "subdivision: face %lld does not continue the fan of polygon %lld (triangle %lld of it)", (long long)tri0[(size_t)j] + i, j, i);
            c[i + 2] = t[3 * i + 2];
        }
        for (int32_t a = 0; a < n; a++)
            for (int32_t b = a + 1; b < n; b++)
                if (c[a] == c[b]) return say(MPT_SUBDIV_DEGENERATE, "subdivision: polygon %lld has two corners on one vertex (vertex %lld)", j, c[a]);
    }
    out = MptSubdivTopoCC{};
    out.levels = levels;
    std::vector<int32_t> &W = out.words;
    W.assign(first_corner.begin(), first_corner.end());
    int64_t V = (int64_t)first_corner.size();
    const std::vector<char> flagged = flags_of(corner, face, V);
    Sharpness sharp;
    Rules R(W);
    std::vector<int32_t> quads1;
    Level lv;
    for (int l = 0; l <= levels; l++) {
        if (const MptSubdivVerdict v = build_level(at, face, V, lv, say)) return v;
        const int64_t E = (int64_t)lv.edge.size() / 4, F = (int64_t)at.size() - 1, S = (int64_t)face.size();
        out.nv[l] = V; out.ne[l] = E; out.nf[l] = F;
        sharp.inherit(lv, l, crease, creased, l ? out.nv[l - 1] : 0);
        const bool last = l == levels;
        R.begin(out, l, last ? V : V + E + F);
        const int32_t fp0 = (int32_t)(V + E);       // the id at level l + 1 of face 0's point
        // an interior vertex reads the points of the faces about it (a boundary vertex's rule reads p and q alone: Loop's words)
        put_vertices(R, lv, V, last, creased, flagged, sharp, [&](int64_t v, std::vector<int32_t> &ids) {
            if (lv.ring_kind[(size_t)v] == MPT_SUBDIV_VERT_BND) return 0;
            const int32_t *rf = &lv.ring_face[(size_t)lv.ring_at[(size_t)v]];
            for (int64_t i = 0, n = lv.ring_n[(size_t)v]; i < n; i++) ids.push_back(fp0 + rf[i]);
            return MPT_SUBDIV_CC;
        });
        if (last) {
            put_records(lv, V, 4, creased, sharp, out, face);
            out.quad_at = (int32_t)W.size(); out.nquads1 = (int64_t)quads1.size() / 2;
            W.insert(W.end(), quads1.begin(), quads1.end());
            out.face_at = (int32_t)W.size();
            for (int64_t q = 0; q < F; q++) {          // a quad (by record, if creased) is emitted as (0, 1, 2), (0, 2, 3)
                const int32_t *r = &face[(size_t)q * 4];
                W.insert(W.end(), { r[0], r[1], r[2], r[0], r[2], r[3] });
            }
            break;
        }
        // an interior edge reads the points of the faces of its half-edges
        put_edges(R, lv, V, creased, sharp, MPT_SUBDIV_CC, [&](int32_t h) { return fp0 + lv.slot_face[(size_t)h]; });
        for (int64_t f = 0; f < F; f++) {
            R.ids.assign(face.begin() + at[(size_t)f], face.begin() + at[(size_t)f + 1]);
            R.put(V + E + f, MPT_SUBDIV_EDGE_BND, MPT_SUBDIV_CC, (int64_t)R.ids.size());
        }
        // face j of corners c_0 .. c_n-1 becomes the quads (c_i, e(c_i, c_i+1), f_j, e(c_i-1, c_i))
        std::vector<int32_t> next((size_t)S * 4);
        for (int64_t f = 0; f < F; f++) {
            const int32_t a0 = at[(size_t)f], n = at[(size_t)f + 1] - a0;
            for (int32_t i = 0; i < n; i++) {
                int32_t *q = &next[(size_t)(a0 + i) * 4];
                q[0] = face[(size_t)(a0 + i)]; q[1] = (int32_t)V + lv.face_edge[(size_t)(a0 + i)]; q[2] = fp0 + (int32_t)f;
                q[3] = (int32_t)V + lv.face_edge[(size_t)(a0 + (i + n - 1) % n)];
                if (l == 0) { quads1.push_back(tri0[(size_t)f]); quads1.push_back(n | i << 8); }
            }
        }
        face.swap(next);
        at = corners_at(S, 4);
        V += E + F;
    }
    return MPT_SUBDIV_OK;
}

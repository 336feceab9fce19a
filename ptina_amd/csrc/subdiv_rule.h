// subdiv_rule.h -- the pure piece of Loop subdivision's host side (scene_subdiv.cpp): the topology of a
// mesh and of its refinements, the tables subdiv.hip gathers through (the run tables of its launches are run_table.h's).  Plain
// C++17 with nothing of HIP and no context (as deform_rule.h), so that a stand-alone program can run it under a sanitizer
// (tools/subdiv_rule_check.cpp); the C ABI has it as mpt_subdiv_topology and, with creases and corners,
// as mpt_subdiv_topology_creased.  The definition it follows is stated in include/miptina.h and at the top of subdiv.hip.
// Catmull-Clark subdivision of a cage of polygons (mpt_subdiv_topology_cc) is the second half of this file.
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

// What the topology function hands back: per level 0..levels the counts, and ONE block of 32-bit words, the layout the device reads
// (offsets in words from the block's start):
//   [0, V_0)                      first corner of every control vertex
//   rule_at[l], l = 1..levels     V_l rules (two words each) of the vertices of level l, then their rings
//   nrule_at                      V_L rules of the rings of the last level (for the normals), then the rings
//   face_at                       [F_L][3] vertex ids of the last level's faces
// A rule is { kind | n << 2, ring }: `ring` is the offset of n vertex ids of the level below (nrule: of the last level) --
//   MPT_SUBDIV_VERT_INT   the n neighbours of an interior vertex in winding order, from the lowest id
//   MPT_SUBDIV_VERT_BND   the n neighbours of a boundary vertex, from the boundary neighbour that begins the fan to the one that ends it
//   MPT_SUBDIV_EDGE_INT   a b c d of an interior edge          MPT_SUBDIV_EDGE_BND   a b of a boundary edge
// The rings of a launch's rules lie behind its rules in the rules' order.
//
// A CREASED mesh (a sharpness above zero or a flagged corner; section 3.19.1) has the same block with more in it.  A head is
// kind | n << 2 | variant << 28, and beside variant 0, the plain rules above, there are
//   MPT_SUBDIV_VERT_INT | MPT_SUBDIV_BLEND_CREASE   the n neighbours, then p q, the far ends of the vertex's two sharp edges, then the
//                                                   f64 f (low word first):  ((1 - f) * M) + (f * C)
//   MPT_SUBDIV_VERT_INT | MPT_SUBDIV_BLEND_CORNER   the n neighbours, then the f64 f:  ((1 - f) * M) + (f * v)
//   MPT_SUBDIV_VERT_INT | MPT_SUBDIV_FIXED          n = 0: the vertex stays (a flagged corner; three or more sharp edges with f >= 1)
//   MPT_SUBDIV_EDGE_INT | MPT_SUBDIV_BLEND_EDGE     a b c d, then the f64 s:  ((1 - s) * E) + (s * H)
// A vertex of two sharp edges with f >= 1 is a plain MPT_SUBDIV_VERT_BND of n = 2, p q; an interior edge with s >= 1 a plain
// MPT_SUBDIV_EDGE_BND: the crease rules are the boundary's.  Behind the last level's rings (nrule_at: whole rings, as above, which
// the displacement's direction is taken of) lie
//   srule_at                      R rules of the last level's RECORDS, then R vertex ids, then the rings of the sectors
//   face_at                       [F_L][3] RECORD ids
// The hard edges of the last level cut a vertex's fan into sectors.  Record v < V_L is vertex v's first sector (from the ring's
// start), or its whole ring where no interior edge of it is hard -- then its rule is the nrule's, ring and all; a further sector is
// a record from V_L on, in the order of the vertices and then of the ring.  A sector's rule is a MPT_SUBDIV_VERT_BND of the
// neighbours from its first hard edge to its last (an interior vertex with one hard edge: n + 1 of them, the first again at the
// end).  An uncreased mesh has nrec = V_L, srule_at = 0 and the block of above, word for word.
struct MptSubdivTopo {
    int levels = 0;
    int64_t nv[MPT_SUBDIV_MAX_LEVELS + 1] = {}, ne[MPT_SUBDIV_MAX_LEVELS + 1] = {}, nf[MPT_SUBDIV_MAX_LEVELS + 1] = {}, nrec = 0;
    int32_t rule_at[MPT_SUBDIV_MAX_LEVELS + 1] = {}, nrule_at = 0, face_at = 0, srule_at = 0;
    std::vector<int32_t> words;
};

namespace mpt_subdiv_detail {

struct Say {
    char *why; size_t size;
    MptSubdivVerdict operator()(MptSubdivVerdict v, const char *fmt, long long a = 0, long long b = 0, long long c = 0) const {
        if (why && size) snprintf(why, size, fmt, a, b, c);
        return v;
    }
};

struct Level {                                  // one level's edges and rings, from its faces alone
    std::vector<int32_t> edge;                  // [E][4]: a b c d (d -1, c the third corner of its face: a boundary edge)
    std::vector<int32_t> face_edge;             // [F][3]: the edge of corners j -> j + 1
    std::vector<int32_t> ring_kind, ring_n, ring_at, ring;
};

struct HalfEdge { int32_t lo, hi, face, j, fwd; };

inline MptSubdivVerdict build_level(const std::vector<int32_t> &face, int64_t V, Level &out, const Say &say) {
    const int64_t F = (int64_t)face.size() / 3;
    std::vector<HalfEdge> he((size_t)F * 3);
    for (int64_t f = 0; f < F; f++)
        for (int j = 0; j < 3; j++) {
            const int32_t p = face[(size_t)(3 * f + j)], q = face[(size_t)(3 * f + (j + 1) % 3)];
            he[(size_t)(3 * f + j)] = { std::min(p, q), std::max(p, q), (int32_t)f, j, p < q ? 1 : 0 };
        }
    std::sort(he.begin(), he.end(), [](const HalfEdge &x, const HalfEdge &y) {
        if (x.lo != y.lo) return x.lo < y.lo;
        if (x.hi != y.hi) return x.hi < y.hi;
        if (x.face != y.face) return x.face < y.face;
        return x.j < y.j;
    });
    out.edge.clear(); out.face_edge.assign((size_t)F * 3, -1);
    for (size_t i = 0; i < he.size();) {
        size_t j = i + 1;
        while (j < he.size() && he[j].lo == he[i].lo && he[j].hi == he[i].hi) j++;
        if (j - i > 2) return say(MPT_SUBDIV_EDGE_FACES, "subdivision: face %lld is the third on the edge of vertices %lld and %lld", he[i + 2].face, he[i].lo, he[i].hi);
        if (j - i == 2 && he[i].fwd == he[i + 1].fwd)
            return say(MPT_SUBDIV_EDGE_DIRECTION, "subdivision: faces %lld and %lld run their shared edge in the same direction (vertex %lld first)", he[i].face,
                       he[i + 1].face, he[i].fwd ? he[i].lo : he[i].hi);
        const int32_t e = (int32_t)(out.edge.size() / 4);
        int32_t c = -1, d = -1;
        for (size_t h = i; h < j; h++) {
            const int32_t opp = face[(size_t)(3 * (int64_t)he[h].face + (he[h].j + 2) % 3)];
            if (j - i == 1 || he[h].fwd) c = opp; else d = opp;
            out.face_edge[(size_t)(3 * (int64_t)he[h].face + he[h].j)] = e;
        }
        out.edge.insert(out.edge.end(), { he[i].lo, he[i].hi, c, d });
        i = j;
    }
    // the faces of every vertex (counting sort), then its ring
    std::vector<int64_t> first((size_t)V + 1, 0);
    for (int32_t v : face) first[(size_t)v + 1]++;
    for (int64_t v = 0; v < V; v++) first[(size_t)v + 1] += first[(size_t)v];
    std::vector<int32_t> slot((size_t)F * 3);
    {
        std::vector<int64_t> at(first.begin(), first.end() - 1);
        for (int64_t s = 0; s < F * 3; s++) slot[(size_t)at[(size_t)face[(size_t)s]]++] = (int32_t)s;
    }
    out.ring_kind.assign((size_t)V, 0); out.ring_n.assign((size_t)V, 0); out.ring_at.assign((size_t)V, 0); out.ring.clear();
    std::vector<int32_t> src, dst; std::vector<char> used;
    for (int64_t v = 0; v < V; v++) {
        const int64_t n = first[(size_t)v + 1] - first[(size_t)v];
        src.resize((size_t)n); dst.resize((size_t)n); used.assign((size_t)n, 0);
        for (int64_t i = 0; i < n; i++) {
            const int32_t s = slot[(size_t)(first[(size_t)v] + i)], f = s / 3, j = s % 3;
            src[(size_t)i] = face[(size_t)(3 * (int64_t)f + (j + 1) % 3)]; dst[(size_t)i] = face[(size_t)(3 * (int64_t)f + (j + 2) % 3)];
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
            out.ring.push_back(cur);
        }
        if (!boundary) {
            if (cur != lowest) return say(MPT_SUBDIV_FAN, fan, n, v);
            out.ring.pop_back();
        }
        out.ring_kind[(size_t)v] = boundary ? MPT_SUBDIV_VERT_BND : MPT_SUBDIV_VERT_INT;
        out.ring_n[(size_t)v] = (int32_t)(boundary ? n + 1 : n);
    }
    return MPT_SUBDIV_OK;
}

struct Spoke { double s; int32_t far; };         // a sharp edge of a vertex: its sharpness at the level, its far end

// the edge of vertices p and q of a level (its edges are sorted by (lower id, higher id))
template <class AnyLevel> inline int64_t edge_of(const AnyLevel &lv, int32_t p, int32_t q) {
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

// The records of a creased mesh's last level, appended to the block: the hard edges (sharpness > 0 at this level, or a boundary) cut
// a vertex's fan into sectors, each an open ring from one hard edge to the next.  Record v is vertex v's first sector -- its whole
// ring where no interior edge of it is hard -- and the others follow V_L in the vertices' order.  face [F][corners]: the last
// level's faces (Loop's triangles, Catmull-Clark's quads) by vertex on entry, by record on return
template <class AnyLevel, class Sharp>
inline void append_records(const AnyLevel &lv, int64_t V, int corners, const Sharp &sharp, MptSubdivTopo &out, std::vector<int32_t> &face) {
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

}  // namespace mpt_subdiv_detail

// The topology of the mesh verts [3k][8] (pos3 nrm3 uv2, f32; only the positions are read) and of `levels` Loop refinements of it,
// with the sharpnesses crease [k][3] (edge j of face f runs from corner j to corner (j + 1) % 3; null: all zero) and the corner
// flags corner [k][3] (null: none).  A refusal writes its words, which name the face and the edge or the vertex, to `why` (always
// terminated) and leaves `out` unspecified.
inline MptSubdivVerdict mpt_subdiv_topology_creased_of(const float *verts, int k, int levels, const float *crease, const uint8_t *corner, MptSubdivTopo &out,
                                                       char *why, size_t why_size) {
    using namespace mpt_subdiv_detail;
    const Say say{ why, why_size };
    if (why && why_size) why[0] = 0;
    if (k < 0 || (k > 0 && !verts)) return say(MPT_SUBDIV_ARGS, "subdivision: verts must hold [%lld][8] values", 3LL * k);
    if (levels < 1 || levels > MPT_SUBDIV_MAX_LEVELS) return say(MPT_SUBDIV_LEVELS, "subdivision: levels %lld outside [1, %lld]", levels, MPT_SUBDIV_MAX_LEVELS);
    if (((long long)k << (2 * levels)) > MPT_SUBDIV_MAX_FACES)
        return say(MPT_SUBDIV_TOO_MANY, "subdivision: too many faces: %lld at level %lld, at most %lld", (long long)k << (2 * levels), levels, MPT_SUBDIV_MAX_FACES);
    bool creased = false;
    for (int64_t s = 0; crease && s < (int64_t)k * 3; s++) {
        const float x = crease[(size_t)s];
        if (std::isnan(x)) return say(MPT_SUBDIV_CREASE, "subdivision: the crease of edge %lld of face %lld is not a number", s % 3, s / 3);
        if (x < 0.0f) return say(MPT_SUBDIV_CREASE, "subdivision: the crease of edge %lld of face %lld is negative", s % 3, s / 3);
        creased = creased || x > 0.0f;
    }
    for (int64_t s = 0; corner && s < (int64_t)k * 3; s++) creased = creased || corner[(size_t)s] != 0;
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
    // a control vertex is a corner if any of its welded corners is flagged; the flags pass to even vertices only (their ids stay)
    std::vector<char> flagged((size_t)V, 0);
    for (int64_t s = 0; corner && s < (int64_t)k * 3; s++)
        if (corner[(size_t)s]) flagged[(size_t)face[(size_t)s]] = 1;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> cage, below;            // per edge of the level: the CAGE sharpness it inherits (0: an edge new inside a face)
    std::vector<Spoke> S;
    std::vector<int32_t> ids;
    int64_t V_below = 0;
    Level lv;
    for (int l = 0; l <= levels; l++) {
        const MptSubdivVerdict verdict = build_level(face, V, lv, say);
        if (verdict != MPT_SUBDIV_OK) return verdict;
        const int64_t E = (int64_t)lv.edge.size() / 4, F = (int64_t)face.size() / 3;
        out.nv[l] = V; out.ne[l] = E; out.nf[l] = F;
        below.swap(cage);
        cage.assign((size_t)E, 0.0);
        if (l == 0) {                           // the two faces on an edge may state different values: the edge takes the larger
            for (int64_t s = 0; crease && s < F * 3; s++) {
                double &c = cage[(size_t)lv.face_edge[(size_t)s]];
                c = std::max(c, (double)crease[(size_t)s]);
            }
        } else if (creased) {                   // both halves of a split edge inherit; an edge between two edge vertices is new
            for (int64_t e = 0; e < E; e++) {
                const int32_t lo = lv.edge[(size_t)e * 4], hi = lv.edge[(size_t)e * 4 + 1];
                if (lo < V_below) cage[(size_t)e] = below[(size_t)(hi - V_below)];
            }
        }
        // the sharpness of edge e at this level: s0 - l where that is positive, else 0; a boundary edge counts as inf
        const auto sharp = [&](int64_t e) {
            if (lv.edge[(size_t)e * 4 + 3] < 0) return inf;
            const double s = cage[(size_t)e] - (double)l;
            return s > 0.0 ? s : 0.0;
        };
        const bool last = l == levels;
        const int64_t nrules = last ? V : V + E;
        const size_t rules = W.size();
        if (last) out.nrule_at = (int32_t)rules; else out.rule_at[l + 1] = (int32_t)rules;
        W.resize(rules + (size_t)nrules * 2);
        // a rule's ids (and the f64 parameter some variants end with, low word first) are appended in the rules' order
        const auto put = [&](size_t at, int64_t i, int kind, int variant, int64_t n, const std::vector<int32_t> &words) {
            W[at + (size_t)i * 2] = (int32_t)(kind | n << 2 | variant << MPT_SUBDIV_VARIANT_SHIFT);
            W[at + (size_t)i * 2 + 1] = (int32_t)W.size();
            W.insert(W.end(), words.begin(), words.end());
        };
        const auto push_f64 = [&](double x) { int32_t w[2]; memcpy(w, &x, 8); ids.push_back(w[0]); ids.push_back(w[1]); };
        for (int64_t v = 0; v < V; v++) {
            const int32_t *ring = &lv.ring[(size_t)lv.ring_at[(size_t)v]];
            const int64_t n = lv.ring_n[(size_t)v];
            const int kind = lv.ring_kind[(size_t)v];
            ids.assign(ring, ring + n);
            if (last || !creased) { put(rules, v, kind, MPT_SUBDIV_PLAIN, n, ids); continue; }
            S.clear();
            for (int64_t i = 0; i < n; i++) {
                const double s = sharp(edge_of(lv, (int32_t)v, ring[i]));
                if (s > 0.0) S.push_back({ s, ring[i] });
            }
            const size_t ks = S.size();
            const bool bnd = kind == MPT_SUBDIV_VERT_BND;
            if (v < (int64_t)flagged.size() && flagged[(size_t)v]) { ids.clear(); put(rules, v, MPT_SUBDIV_VERT_INT, MPT_SUBDIV_FIXED, 0, ids); }
            else if (ks <= 1 || (bnd && ks == 2)) put(rules, v, kind, MPT_SUBDIV_PLAIN, n, ids);       // (a boundary vertex's two boundary edges: today's rule)
            else if (ks == 2) {
                const double f = 0.5 * (S[0].s + S[1].s);
                if (f >= 1.0) { ids = { S[0].far, S[1].far }; put(rules, v, MPT_SUBDIV_VERT_BND, MPT_SUBDIV_PLAIN, 2, ids); }
                else { ids.push_back(S[0].far); ids.push_back(S[1].far); push_f64(f); put(rules, v, MPT_SUBDIV_VERT_INT, MPT_SUBDIV_BLEND_CREASE, n, ids); }
            } else {
                double f = S[0].s + S[1].s;
                for (size_t i = 2; i < ks; i++) f = f + S[i].s;
                f = f / (double)ks;
                if (f >= 1.0) { ids.clear(); put(rules, v, MPT_SUBDIV_VERT_INT, MPT_SUBDIV_FIXED, 0, ids); }
                else { push_f64(f); put(rules, v, MPT_SUBDIV_VERT_INT, MPT_SUBDIV_BLEND_CORNER, n, ids); }
            }
        }
        if (last) {
            out.nrec = V; out.srule_at = 0;
            if (creased) append_records(lv, V, 3, sharp, out, face);      // (the face table then indexes records)
            break;
        }
        for (int64_t e = 0; e < E; e++) {
            const bool inner = lv.edge[(size_t)e * 4 + 3] >= 0;
            const double s = creased ? sharp(e) : 0.0;
            const bool half = !inner || s >= 1.0;            // 0.5 * (a + b): a boundary edge, and an edge that is sharp at this level
            ids.assign(4, 0);
            for (int a = 0; a < 4; a++) ids[(size_t)a] = !half || a < 2 ? lv.edge[(size_t)e * 4 + (size_t)a] : 0;
            if (half) put(rules, V + e, MPT_SUBDIV_EDGE_BND, MPT_SUBDIV_PLAIN, 2, ids);
            else if (s == 0.0) put(rules, V + e, MPT_SUBDIV_EDGE_INT, MPT_SUBDIV_PLAIN, 4, ids);
            else { push_f64(s); put(rules, V + e, MPT_SUBDIV_EDGE_INT, MPT_SUBDIV_BLEND_EDGE, 4, ids); }
        }
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
        V_below = V;
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

// ---------------------------------------------------------------- Catmull-Clark
// The topology of a cage of POLYGONS and of `levels` Catmull-Clark refinements of it.  The mesh verts [3k][8] holds polygon j, of
// polys[j] corners, as polys[j] - 2 consecutive triangles, a fan about its first corner: triangle i is (c_0, c_i+1, c_i+2) (polys
// null: every triangle is a polygon).  crease and corner are flat [sum polys]: entry i of polygon j is the edge from its corner i to
// corner (i + 1) % n, respectively its corner i.  Level 0 has the polygons for faces, every later level quads: polygon or quad j
// of corners c_0 .. c_n-1 becomes the quads (c_i, e(c_i, c_i+1), f_j, e(c_i-1, c_i)), at level 1 from the sum of the n before it,
// later 4 j + i.  Vertex ids of level l + 1: V_l even vertices, then the E_l edge points, then the F_l face points.
//
// The block has the layout of above, with these differences:
//   rule_at[l]                    V_l-1 + E_l-1 + F_l-1 rules: the vertices, the edges, then the FACES of level l - 1, then the rings
//   quad_at                       [Q_1][2] per quad of level 1: the first triangle of its polygon in the mesh, n | i << 8
//   face_at                       [2 Q_L][3] record ids: quad q = (v0, v1, v2, v3) of the last level is faces 2q (v0, v1, v2), 2q + 1 (v0, v2, v3)
// A boundary vertex, a boundary edge (and an edge of sharpness >= 1), a vertex that stays and the rings and sectors of the last
// level have the heads of above: those rules are Loop's.  The rules that are Catmull-Clark's carry MPT_SUBDIV_CC in the variant:
//   MPT_SUBDIV_EDGE_BND | MPT_SUBDIV_CC          a FACE POINT: the n corners of the face in its own order
//   MPT_SUBDIV_EDGE_INT | MPT_SUBDIV_CC          n = 4: a b, then the ids at level l of the face points of the face that runs a -> b
//                                                and of the other (a face point's rule is rule `id` of the same launch: the lane
//                                                evaluates it again);  | MPT_SUBDIV_BLEND_EDGE: then the f64 s
//   MPT_SUBDIV_VERT_INT | MPT_SUBDIV_CC          the n neighbours, then n face point ids, the i-th the face between r_i and r_i+1;
//                                                | MPT_SUBDIV_BLEND_CREASE: then p q and the f64 f;  | MPT_SUBDIV_BLEND_CORNER: then the f64 f
struct MptSubdivTopoCC : MptSubdivTopo { int32_t quad_at = 0; int64_t nquads1 = 0; };

namespace mpt_subdiv_detail {

struct LevelCC {                                // one level's edges and rings, from its faces (corner lists) alone
    std::vector<int32_t> edge;                  // [E][4]: a b f1 f2 -- f1 the face that runs a -> b, f2 the other; a boundary edge: f1 its face, f2 -1
    std::vector<int32_t> face_edge;             // per corner slot: the edge of corners i -> i + 1
    std::vector<int32_t> ring_kind, ring_n, ring_at, ring, ring_face;   // ring_face: beside ring, the face between r_i and r_i+1 (-1 behind a boundary ring's last)
};

// faces: corner lists, face f's at [at[f], at[f + 1])
inline MptSubdivVerdict build_level_cc(const std::vector<int32_t> &at, const std::vector<int32_t> &face, int64_t V, LevelCC &out, const Say &say) {
    const int64_t F = (int64_t)at.size() - 1, S = (int64_t)face.size();
    std::vector<HalfEdge> he((size_t)S);
    for (int64_t f = 0; f < F; f++) {
        const int32_t n = at[(size_t)f + 1] - at[(size_t)f];
        for (int32_t j = 0; j < n; j++) {
            const int32_t p = face[(size_t)(at[(size_t)f] + j)], q = face[(size_t)(at[(size_t)f] + (j + 1) % n)];
            he[(size_t)(at[(size_t)f] + j)] = { std::min(p, q), std::max(p, q), (int32_t)f, j, p < q ? 1 : 0 };
        }
    }
    std::sort(he.begin(), he.end(), [](const HalfEdge &x, const HalfEdge &y) {
        if (x.lo != y.lo) return x.lo < y.lo;
        if (x.hi != y.hi) return x.hi < y.hi;
        if (x.face != y.face) return x.face < y.face;
        return x.j < y.j;
    });
    out.edge.clear(); out.face_edge.assign((size_t)S, -1);
    for (size_t i = 0; i < he.size();) {
        size_t j = i + 1;
        while (j < he.size() && he[j].lo == he[i].lo && he[j].hi == he[i].hi) j++;
        if (j - i > 2) return say(MPT_SUBDIV_EDGE_FACES, "subdivision: face %lld is the third on the edge of vertices %lld and %lld", he[i + 2].face, he[i].lo, he[i].hi);
        if (j - i == 2 && he[i].fwd == he[i + 1].fwd)
            return say(MPT_SUBDIV_EDGE_DIRECTION, "subdivision: faces %lld and %lld run their shared edge in the same direction (vertex %lld first)", he[i].face,
                       he[i + 1].face, he[i].fwd ? he[i].lo : he[i].hi);
        const int32_t e = (int32_t)(out.edge.size() / 4);
        int32_t f1 = -1, f2 = -1;
        for (size_t h = i; h < j; h++) {
            if (j - i == 1 || he[h].fwd) f1 = he[h].face; else f2 = he[h].face;
            out.face_edge[(size_t)(at[(size_t)he[h].face] + he[h].j)] = e;
        }
        out.edge.insert(out.edge.end(), { he[i].lo, he[i].hi, f1, f2 });
        i = j;
    }
    // the corner slots of every vertex (counting sort), then its ring of edge neighbours
    std::vector<int32_t> slot_face((size_t)S);
    for (int64_t f = 0; f < F; f++)
        for (int32_t s = at[(size_t)f]; s < at[(size_t)f + 1]; s++) slot_face[(size_t)s] = (int32_t)f;
    std::vector<int64_t> first((size_t)V + 1, 0);
    for (int32_t v : face) first[(size_t)v + 1]++;
    for (int64_t v = 0; v < V; v++) first[(size_t)v + 1] += first[(size_t)v];
    std::vector<int32_t> slot((size_t)S);
    {
        std::vector<int64_t> put(first.begin(), first.end() - 1);
        for (int64_t s = 0; s < S; s++) slot[(size_t)put[(size_t)face[(size_t)s]]++] = (int32_t)s;
    }
    out.ring_kind.assign((size_t)V, 0); out.ring_n.assign((size_t)V, 0); out.ring_at.assign((size_t)V, 0); out.ring.clear(); out.ring_face.clear();
    std::vector<int32_t> src, dst, fc; std::vector<char> used;
    for (int64_t v = 0; v < V; v++) {
        const int64_t n = first[(size_t)v + 1] - first[(size_t)v];
        src.resize((size_t)n); dst.resize((size_t)n); fc.resize((size_t)n); used.assign((size_t)n, 0);
        for (int64_t i = 0; i < n; i++) {               // in face (v, a, ..., b), a comes before b
            const int32_t s = slot[(size_t)(first[(size_t)v] + i)], f = slot_face[(size_t)s], a0 = at[(size_t)f], m = at[(size_t)f + 1] - a0, j = s - a0;
            src[(size_t)i] = face[(size_t)(a0 + (j + 1) % m)]; dst[(size_t)i] = face[(size_t)(a0 + (j + m - 1) % m)]; fc[(size_t)i] = f;
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

}  // namespace mpt_subdiv_detail

// A refusal writes its words, which name the face, the polygon, the edge or the vertex, to `why` (always terminated) and leaves
// `out` unspecified
inline MptSubdivVerdict mpt_subdiv_topology_cc_of(const float *verts, int k, int levels, const int32_t *polys, int m, const float *crease, const uint8_t *corner,
                                                  MptSubdivTopoCC &out, char *why, size_t why_size) {
    using namespace mpt_subdiv_detail;
    const Say say{ why, why_size };
    if (why && why_size) why[0] = 0;
    if (k < 0 || (k > 0 && !verts)) return say(MPT_SUBDIV_ARGS, "subdivision: verts must hold [%lld][8] values", 3LL * k);
    if (levels < 1 || levels > MPT_SUBDIV_MAX_LEVELS) return say(MPT_SUBDIV_LEVELS, "subdivision: levels %lld outside [1, %lld]", levels, MPT_SUBDIV_MAX_LEVELS);
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
    if (((long long)(2 * S0) << (2 * (levels - 1))) > MPT_SUBDIV_MAX_FACES)
        return say(MPT_SUBDIV_TOO_MANY, "subdivision: too many faces: %lld at level %lld, at most %lld", (long long)(2 * S0) << (2 * (levels - 1)), levels, MPT_SUBDIV_MAX_FACES);
    // the corner slot a crease or a flag is named by: the polygon and the entry in it
    const auto owner = [&](int64_t s) { return (int64_t)(std::upper_bound(at.begin(), at.end(), (int32_t)s) - at.begin()) - 1; };
    bool creased = false;
    for (int64_t s = 0; crease && s < S0; s++) {
        const float x = crease[(size_t)s];
        if (std::isnan(x)) return say(MPT_SUBDIV_CREASE, "subdivision: the crease of edge %lld of polygon %lld is not a number", s - at[(size_t)owner(s)], owner(s));
        if (x < 0.0f) return say(MPT_SUBDIV_CREASE, "subdivision: the crease of edge %lld of polygon %lld is negative", s - at[(size_t)owner(s)], owner(s));
        creased = creased || x > 0.0f;
    }
    for (int64_t s = 0; corner && s < S0; s++) creased = creased || corner[(size_t)s] != 0;
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
    std::vector<char> flagged((size_t)V, 0);
    for (int64_t s = 0; corner && s < S0; s++)
        if (corner[(size_t)s]) flagged[(size_t)face[(size_t)s]] = 1;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> cage, below;            // per edge of the level: the CAGE sharpness it inherits (0: an edge new inside a face)
    std::vector<Spoke> Sp;
    std::vector<int32_t> ids, quads1;
    int64_t V_below = 0;
    LevelCC lv;
    for (int l = 0; l <= levels; l++) {
        const MptSubdivVerdict verdict = build_level_cc(at, face, V, lv, say);
        if (verdict != MPT_SUBDIV_OK) return verdict;
        const int64_t E = (int64_t)lv.edge.size() / 4, F = (int64_t)at.size() - 1, S = (int64_t)face.size();
        out.nv[l] = V; out.ne[l] = E; out.nf[l] = F;
        below.swap(cage);
        cage.assign((size_t)E, 0.0);
        if (l == 0) {                           // the two faces on an edge may state different values: the edge takes the larger
            for (int64_t s = 0; crease && s < S; s++) {
                double &c = cage[(size_t)lv.face_edge[(size_t)s]];
                c = std::max(c, (double)crease[(size_t)s]);
            }
        } else if (creased) {                   // both halves of a split edge inherit (an even vertex's edges all end in edge points); the others are new
            for (int64_t e = 0; e < E; e++) {
                const int32_t lo = lv.edge[(size_t)e * 4], hi = lv.edge[(size_t)e * 4 + 1];
                if (lo < V_below) cage[(size_t)e] = below[(size_t)(hi - V_below)];
            }
        }
        const auto sharp = [&](int64_t e) {
            if (lv.edge[(size_t)e * 4 + 3] < 0) return inf;
            const double s = cage[(size_t)e] - (double)l;
            return s > 0.0 ? s : 0.0;
        };
        const bool last = l == levels;
        const int64_t nrules = last ? V : V + E + F;
        const size_t rules = W.size();
        if (last) out.nrule_at = (int32_t)rules; else out.rule_at[l + 1] = (int32_t)rules;
        W.resize(rules + (size_t)nrules * 2);
        const auto put = [&](size_t base, int64_t i, int kind, int variant, int64_t n, const std::vector<int32_t> &words) {
            W[base + (size_t)i * 2] = (int32_t)(kind | n << 2 | variant << MPT_SUBDIV_VARIANT_SHIFT);
            W[base + (size_t)i * 2 + 1] = (int32_t)W.size();
            W.insert(W.end(), words.begin(), words.end());
        };
        const auto push_f64 = [&](double x) { int32_t w[2]; memcpy(w, &x, 8); ids.push_back(w[0]); ids.push_back(w[1]); };
        const int32_t fp0 = (int32_t)(V + E);       // the id at level l + 1 of face 0's point
        for (int64_t v = 0; v < V; v++) {
            const size_t rat = (size_t)lv.ring_at[(size_t)v];
            const int32_t *ring = &lv.ring[rat];
            const int64_t n = lv.ring_n[(size_t)v];
            const int kind = lv.ring_kind[(size_t)v];
            ids.assign(ring, ring + n);
            if (last) { put(rules, v, kind, MPT_SUBDIV_PLAIN, n, ids); continue; }
            const bool bnd = kind == MPT_SUBDIV_VERT_BND;
            const auto smooth = [&](int variant) {          // (a boundary vertex's rule reads p and q alone: Loop's words)
                if (bnd) { put(rules, v, kind, MPT_SUBDIV_PLAIN, n, ids); return; }
                std::vector<int32_t> tail(ids.begin() + n, ids.end());
                ids.resize((size_t)n);
                for (int64_t i = 0; i < n; i++) ids.push_back(fp0 + lv.ring_face[rat + (size_t)i]);
                ids.insert(ids.end(), tail.begin(), tail.end());
                put(rules, v, kind, variant | MPT_SUBDIV_CC, n, ids);
            };
            if (!creased) { smooth(MPT_SUBDIV_PLAIN); continue; }
            Sp.clear();
            for (int64_t i = 0; i < n; i++) {
                const double s = sharp(edge_of(lv, (int32_t)v, ring[i]));
                if (s > 0.0) Sp.push_back({ s, ring[i] });
            }
            const size_t ks = Sp.size();
            if (v < (int64_t)flagged.size() && flagged[(size_t)v]) { ids.clear(); put(rules, v, MPT_SUBDIV_VERT_INT, MPT_SUBDIV_FIXED, 0, ids); }
            else if (ks <= 1 || (bnd && ks == 2)) smooth(MPT_SUBDIV_PLAIN);
            else if (ks == 2) {
                const double f = 0.5 * (Sp[0].s + Sp[1].s);
                if (f >= 1.0) { ids = { Sp[0].far, Sp[1].far }; put(rules, v, MPT_SUBDIV_VERT_BND, MPT_SUBDIV_PLAIN, 2, ids); }
                else { ids.push_back(Sp[0].far); ids.push_back(Sp[1].far); push_f64(f); smooth(MPT_SUBDIV_BLEND_CREASE); }
            } else {
                double f = Sp[0].s + Sp[1].s;
                for (size_t i = 2; i < ks; i++) f = f + Sp[i].s;
                f = f / (double)ks;
                if (f >= 1.0) { ids.clear(); put(rules, v, MPT_SUBDIV_VERT_INT, MPT_SUBDIV_FIXED, 0, ids); }
                else { push_f64(f); smooth(MPT_SUBDIV_BLEND_CORNER); }      // (an interior vertex: a boundary vertex's S holds an inf)
            }
        }
        if (last) {
            out.nrec = V; out.srule_at = 0;
            if (creased) append_records(lv, V, 4, sharp, out, face);
            out.quad_at = (int32_t)W.size(); out.nquads1 = (int64_t)quads1.size() / 2;
            W.insert(W.end(), quads1.begin(), quads1.end());
            out.face_at = (int32_t)W.size();
            for (int64_t q = 0; q < F; q++) {          // a quad (by record, if creased) is emitted as (0, 1, 2), (0, 2, 3)
                const int32_t *r = &face[(size_t)q * 4];
                W.insert(W.end(), { r[0], r[1], r[2], r[0], r[2], r[3] });
            }
            break;
        }
        for (int64_t e = 0; e < E; e++) {
            const int32_t *ed = &lv.edge[(size_t)e * 4];
            const bool inner = ed[3] >= 0;
            const double s = creased ? sharp(e) : 0.0;
            const bool half = !inner || s >= 1.0;            // 0.5 * (a + b): a boundary edge, and an edge that is sharp at this level
            if (half) { ids = { ed[0], ed[1], 0, 0 }; put(rules, V + e, MPT_SUBDIV_EDGE_BND, MPT_SUBDIV_PLAIN, 2, ids); continue; }
            ids = { ed[0], ed[1], fp0 + ed[2], fp0 + ed[3] };
            if (s == 0.0) put(rules, V + e, MPT_SUBDIV_EDGE_INT, MPT_SUBDIV_CC, 4, ids);
            else { push_f64(s); put(rules, V + e, MPT_SUBDIV_EDGE_INT, MPT_SUBDIV_CC | MPT_SUBDIV_BLEND_EDGE, 4, ids); }
        }
        for (int64_t f = 0; f < F; f++) {
            ids.assign(face.begin() + at[(size_t)f], face.begin() + at[(size_t)f + 1]);
            put(rules, V + E + f, MPT_SUBDIV_EDGE_BND, MPT_SUBDIV_CC, (int64_t)ids.size(), ids);
        }
        // face j of corners c_0 .. c_n-1 becomes the quads (c_i, e(c_i, c_i+1), f_j, e(c_i-1, c_i))
        std::vector<int32_t> next((size_t)S * 4), next_at((size_t)S + 1);
        for (int64_t f = 0; f < F; f++) {
            const int32_t a0 = at[(size_t)f], n = at[(size_t)f + 1] - a0;
            for (int32_t i = 0; i < n; i++) {
                int32_t *q = &next[(size_t)(a0 + i) * 4];
                q[0] = face[(size_t)(a0 + i)]; q[1] = (int32_t)V + lv.face_edge[(size_t)(a0 + i)]; q[2] = fp0 + (int32_t)f;
                q[3] = (int32_t)V + lv.face_edge[(size_t)(a0 + (i + n - 1) % n)];
                if (l == 0) { quads1.push_back(tri0[(size_t)f]); quads1.push_back(n | i << 8); }
            }
        }
        for (int64_t s = 0; s <= S; s++) next_at[(size_t)s] = (int32_t)(4 * s);
        face.swap(next); at.swap(next_at);
        V_below = V;
        V += E + F;
    }
    return MPT_SUBDIV_OK;
}

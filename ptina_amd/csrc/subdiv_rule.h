// subdiv_rule.h -- the pure piece of Loop subdivision's host side (scene_subdiv.cpp): the topology of a
// mesh and of its refinements, the tables subdiv.hip gathers through (the run tables of its launches are run_table.h's).  Plain
// C++17 with nothing of HIP and no context (as deform_rule.h), so that a stand-alone program can run it under a sanitizer
// (tools/subdiv_rule_check.cpp); the C ABI has it as mpt_subdiv_topology.  The definition it follows is stated in
// include/miptina.h and at the top of subdiv.hip.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>
#include "mpt_types.h"          // MPT_SUBDIV_* (plain structures and constants)

enum MptSubdivVerdict {
    MPT_SUBDIV_OK = 0, MPT_SUBDIV_ARGS, MPT_SUBDIV_LEVELS, MPT_SUBDIV_TOO_MANY, MPT_SUBDIV_NOT_FINITE, MPT_SUBDIV_DEGENERATE,
    MPT_SUBDIV_EDGE_FACES, MPT_SUBDIV_EDGE_DIRECTION, MPT_SUBDIV_FAN
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
struct MptSubdivTopo {
    int levels = 0;
    int64_t nv[MPT_SUBDIV_MAX_LEVELS + 1] = {}, ne[MPT_SUBDIV_MAX_LEVELS + 1] = {}, nf[MPT_SUBDIV_MAX_LEVELS + 1] = {};
    int32_t rule_at[MPT_SUBDIV_MAX_LEVELS + 1] = {}, nrule_at = 0, face_at = 0;
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

struct KeyHash {
    size_t operator()(const uint64_t &k) const { return (size_t)(k * 0x9E3779B97F4A7C15ull >> 17); }
};

}  // namespace mpt_subdiv_detail

// The topology of the mesh verts [3k][8] (pos3 nrm3 uv2, f32; only the positions are read) and of `levels` Loop refinements of it.
// A refusal writes its words, which name the face or the vertex, to `why` (always terminated) and leaves `out` unspecified.
inline MptSubdivVerdict mpt_subdiv_topology_of(const float *verts, int k, int levels, MptSubdivTopo &out, char *why, size_t why_size) {
    using namespace mpt_subdiv_detail;
    const Say say{ why, why_size };
    if (why && why_size) why[0] = 0;
    if (k < 0 || (k > 0 && !verts)) return say(MPT_SUBDIV_ARGS, "subdivision: verts must hold [%lld][8] values", 3LL * k);
    if (levels < 1 || levels > MPT_SUBDIV_MAX_LEVELS) return say(MPT_SUBDIV_LEVELS, "subdivision: levels %lld outside [1, %lld]", levels, MPT_SUBDIV_MAX_LEVELS);
    if (((long long)k << (2 * levels)) > MPT_SUBDIV_MAX_FACES)
        return say(MPT_SUBDIV_TOO_MANY, "subdivision: too many faces: %lld at level %lld, at most %lld", (long long)k << (2 * levels), levels, MPT_SUBDIV_MAX_FACES);
    // control vertices: corners whose positions are equal as values (-0 is +0), numbered by first appearance
    std::vector<int32_t> face((size_t)k * 3), first_corner;
    {
        struct Key { uint32_t x, y, z; bool operator==(const Key &o) const { return x == o.x && y == o.y && z == o.z; } };
        struct Hash { size_t operator()(const Key &q) const { return KeyHash()(((uint64_t)q.x << 32 | q.y) ^ (uint64_t)q.z * 0xD6E8FEB86659FD93ull); } };
        std::unordered_map<Key, int32_t, Hash> ids;
        ids.reserve((size_t)k * 2);
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
            face[(size_t)s] = it->second;
        }
    }
    for (int64_t f = 0; f < k; f++) {
        const int32_t *v = &face[(size_t)f * 3];
        if (v[0] == v[1] || v[1] == v[2] || v[2] == v[0]) return say(MPT_SUBDIV_DEGENERATE, "subdivision: face %lld has two corners on one vertex (vertex %lld)", f, v[0] == v[1] || v[0] == v[2] ? v[0] : v[1]);
    }
    out = MptSubdivTopo{};
    out.levels = levels;
    std::vector<int32_t> &W = out.words;
    W.assign(first_corner.begin(), first_corner.end());
    int64_t V = (int64_t)first_corner.size();
    Level lv;
    for (int l = 0; l <= levels; l++) {
        const MptSubdivVerdict verdict = build_level(face, V, lv, say);
        if (verdict != MPT_SUBDIV_OK) return verdict;
        const int64_t E = (int64_t)lv.edge.size() / 4, F = (int64_t)face.size() / 3;
        out.nv[l] = V; out.ne[l] = E; out.nf[l] = F;
        const bool last = l == levels;
        const int64_t nrules = last ? V : V + E;
        const size_t rules = W.size(), rings = rules + (size_t)nrules * 2;
        if (last) out.nrule_at = (int32_t)rules; else out.rule_at[l + 1] = (int32_t)rules;
        W.resize(rings + lv.ring.size() + (last ? 0 : (size_t)E * 4));
        std::copy(lv.ring.begin(), lv.ring.end(), W.begin() + (std::ptrdiff_t)rings);
        for (int64_t v = 0; v < V; v++) {
            W[rules + (size_t)v * 2] = lv.ring_kind[(size_t)v] | lv.ring_n[(size_t)v] << 2;
            W[rules + (size_t)v * 2 + 1] = (int32_t)(rings + (size_t)lv.ring_at[(size_t)v]);
        }
        if (last) break;
        const size_t erings = rings + lv.ring.size();
        for (int64_t e = 0; e < E; e++) {
            const bool inner = lv.edge[(size_t)e * 4 + 3] >= 0;
            for (int a = 0; a < 4; a++) W[erings + (size_t)e * 4 + (size_t)a] = inner || a < 2 ? lv.edge[(size_t)e * 4 + (size_t)a] : 0;
            W[rules + (size_t)(V + e) * 2] = inner ? (MPT_SUBDIV_EDGE_INT | 4 << 2) : (MPT_SUBDIV_EDGE_BND | 2 << 2);
            W[rules + (size_t)(V + e) * 2 + 1] = (int32_t)(erings + (size_t)e * 4);
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
        V += E;
    }
    out.face_at = (int32_t)W.size();
    W.insert(W.end(), face.begin(), face.end());
    return MPT_SUBDIV_OK;
}

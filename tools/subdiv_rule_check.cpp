// subdiv_rule_check.cpp -- the pure host piece of Loop subdivision (ptina_amd/csrc/subdiv_rule.h: the topology of a mesh and its
// refinements; the run table of a launch is tools/run_table_check.cpp's) exercised by a stand-alone program, so that it can run
// under the host sanitizers without a GPU and without loading anything into an interpreter:
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/subdiv_rule_check.cpp -o subdiv_rule_check && ./subdiv_rule_check
//
// Every fixture topology of tests/subdiv_ref.py (built here procedurally: triangle, pair, tetrahedron, octahedron, icosahedron,
// closed fans of valence 7 and 12, the open 5 x 5 grid, the open cylinder) at levels 1 to 4, from record arrays that are exactly as
// long as the function may read: counts (Euler's number on the closed ones, four faces per face), every id of every table inside
// its level, every ring inside the block; every refusal, with message buffers of every size (cut, terminated, never overrun).
// The same fixtures CREASED, from crease and corner arrays that are exactly as long as the function may
// read -- every edge inf; a pattern of 0, 0.25, 0.5, 1, 1.5, 2.5 and inf that the two faces on an edge state differently, with every
// seventh corner flagged --: every variant's ids and parameter inside the block, a blend's parameter inside (0, 1), every record's
// vertex and ring inside the last level, every face corner in a sector of its own vertex that holds the face; all-zero arrays give
// the uncreased block, word for word; a negative sharpness and a NaN are refused by face and edge.
// CATMULL-CLARK (mpt_subdiv_topology_cc_of): polygon cages built here as fans -- a quad, a triangle, a
// pentagon, the cube of six quads, a square pyramid, the 5 x 5 grid and the cylinder as quads, the same meshes with every triangle a
// polygon of its own -- at levels 1 to 4, uncreased, every edge inf, and the pattern above with flagged corners, from arrays exactly
// as long as the function may read: counts (V + E + F vertices a level up, n quads per polygon, four per quad, Euler's number), every
// id of every rule inside its level, a face point id naming a face rule of the same launch, a blend's parameter inside (0, 1), the
// table of level-1 quads inside the mesh, every record and emitted corner inside the last level; all-zero arrays give the uncreased
// block; the refusals of the polygons (their sum, an n outside [3, 64], a broken fan, a corner twice) and of a crease by polygon.

#include "../ptina_amd/csrc/subdiv_rule.h"
#include <cstdlib>
#include <limits>
#include <string>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

struct Mesh { std::string name; std::vector<float> v; std::vector<int> f; bool closed; };

// records [3k][8] on the heap, exactly 24 k floats
static std::vector<float> records(const Mesh &m) {
    std::vector<float> rec(m.f.size() * 8, 0.0f);
    for (size_t s = 0; s < m.f.size(); s++) {
        for (int a = 0; a < 3; a++) rec[s * 8 + a] = m.v[(size_t)m.f[s] * 3 + a];
        rec[s * 8 + 5] = 1.0f;
    }
    return rec;
}

static Mesh bipyramid(int n) {
    Mesh m{ "fan" + std::to_string(n), { 0, 0, 1.0f, 0, 0, -0.8f }, {}, true };
    for (int i = 0; i < n; i++) { const double a = 6.283185307179586 * i / n; m.v.insert(m.v.end(), { (float)std::cos(a), (float)std::sin(a), 0.1f * (float)std::cos(3 * a) }); }
    for (int i = 0; i < n; i++) { const int a = 2 + i, b = 2 + (i + 1) % n; m.f.insert(m.f.end(), { 0, a, b, 1, b, a }); }
    return m;
}

static Mesh grid(int nx, int ny) {
    Mesh m{ "grid", {}, {}, false };
    for (int y = 0; y <= ny; y++) for (int x = 0; x <= nx; x++) m.v.insert(m.v.end(), { x - nx / 2.0f, y - ny / 2.0f, 0.15f * (float)std::sin(1.3 * x + 0.7 * y) });
    for (int y = 0; y < ny; y++)
        for (int x = 0; x < nx; x++) {
            const int a = y * (nx + 1) + x, b = a + 1, c = a + nx + 2, d = a + nx + 1;
            m.f.insert(m.f.end(), { a, b, c, a, c, d });
        }
    return m;
}

static Mesh cylinder(int n, int rings) {
    Mesh m{ "cylinder", {}, {}, false };
    for (int r = 0; r < rings; r++) for (int i = 0; i < n; i++) { const double a = 6.283185307179586 * i / n; m.v.insert(m.v.end(), { (float)std::cos(a), (float)std::sin(a), 0.7f * r }); }
    for (int r = 0; r + 1 < rings; r++)
        for (int i = 0; i < n; i++) {
            const int a = r * n + i, b = r * n + (i + 1) % n;
            m.f.insert(m.f.end(), { a, b, b + n, a, b + n, a + n });
        }
    return m;
}

static std::vector<Mesh> fixtures() {
    const float t = 1.618034f;
    std::vector<Mesh> out;
    out.push_back({ "triangle", { 0, 0, 0, 1, 0, 0.25f, 0.25f, 1, 0 }, { 0, 1, 2 }, false });
    out.push_back({ "pair", { 0, 0, 0, 1, 0, 0.25f, 1, 1, 0, -0.0f, 1, 0.5f }, { 0, 1, 2, 0, 2, 3 }, false });
    out.push_back({ "tetrahedron", { 1, 1, 1, 1, -1, -1, -1, 1, -1, -1, -1, 1 }, { 0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2 }, true });
    {
        Mesh m{ "octahedron", { 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1 }, {}, true };
        for (int sx = 0; sx < 2; sx++) for (int sy = 0; sy < 2; sy++) for (int sz = 0; sz < 2; sz++) {
            const int x = sx, y = 2 + sy, z = 4 + sz;
            if ((sx + sy + sz) % 2 == 0) m.f.insert(m.f.end(), { x, y, z }); else m.f.insert(m.f.end(), { x, z, y });
        }
        out.push_back(m);
    }
    out.push_back({ "icosahedron", { -1, t, 0, 1, t, 0, -1, -t, 0, 1, -t, 0, 0, -1, t, 0, 1, t, 0, -1, -t, 0, 1, -t, t, 0, -1, t, 0, 1, -t, 0, -1, -t, 0, 1 },
                    { 0, 11, 5, 0, 5, 1, 0, 1, 7, 0, 7, 10, 0, 10, 11, 1, 5, 9, 5, 11, 4, 11, 10, 2, 10, 7, 6, 7, 1, 8,
                      3, 9, 4, 3, 4, 2, 3, 2, 6, 3, 6, 8, 3, 8, 9, 4, 9, 5, 2, 4, 11, 6, 2, 10, 8, 6, 7, 9, 8, 1 }, true });
    out.push_back(bipyramid(7));
    out.push_back(bipyramid(12));
    out.push_back(grid(5, 5));
    out.push_back(cylinder(8, 3));
    return out;
}

// rules [n] at word `at` of the block: every ring inside the block, every id below `ids`, the kinds those of `edges` or of vertices
static void check_rules(const MptSubdivTopo &t, int32_t at, int64_t n, int64_t nverts, int64_t ids, bool closed) {
    const int64_t W = (int64_t)t.words.size();
    CHECK(at >= 0 && at + 2 * n <= W);
    for (int64_t i = 0; i < n; i++) {
        const int32_t head = t.words[(size_t)(at + 2 * i)], ring = t.words[(size_t)(at + 2 * i + 1)];
        const int kind = head & 3, len = head >> 2;
        CHECK(ring >= 0 && (int64_t)ring + len <= W);
        CHECK(i < nverts ? kind == MPT_SUBDIV_VERT_INT || kind == MPT_SUBDIV_VERT_BND : kind == MPT_SUBDIV_EDGE_INT || kind == MPT_SUBDIV_EDGE_BND);
        if (closed) CHECK(kind == MPT_SUBDIV_VERT_INT || kind == MPT_SUBDIV_EDGE_INT);
        CHECK(kind == MPT_SUBDIV_EDGE_INT ? len == 4 : kind == MPT_SUBDIV_EDGE_BND ? len == 2 : len >= 2);
        for (int k = 0; k < len && (int64_t)ring + len <= W; k++) CHECK(t.words[(size_t)ring + (size_t)k] >= 0 && t.words[(size_t)ring + (size_t)k] < ids);
    }
}

// the rules of a creased mesh: as check_rules, with the variants, their further ids and their parameters
static void check_creased_rules(const MptSubdivTopo &t, int32_t at, int64_t n, int64_t nverts, int64_t ids) {
    const int64_t W = (int64_t)t.words.size();
    CHECK(at >= 0 && at + 2 * n <= W);
    for (int64_t i = 0; i < n; i++) {
        const int32_t head = t.words[(size_t)(at + 2 * i)], ring = t.words[(size_t)(at + 2 * i + 1)];
        const int kind = head & 3, variant = head >> MPT_SUBDIV_VARIANT_SHIFT & 7, len = head >> 2 & MPT_SUBDIV_N_MASK;
        CHECK(head >= 0 && variant <= MPT_SUBDIV_FIXED);
        CHECK(i < nverts ? kind == MPT_SUBDIV_VERT_INT || kind == MPT_SUBDIV_VERT_BND : kind == MPT_SUBDIV_EDGE_INT || kind == MPT_SUBDIV_EDGE_BND);
        const bool vert = kind == MPT_SUBDIV_VERT_INT, edge = kind == MPT_SUBDIV_EDGE_INT;
        CHECK(variant == MPT_SUBDIV_PLAIN || vert || (edge && variant == MPT_SUBDIV_BLEND_EDGE));
        const int more = vert && variant == MPT_SUBDIV_BLEND_CREASE ? 2 : 0;
        const bool blends = (vert && (variant == MPT_SUBDIV_BLEND_CREASE || variant == MPT_SUBDIV_BLEND_CORNER)) || (edge && variant == MPT_SUBDIV_BLEND_EDGE);
        const int64_t words = len + more + (blends ? 2 : 0);
        CHECK(ring >= 0 && (int64_t)ring + words <= W);
        if (ring < 0 || (int64_t)ring + words > W) continue;
        CHECK(vert && variant == MPT_SUBDIV_FIXED ? len == 0 : edge ? len == 4 : len >= 2);
        for (int k = 0; k < len + more; k++) CHECK(t.words[(size_t)ring + (size_t)k] >= 0 && t.words[(size_t)ring + (size_t)k] < ids);
        if (blends) {
            double f;
            std::memcpy(&f, &t.words[(size_t)ring + (size_t)(len + more)], 8);
            CHECK(f > 0.0 && f < 1.0);
        }
    }
}

static void check_creased(const Mesh &m, const std::vector<float> &rec, int levels, const std::vector<float> &crease, const std::vector<uint8_t> &corner, bool hard) {
    const int k = (int)(m.f.size() / 3);
    MptSubdivTopo t, plain;
    char why[64];
    const MptSubdivVerdict v = mpt_subdiv_topology_creased_of(rec.data(), k, levels, crease.data(), corner.empty() ? nullptr : corner.data(), t, why, sizeof why);
    CHECK(v == MPT_SUBDIV_OK && why[0] == 0);
    if (v != MPT_SUBDIV_OK) { std::fprintf(stderr, "%s creased at level %d: %s\n", m.name.c_str(), levels, why); return; }
    CHECK(mpt_subdiv_topology_of(rec.data(), k, levels, plain, nullptr, 0) == MPT_SUBDIV_OK);
    const int64_t V = t.nv[levels], W = (int64_t)t.words.size();
    for (int l = 0; l <= levels; l++) {
        CHECK(t.nv[l] == plain.nv[l] && t.ne[l] == plain.ne[l] && t.nf[l] == plain.nf[l]);
        if (l > 0) check_creased_rules(t, t.rule_at[l], t.nv[l], t.nv[l - 1], t.nv[l - 1]);
    }
    check_rules(t, t.nrule_at, V, V, V, m.closed);
    CHECK(t.srule_at > t.nrule_at && t.nrec >= V && (int64_t)t.srule_at + 3 * t.nrec <= W);
    if (hard && k > 1) CHECK(t.nrec > V);                          // (an interior edge that stays hard splits the vertices on it)
    if (t.srule_at <= 0 || (int64_t)t.srule_at + 3 * t.nrec > W) return;
    check_rules(t, t.srule_at, t.nrec, t.nrec, V, false);
    const int32_t *vert = &t.words[(size_t)t.srule_at + (size_t)t.nrec * 2];
    for (int64_t r = 0; r < t.nrec; r++) CHECK(r < V ? vert[r] == r : vert[r] >= 0 && vert[r] < V);
    CHECK((int64_t)t.face_at + 3 * t.nf[levels] == W);
    const int32_t *pf = &plain.words[(size_t)plain.face_at];
    for (int64_t s = 0; s < 3 * t.nf[levels]; s++) {
        const int32_t r = t.words[(size_t)t.face_at + (size_t)s];
        CHECK(r >= 0 && r < t.nrec);
        if (r < 0 || r >= t.nrec) continue;
        CHECK(vert[r] == pf[s]);                                     // the record is of the corner's own vertex ...
        const int32_t head = t.words[(size_t)t.srule_at + (size_t)r * 2], ring = t.words[(size_t)t.srule_at + (size_t)r * 2 + 1];
        const int len = head >> 2, faces = (head & 3) == MPT_SUBDIV_VERT_BND ? len - 1 : len;
        const int32_t a = pf[s - s % 3 + (s + 1) % 3], b = pf[s - s % 3 + (s + 2) % 3];
        bool held = false;                                            // ... and its sector holds the face (v, a, b)
        for (int i = 0; i < faces && !held; i++) held = t.words[(size_t)ring + (size_t)i] == a && t.words[(size_t)ring + (size_t)((i + 1) % len)] == b;
        CHECK(held);
    }
}

static MptSubdivVerdict crease_refusal(const std::vector<float> &rec, const std::vector<float> &crease, const char *words) {
    MptSubdivTopo t;
    const int k = (int)(rec.size() / 24);
    const MptSubdivVerdict want = mpt_subdiv_topology_creased_of(rec.data(), k, 2, crease.data(), nullptr, t, nullptr, 0);
    for (size_t cap = 0; cap <= 240; cap += cap < 8 ? 1 : 29) {
        std::vector<char> why(cap, 'x');
        CHECK(mpt_subdiv_topology_creased_of(rec.data(), k, 2, crease.data(), nullptr, t, cap ? why.data() : nullptr, cap) == want);
        if (!cap) continue;
        CHECK(std::memchr(why.data(), 0, cap) != nullptr);
        if (cap >= 200) CHECK(!std::strncmp(why.data(), "subdivision: ", 13) && std::strstr(why.data(), words) != nullptr);
    }
    return want;
}

static MptSubdivVerdict refusal(const std::vector<float> &rec, int levels, const char *words) {
    MptSubdivTopo t;
    const int k = (int)(rec.size() / 24);
    const MptSubdivVerdict want = mpt_subdiv_topology_of(rec.data(), k, levels, t, nullptr, 0);
    CHECK(mpt_subdiv_topology_of(rec.data(), k, levels, t, nullptr, 64) == want);
    for (size_t cap = 0; cap <= 240; cap += cap < 8 ? 1 : 29) {
        std::vector<char> why(cap, 'x');
        CHECK(mpt_subdiv_topology_of(rec.data(), k, levels, t, cap ? why.data() : nullptr, cap) == want);
        if (!cap) continue;
        CHECK(std::memchr(why.data(), 0, cap) != nullptr);
        if (want == MPT_SUBDIV_OK) CHECK(why[0] == 0);
        else if (cap >= 200) CHECK(!std::strncmp(why.data(), "subdivision: ", 13) && std::strstr(why.data(), words) != nullptr);
    }
    return want;
}

static std::vector<float> soup(std::initializer_list<int> pts) {       // triangles over the points A..F below, a corner per entry
    static const float P[6][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 }, { 1, 1, 1 }, { 2, 0, 1 } };
    std::vector<float> rec(pts.size() * 8, 0.0f);
    size_t s = 0;
    for (int p : pts) { for (int a = 0; a < 3; a++) rec[s * 8 + a] = P[p][a]; s++; }
    return rec;
}

// ---------------------------------------------------------------- Catmull-Clark
struct Cage { std::string name; std::vector<float> v; std::vector<std::vector<int>> polys; int euler; };

// the fan-ordered records of a cage, exactly 24 k floats, and its polygon sizes
static std::vector<float> fan_records(const Cage &c, std::vector<int32_t> &polys) {
    std::vector<float> rec;
    polys.clear();
    for (const auto &p : c.polys) {
        polys.push_back((int32_t)p.size());
        for (size_t i = 0; i + 2 < p.size(); i++)
            for (int corner : { p[0], p[i + 1], p[i + 2] }) {
                for (int a = 0; a < 3; a++) rec.push_back(c.v[(size_t)corner * 3 + (size_t)a]);
                rec.insert(rec.end(), { 0.0f, 0.0f, 1.0f, 0.0f, 0.0f });
            }
    }
    return rec;
}

static Cage quads_of(const Mesh &m, const char *name, int euler) {      // the quads of a mesh built of pairs (a b c), (a c d)
    Cage c{ name, m.v, {}, euler };
    for (size_t f = 0; f + 5 < m.f.size() + 1; f += 6) c.polys.push_back({ m.f[f], m.f[f + 1], m.f[f + 2], m.f[f + 5] });
    return c;
}

static std::vector<Cage> cages() {
    std::vector<Cage> out;
    out.push_back({ "quad", { 0, 0, 0, 1, 0, 0.25f, 1, 1, 0, -0.0f, 1, 0.5f }, { { 0, 1, 2, 3 } }, 1 });
    out.push_back({ "triangle", { 0, 0, 0, 1, 0, 0.25f, 0.25f, 1, 0 }, { { 0, 1, 2 } }, 1 });
    out.push_back({ "pentagon", { 1, 0, 0.1f, 0.31f, 0.95f, -0.08f, -0.81f, 0.59f, 0.03f, -0.81f, -0.59f, 0.03f, 0.31f, -0.95f, -0.08f }, { { 0, 1, 2, 3, 4 } }, 1 });
    out.push_back({ "cube", { -1, -1, -1, 1, -1, -1, -1, 1, -1, 1, 1, -1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1 },
                    { { 0, 2, 3, 1 }, { 4, 5, 7, 6 }, { 0, 1, 5, 4 }, { 2, 6, 7, 3 }, { 0, 4, 6, 2 }, { 1, 3, 7, 5 } }, 2 });
    out.push_back({ "pyramid", { -1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0, 0.1f, 0, 1.5f }, { { 0, 1, 4 }, { 1, 2, 4 }, { 2, 3, 4 }, { 3, 0, 4 }, { 3, 2, 1, 0 } }, 2 });
    out.push_back(quads_of(grid(5, 5), "grid", 1));
    out.push_back(quads_of(cylinder(8, 3), "cylinder", 0));
    return out;
}

// the rules of one Catmull-Clark launch: nv vertices, ne edges, nf faces of the level below, ids below nv; a face point id names a face's rule
static void check_cc_rules(const MptSubdivTopoCC &t, int32_t at, int64_t nv, int64_t ne, int64_t nf) {
    const int64_t W = (int64_t)t.words.size(), n = nv + ne + nf;
    CHECK(at >= 0 && at + 2 * n <= W);
    if (at < 0 || at + 2 * n > W) return;
    for (int64_t i = 0; i < n; i++) {
        const int32_t head = t.words[(size_t)(at + 2 * i)], ring = t.words[(size_t)(at + 2 * i + 1)];
        const int kind = head & 3, variant = head >> MPT_SUBDIV_VARIANT_SHIFT & 7, len = head >> 2 & MPT_SUBDIV_N_MASK;
        const bool cc = (variant & MPT_SUBDIV_CC) != 0;
        const int blend = variant & 3;
        CHECK(head >= 0);
        const bool vert = i < nv, edge = !vert && i < nv + ne, face = !vert && !edge;
        int64_t ids = len, fids = 0, more = 0;
        bool blends = false;
        if (face) CHECK(cc && kind == MPT_SUBDIV_EDGE_BND && blend == 0 && len >= 3 && len <= MPT_SUBDIV_MAX_CORNERS);
        else if (edge && cc) { CHECK(kind == MPT_SUBDIV_EDGE_INT && len == 4 && blend <= MPT_SUBDIV_BLEND_EDGE); ids = 2; fids = 2; blends = blend == MPT_SUBDIV_BLEND_EDGE; }
        else if (edge) CHECK(kind == MPT_SUBDIV_EDGE_BND && variant == 0 && len == 2);
        else if (cc) {
            CHECK(kind == MPT_SUBDIV_VERT_INT && len >= 2 && blend != MPT_SUBDIV_FIXED);
            fids = len; more = blend == MPT_SUBDIV_BLEND_CREASE ? 2 : 0; blends = blend != 0;
        } else CHECK((kind == MPT_SUBDIV_VERT_BND && variant == 0 && len >= 2) || (kind == MPT_SUBDIV_VERT_INT && variant == MPT_SUBDIV_FIXED && len == 0));
        const int64_t words = ids + fids + more + (blends ? 2 : 0);
        CHECK(ring >= 0 && (int64_t)ring + words <= W);
        if (ring < 0 || (int64_t)ring + words > W) continue;
        const int32_t *w = &t.words[(size_t)ring];
        for (int64_t k = 0; k < ids; k++) CHECK(w[k] >= 0 && w[k] < nv);
        for (int64_t k = ids; k < ids + fids; k++) CHECK(w[k] >= nv + ne && w[k] < n);
        for (int64_t k = ids + fids; k < ids + fids + more; k++) CHECK(w[k] >= 0 && w[k] < nv);
        if (blends) {
            double f;
            std::memcpy(&f, w + ids + fids + more, 8);
            CHECK(f > 0.0 && f < 1.0);
        }
    }
}

static bool check_cc(const Cage &c, const std::vector<float> &rec, const std::vector<int32_t> &polys, bool as_triangles, int levels, const float *crease,
                     const uint8_t *corner, bool creased) {
    const int k = (int)(rec.size() / 24), m = as_triangles ? k : (int)polys.size();
    MptSubdivTopoCC t;
    char why[64];
    const MptSubdivVerdict v = mpt_subdiv_topology_cc_of(rec.data(), k, levels, as_triangles ? nullptr : polys.data(), as_triangles ? -7 : m, crease, corner, t, why, sizeof why);
    CHECK(v == MPT_SUBDIV_OK && why[0] == 0);
    if (v != MPT_SUBDIV_OK) { std::fprintf(stderr, "%s at level %d: %s\n", c.name.c_str(), levels, why); return false; }
    int64_t corners = 0;
    for (int j = 0; j < m; j++) corners += as_triangles ? 3 : polys[(size_t)j];
    const int64_t W = (int64_t)t.words.size(), V = t.nv[levels], Q = t.nf[levels];
    CHECK(t.levels == levels && t.nv[0] == (int64_t)(c.v.size() / 3) && t.nf[0] == m);
    for (int64_t i = 0; i < t.nv[0]; i++) CHECK(t.words[(size_t)i] >= 0 && t.words[(size_t)i] < 3 * k);
    for (int l = 0; l <= levels; l++) {
        CHECK(t.nv[l] - t.ne[l] + t.nf[l] == c.euler);
        if (l > 0) {
            CHECK(t.nf[l] == corners << (2 * (l - 1)) && t.nv[l] == t.nv[l - 1] + t.ne[l - 1] + t.nf[l - 1]);
            check_cc_rules(t, t.rule_at[l], t.nv[l - 1], t.ne[l - 1], t.nf[l - 1]);
        }
    }
    check_rules(t, t.nrule_at, V, V, V, c.euler == 2);
    CHECK(creased ? t.srule_at > t.nrule_at && t.nrec >= V : t.srule_at == 0 && t.nrec == V);
    const int32_t *vert = nullptr;
    if (t.srule_at > 0) {
        CHECK((int64_t)t.srule_at + 3 * t.nrec <= W);
        if ((int64_t)t.srule_at + 3 * t.nrec > W) return false;
        check_rules(t, t.srule_at, t.nrec, t.nrec, V, false);
        vert = &t.words[(size_t)t.srule_at + (size_t)t.nrec * 2];
        for (int64_t r = 0; r < t.nrec; r++) CHECK(r < V ? vert[r] == r : vert[r] >= 0 && vert[r] < V);
    }
    CHECK(t.nquads1 == corners && t.quad_at > 0 && (int64_t)t.quad_at + 2 * corners == t.face_at && (int64_t)t.face_at + 6 * Q == W);
    if ((int64_t)t.quad_at + 2 * corners != t.face_at || (int64_t)t.face_at + 6 * Q != W) return false;
    for (int64_t q = 0; q < corners; q++) {
        const int32_t first = t.words[(size_t)t.quad_at + (size_t)q * 2], ni = t.words[(size_t)t.quad_at + (size_t)q * 2 + 1], n = ni & 255, i = ni >> 8;
        CHECK(n >= 3 && n <= MPT_SUBDIV_MAX_CORNERS && i >= 0 && i < n && first >= 0 && (int64_t)first + n - 2 <= k);
    }
    for (int64_t g = 0; g < 2 * Q; g += 2) {                            // the halves of a quad: (r0, r1, r2), (r0, r2, r3)
        const int32_t *f = &t.words[(size_t)t.face_at + (size_t)g * 3];
        for (int s = 0; s < 6; s++) CHECK(f[s] >= 0 && f[s] < t.nrec);
        CHECK(f[3] == f[0] && f[4] == f[2]);
        if (vert && f[0] >= 0 && f[0] < t.nrec && f[1] >= 0 && f[1] < t.nrec) CHECK(vert[f[0]] != vert[f[1]]);
    }
    return true;
}

static MptSubdivVerdict cc_refusal(const std::vector<float> &rec, int levels, const std::vector<int32_t> &polys, const std::vector<float> &crease, const char *words) {
    MptSubdivTopoCC t;
    const int k = (int)(rec.size() / 24);
    const float *cr = crease.empty() ? nullptr : crease.data();
    const MptSubdivVerdict want = mpt_subdiv_topology_cc_of(rec.data(), k, levels, polys.data(), (int)polys.size(), cr, nullptr, t, nullptr, 0);
    for (size_t cap = 0; cap <= 240; cap += cap < 8 ? 1 : 29) {
        std::vector<char> why(cap, 'x');
        CHECK(mpt_subdiv_topology_cc_of(rec.data(), k, levels, polys.data(), (int)polys.size(), cr, nullptr, t, cap ? why.data() : nullptr, cap) == want);
        if (!cap) continue;
        CHECK(std::memchr(why.data(), 0, cap) != nullptr);
        if (want == MPT_SUBDIV_OK) CHECK(why[0] == 0);
        else if (cap >= 200) CHECK(!std::strncmp(why.data(), "subdivision: ", 13) && std::strstr(why.data(), words) != nullptr);
    }
    return want;
}

int main() {
    int topologies = 0;
    for (const Mesh &m : fixtures()) {
        const std::vector<float> rec = records(m);
        const int k = (int)(m.f.size() / 3);
        for (int levels = 1; levels <= 4; levels++) {
            MptSubdivTopo t;
            char why[64];
            const MptSubdivVerdict v = mpt_subdiv_topology_of(rec.data(), k, levels, t, why, sizeof why);
            CHECK(v == MPT_SUBDIV_OK && why[0] == 0);
            if (v != MPT_SUBDIV_OK) { std::fprintf(stderr, "%s at level %d: %s\n", m.name.c_str(), levels, why); continue; }
            topologies++;
            CHECK(t.levels == levels && t.nv[0] == (int64_t)(m.v.size() / 3));
            for (int64_t c = 0; c < t.nv[0]; c++) CHECK(t.words[(size_t)c] >= 0 && t.words[(size_t)c] < 3 * k);
            for (int l = 0; l <= levels; l++) {
                CHECK(t.nf[l] == ((int64_t)k << (2 * l)));
                if (m.closed) CHECK(t.nv[l] - t.ne[l] + t.nf[l] == 2);
                if (l > 0) { CHECK(t.nv[l] == t.nv[l - 1] + t.ne[l - 1]); check_rules(t, t.rule_at[l], t.nv[l], t.nv[l - 1], t.nv[l - 1], m.closed); }
            }
            check_rules(t, t.nrule_at, t.nv[levels], t.nv[levels], t.nv[levels], m.closed);
            CHECK((int64_t)t.face_at + 3 * t.nf[levels] == (int64_t)t.words.size());
            for (int64_t s = 0; s < 3 * t.nf[levels]; s++) CHECK(t.words[(size_t)t.face_at + (size_t)s] >= 0 && t.words[(size_t)t.face_at + (size_t)s] < t.nv[levels]);
        }
    }
    int creased = 0;
    for (const Mesh &m : fixtures()) {
        const std::vector<float> rec = records(m);
        const size_t n = m.f.size();                                  // 3 k: one sharpness per face edge, one flag per face corner
        const float inf = std::numeric_limits<float>::infinity();
        static const float some[7] = { 0.0f, 0.25f, 0.5f, 1.0f, 1.5f, 2.5f, inf };
        std::vector<float> every(n, inf), pattern(n), zero(n, 0.0f);
        std::vector<uint8_t> flags(n, 0), none(n, 0);
        for (size_t s = 0; s < n; s++) { pattern[s] = some[(s * 5 + s / 3) % 7]; flags[s] = s % 7 == 3; }
        for (int levels = 1; levels <= 4; levels++) {
            check_creased(m, rec, levels, every, {}, true); creased++;
            check_creased(m, rec, levels, pattern, flags, false); creased++;
            MptSubdivTopo plain, t;
            CHECK(mpt_subdiv_topology_of(rec.data(), (int)(n / 3), levels, plain, nullptr, 0) == MPT_SUBDIV_OK);
            CHECK(mpt_subdiv_topology_creased_of(rec.data(), (int)(n / 3), levels, zero.data(), none.data(), t, nullptr, 0) == MPT_SUBDIV_OK);
            CHECK(t.words == plain.words && t.srule_at == 0 && t.nrec == plain.nv[levels] && t.nrule_at == plain.nrule_at && t.face_at == plain.face_at);
        }
    }
    {   // k = 0 is a mesh and stays one
        MptSubdivTopo t;
        CHECK(mpt_subdiv_topology_of(nullptr, 0, 3, t, nullptr, 0) == MPT_SUBDIV_OK && t.words.empty() && t.nf[3] == 0);
    }

    int refusals = 0;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    {
        std::vector<float> rec = soup({ 0, 1, 2, 0, 2, 4 });
        CHECK(refusal(rec, 2, "") == MPT_SUBDIV_OK);
        for (float bad : { inf, -inf, nan })
            for (size_t where : { (size_t)0, rec.size() - 8 + 2 }) {             // the first and the last position read
                std::vector<float> r = rec;
                r[where] = bad;
                CHECK(refusal(r, 2, "is not finite") == MPT_SUBDIV_NOT_FINITE); refusals++;
            }
        rec[rec.size() - 1] = nan; rec[3] = inf;                                 // normals and texcoords are not read
        CHECK(refusal(rec, 2, "") == MPT_SUBDIV_OK);
    }
    CHECK(refusal(soup({ 0, 1, 2, 0, 3, 0 }), 2, "face 1 has two corners on one vertex") == MPT_SUBDIV_DEGENERATE); refusals++;
    CHECK(refusal(soup({ 0, 1, 2, 1, 0, 3, 0, 1, 4 }), 2, "face 2 is the third on the edge") == MPT_SUBDIV_EDGE_FACES); refusals++;
    CHECK(refusal(soup({ 0, 1, 2, 0, 1, 3 }), 2, "same direction") == MPT_SUBDIV_EDGE_DIRECTION); refusals++;
    CHECK(refusal(soup({ 0, 1, 2, 0, 3, 4 }), 2, "of vertex 0 are not one fan") == MPT_SUBDIV_FAN); refusals++;
    CHECK(refusal(soup({ 0, 1, 2, 0, 2, 1, 0, 3, 4, 0, 4, 3 }), 1, "not one fan") == MPT_SUBDIV_FAN); refusals++;   // two closed fans on one vertex
    CHECK(refusal(soup({ 0, 1, 2 }), 0, "levels 0 outside [1, 5]") == MPT_SUBDIV_LEVELS); refusals++;
    CHECK(refusal(soup({ 0, 1, 2 }), 6, "levels 6 outside") == MPT_SUBDIV_LEVELS); refusals++;
    {
        const std::vector<float> rec = soup({ 0, 1, 2, 0, 2, 4 });
        for (size_t where : { (size_t)0, (size_t)5 }) {                          // the first and the last sharpness read
            std::vector<float> crease(6, 0.5f);
            const std::string edge = "the crease of edge " + std::to_string(where % 3) + " of face " + std::to_string(where / 3);
            crease[where] = -0.25f;
            CHECK(crease_refusal(rec, crease, (edge + " is negative").c_str()) == MPT_SUBDIV_CREASE); refusals++;
            crease[where] = -inf;
            CHECK(crease_refusal(rec, crease, (edge + " is negative").c_str()) == MPT_SUBDIV_CREASE); refusals++;
            crease[where] = nan;
            CHECK(crease_refusal(rec, crease, (edge + " is not a number").c_str()) == MPT_SUBDIV_CREASE); refusals++;
        }
        MptSubdivTopo t;
        CHECK(mpt_subdiv_topology_creased_of(nullptr, 0, 2, nullptr, nullptr, t, nullptr, 0) == MPT_SUBDIV_OK && t.words.empty());
    }
    {
        MptSubdivTopo t;
        CHECK(mpt_subdiv_topology_of(nullptr, 1, 1, t, nullptr, 0) == MPT_SUBDIV_ARGS);
        CHECK(mpt_subdiv_topology_of(nullptr, -1, 1, t, nullptr, 0) == MPT_SUBDIV_ARGS);
        const float one[24] = {};
        CHECK(mpt_subdiv_topology_of(one, 20000, 5, t, nullptr, 0) == MPT_SUBDIV_TOO_MANY);      // refused before anything is read
    }

    // ---------------------------------------------------------------- Catmull-Clark
    int cc_topologies = 0, cc_creased = 0, cc_refusals = 0;
    for (const Cage &c : cages()) {
        std::vector<int32_t> polys;
        const std::vector<float> rec = fan_records(c, polys);
        for (int as_triangles = 0; as_triangles < 2; as_triangles++) {
            if (as_triangles && (c.name == "triangle" || c.name == "cube")) continue;
            const size_t n = as_triangles ? rec.size() / 8 : [&] { size_t s = 0; for (int32_t p : polys) s += (size_t)p; return s; }();
            static const float some[7] = { 0.0f, 0.25f, 0.5f, 1.0f, 1.5f, 2.5f, inf };
            std::vector<float> every(n, inf), pattern(n), zero(n, 0.0f);
            std::vector<uint8_t> flags(n, 0), none(n, 0);
            for (size_t s = 0; s < n; s++) { pattern[s] = some[(s * 5 + s / 3) % 7]; flags[s] = s % 7 == 3; }
            for (int levels = 1; levels <= 4; levels++) {
                cc_topologies += check_cc(c, rec, polys, as_triangles != 0, levels, nullptr, nullptr, false);
                cc_creased += check_cc(c, rec, polys, as_triangles != 0, levels, every.data(), nullptr, true);
                cc_creased += check_cc(c, rec, polys, as_triangles != 0, levels, pattern.data(), flags.data(), true);
                MptSubdivTopoCC plain, t;
                const int k = (int)(rec.size() / 24);
                const int32_t *po = as_triangles ? nullptr : polys.data();
                CHECK(mpt_subdiv_topology_cc_of(rec.data(), k, levels, po, (int)polys.size(), nullptr, nullptr, plain, nullptr, 0) == MPT_SUBDIV_OK);
                CHECK(mpt_subdiv_topology_cc_of(rec.data(), k, levels, po, (int)polys.size(), zero.data(), none.data(), t, nullptr, 0) == MPT_SUBDIV_OK);
                CHECK(t.words == plain.words && t.srule_at == 0 && t.quad_at == plain.quad_at && t.face_at == plain.face_at);
            }
        }
    }
    {
        const Cage two{ "two", { 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0.5f, 2, 0, 0, 2, 1, 0 }, { { 0, 1, 2, 3 }, { 1, 4, 5, 2 } }, 1 };
        std::vector<int32_t> polys;
        const std::vector<float> rec = fan_records(two, polys);
        CHECK(cc_refusal(rec, 2, polys, {}, "") == MPT_SUBDIV_OK);
        CHECK(cc_refusal(rec, 2, { 4, 5 }, {}, "the polygons hold 5 triangles, the mesh has 4") == MPT_SUBDIV_POLYS); cc_refusals++;
        CHECK(cc_refusal(rec, 2, { 4 }, {}, "the polygons hold 2 triangles, the mesh has 4") == MPT_SUBDIV_POLYS); cc_refusals++;
        CHECK(cc_refusal(rec, 2, { 4, 2, 4 }, {}, "polygon 1 has 2 corners, outside [3, 64]") == MPT_SUBDIV_POLYS); cc_refusals++;
        CHECK(cc_refusal(rec, 2, { 65, 4 }, {}, "polygon 0 has 65 corners") == MPT_SUBDIV_POLYS); cc_refusals++;
        CHECK(cc_refusal(rec, 2, { -1 }, {}, "polygon 0 has -1 corners") == MPT_SUBDIV_POLYS); cc_refusals++;
        CHECK(cc_refusal(rec, 2, { 6 }, {}, "face 2 does not continue the fan of polygon 0") == MPT_SUBDIV_POLYS); cc_refusals++;
        CHECK(cc_refusal(rec, 2, { 3, 4, 3 }, {}, "face 2 does not continue the fan of polygon 1") == MPT_SUBDIV_POLYS); cc_refusals++;
        CHECK(cc_refusal(rec, 0, polys, {}, "levels 0 outside [1, 5]") == MPT_SUBDIV_LEVELS); cc_refusals++;
        CHECK(cc_refusal(rec, 6, polys, {}, "levels 6 outside") == MPT_SUBDIV_LEVELS); cc_refusals++;
        for (size_t where : { (size_t)0, (size_t)7 }) {                         // the first and the last sharpness read
            std::vector<float> crease(8, 0.5f);
            const std::string edge = "the crease of edge " + std::to_string(where % 4) + " of polygon " + std::to_string(where / 4);
            crease[where] = -0.25f;
            CHECK(cc_refusal(rec, 2, polys, crease, (edge + " is negative").c_str()) == MPT_SUBDIV_CREASE); cc_refusals++;
            crease[where] = nan;
            CHECK(cc_refusal(rec, 2, polys, crease, (edge + " is not a number").c_str()) == MPT_SUBDIV_CREASE); cc_refusals++;
        }
        std::vector<float> bad = rec;
        bad[bad.size() - 8 + 2] = inf;
        CHECK(cc_refusal(bad, 2, polys, {}, "corner 2 of face 3 is not finite") == MPT_SUBDIV_NOT_FINITE); cc_refusals++;
        // a quad whose fan runs (a b c), (a c b): corners a b c b
        const std::vector<float> twice = soup({ 0, 1, 2, 0, 2, 1 });
        CHECK(cc_refusal(twice, 2, { 4 }, {}, "polygon 0 has two corners on one vertex (vertex 1)") == MPT_SUBDIV_DEGENERATE); cc_refusals++;
        // readobj's split of a quad, (0 1 2), (2 3 0), is not the fan
        CHECK(cc_refusal(soup({ 0, 1, 4, 4, 2, 0 }), 2, { 4 }, {}, "face 1 does not continue the fan of polygon 0") == MPT_SUBDIV_POLYS); cc_refusals++;
        CHECK(cc_refusal(soup({ 0, 1, 2, 0, 1, 3 }), 2, { 3, 3 }, {}, "same direction") == MPT_SUBDIV_EDGE_DIRECTION); cc_refusals++;
        CHECK(cc_refusal(soup({ 0, 1, 2, 1, 0, 3, 0, 1, 4 }), 2, { 3, 3, 3 }, {}, "face 2 is the third on the edge") == MPT_SUBDIV_EDGE_FACES); cc_refusals++;
        CHECK(cc_refusal(soup({ 0, 1, 2, 0, 3, 4 }), 2, { 3, 3 }, {}, "of vertex 0 are not one fan") == MPT_SUBDIV_FAN); cc_refusals++;
        MptSubdivTopoCC t;
        CHECK(mpt_subdiv_topology_cc_of(nullptr, 0, 2, nullptr, 0, nullptr, nullptr, t, nullptr, 0) == MPT_SUBDIV_OK && t.nf[2] == 0);
        CHECK(mpt_subdiv_topology_cc_of(nullptr, 1, 1, nullptr, 0, nullptr, nullptr, t, nullptr, 0) == MPT_SUBDIV_ARGS);
        const float one[24] = {};
        std::vector<int32_t> many(40000, 3);
        CHECK(mpt_subdiv_topology_cc_of(one, 40000, 5, many.data(), 40000, nullptr, nullptr, t, nullptr, 0) == MPT_SUBDIV_TOO_MANY);   // refused before a position is read
    }

    std::printf("subdiv_rule_check: %d topologies, %d creased, %d refusals, %d failures\n", topologies, creased, refusals, failures);
    std::printf("subdiv_rule_check: Catmull-Clark: %d topologies, %d creased, %d refusals\n", cc_topologies, cc_creased, cc_refusals);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

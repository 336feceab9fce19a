// displace_rule_check.cpp -- the pure host piece of texture displacement (ptina_amd/csrc/displace_rule.h: the first-corner table of a
// level's vertices and the admission check of a mesh's corner uvs) exercised by a stand-alone program, so that it can run under the
// host sanitizers without a GPU and without loading anything into an interpreter:
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/displace_rule_check.cpp -o displace_rule_check && ./displace_rule_check
//
// The first-corner table of the last level of procedural meshes (a tetrahedron, closed fans of valence 7 and 12, the open 5 x 5
// grid) at levels 1 to 4, the face tables subdiv_rule.h's, from arrays on the heap that are exactly as long as the function may read
// and write: every entry names its vertex and no corner before it does; both refusals and the arguments that name no table.  The uv
// check over records exactly 24 k floats long: the bounds on both sides, every value that is not a number, the corner named, with
// message buffers of every size (cut, terminated, never overrun).

#include "../ptina_amd/csrc/subdiv_rule.h"
#include "../ptina_amd/csrc/displace_rule.h"
#include <cstdlib>
#include <limits>
#include <string>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

struct Mesh { std::string name; std::vector<float> v; std::vector<int> f; };

static std::vector<float> records(const Mesh &m) {
    std::vector<float> rec(m.f.size() * 8, 0.0f);
    for (size_t s = 0; s < m.f.size(); s++) {
        for (int a = 0; a < 3; a++) rec[s * 8 + a] = m.v[(size_t)m.f[s] * 3 + a];
        rec[s * 8 + 5] = 1.0f;
        rec[s * 8 + 6] = 0.25f * m.v[(size_t)m.f[s] * 3] + 0.5f; rec[s * 8 + 7] = 0.25f * m.v[(size_t)m.f[s] * 3 + 1] + 0.5f;
    }
    return rec;
}

static Mesh bipyramid(int n) {
    Mesh m{ "fan" + std::to_string(n), { 0, 0, 1.0f, 0, 0, -0.8f }, {} };
    for (int i = 0; i < n; i++) { const double a = 6.283185307179586 * i / n; m.v.insert(m.v.end(), { (float)std::cos(a), (float)std::sin(a), 0.1f * (float)std::cos(3 * a) }); }
    for (int i = 0; i < n; i++) { const int a = 2 + i, b = 2 + (i + 1) % n; m.f.insert(m.f.end(), { 0, a, b, 1, b, a }); }
    return m;
}

static Mesh grid(int nx, int ny) {
    Mesh m{ "grid", {}, {} };
    for (int y = 0; y <= ny; y++) for (int x = 0; x <= nx; x++) m.v.insert(m.v.end(), { x - nx / 2.0f, y - ny / 2.0f, 0.15f * (float)std::sin(1.3 * x + 0.7 * y) });
    for (int y = 0; y < ny; y++)
        for (int x = 0; x < nx; x++) {
            const int a = y * (nx + 1) + x, b = a + 1, c = a + nx + 2, d = a + nx + 1;
            m.f.insert(m.f.end(), { a, b, c, a, c, d });
        }
    return m;
}

static int uv_refusal(const std::vector<float> &rec, const char *words) {
    const int64_t k = (int64_t)(rec.size() / 24);
    const int want = mpt_displace_uv_check_of(rec.data(), k, nullptr, 0);
    for (size_t cap = 0; cap <= 240; cap += cap < 8 ? 1 : 29) {
        std::vector<char> why(cap, 'x');
        CHECK(mpt_displace_uv_check_of(rec.data(), k, cap ? why.data() : nullptr, cap) == want);
        if (!cap) continue;
        CHECK(std::memchr(why.data(), 0, cap) != nullptr);
        if (want == 0) CHECK(why[0] == 0);
        else if (cap >= 200) CHECK(!std::strncmp(why.data(), "displacement: ", 14) && std::strstr(why.data(), words) != nullptr);
    }
    return want;
}

int main() {
    int tables = 0, refusals = 0;
    std::vector<Mesh> meshes;
    meshes.push_back({ "tetrahedron", { 1, 1, 1, 1, -1, -1, -1, 1, -1, -1, -1, 1 }, { 0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2 } });
    meshes.push_back(bipyramid(7));
    meshes.push_back(bipyramid(12));
    meshes.push_back(grid(5, 5));
    for (const Mesh &m : meshes) {
        const std::vector<float> rec = records(m);
        const int k = (int)(m.f.size() / 3);
        CHECK(uv_refusal(rec, "") == 0);
        for (int levels = 1; levels <= 4; levels++) {
            MptSubdivTopo t;
            if (mpt_subdiv_topology_of(rec.data(), k, levels, t, nullptr, 0) != MPT_SUBDIV_OK) { CHECK(!"the topology"); continue; }
            const int64_t nf = t.nf[levels], nv = t.nv[levels];
            const std::vector<int32_t> faces(t.words.begin() + t.face_at, t.words.begin() + t.face_at + 3 * nf);      // exactly 3 nf words
            std::vector<int32_t> corner((size_t)nv, -7);                                                              // exactly nv words
            CHECK(mpt_displace_corners_of(faces.data(), nf, (int32_t)nv, corner.data()) == 0);
            tables++;
            std::vector<int32_t> first((size_t)nv, -1);
            for (int64_t s = 0; s < 3 * nf; s++)
                if (first[(size_t)faces[(size_t)s]] < 0) first[(size_t)faces[(size_t)s]] = (int32_t)s;
            CHECK(corner == first);
            for (int64_t v = 0; v < nv; v++) CHECK(corner[(size_t)v] >= 0 && corner[(size_t)v] < 3 * nf && faces[(size_t)corner[(size_t)v]] == v);
            // an id out of range, on either side, at the first and at the last corner
            for (int32_t bad : { (int32_t)nv, (int32_t)-1, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min() })
                for (size_t where : { (size_t)0, faces.size() - 1 }) {
                    std::vector<int32_t> f = faces;
                    f[where] = bad;
                    CHECK(mpt_displace_corners_of(f.data(), nf, (int32_t)nv, corner.data()) == 2 && corner[0] == (int32_t)where); refusals++;
                }
            // a vertex no face touches: one more vertex than the faces name
            std::vector<int32_t> more((size_t)nv + 1);
            CHECK(mpt_displace_corners_of(faces.data(), nf, (int32_t)nv + 1, more.data()) == 3 && more[0] == (int32_t)nv); refusals++;
        }
    }
    {   // arguments that name no table; nothing is a table
        int32_t one[3] = { 0, 0, 0 }, c = 0;
        CHECK(mpt_displace_corners_of(nullptr, 0, 0, nullptr) == 0);
        CHECK(mpt_displace_corners_of(nullptr, 1, 1, &c) == 1);
        CHECK(mpt_displace_corners_of(one, 1, 1, nullptr) == 1);
        CHECK(mpt_displace_corners_of(one, -1, 1, &c) == 1);
        CHECK(mpt_displace_corners_of(one, 1, -1, &c) == 1);
        CHECK(mpt_displace_corners_of(one, (int64_t)1 << 40, 1, &c) == 1);                       // refused before anything is read
        CHECK(mpt_displace_corners_of(one, 1, 1, &c) == 0 && c == 0);
        CHECK(mpt_displace_corners_of(nullptr, 0, 1, &c) == 3);
    }
    {   // the uv check: the bound holds on both sides, the corner is named, positions and normals are not read
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        std::vector<float> rec = records(meshes[0]);
        for (float ok : { 1048576.0f, -1048576.0f, 0.0f, -0.0f, 1e-40f })
            for (size_t where : { (size_t)6, rec.size() - 1 }) {
                std::vector<float> r = rec;
                r[where] = ok;
                CHECK(uv_refusal(r, "") == 0);
            }
        for (float bad : { inf, -inf, nan, 1048577.0f, -1048577.0f, std::numeric_limits<float>::max() }) {
            std::vector<float> r = rec;
            r[6] = bad;
            CHECK(uv_refusal(r, "the uv of corner 0 of face 0 is not finite or exceeds 2^20") == 1); refusals++;
            r = rec;
            r[rec.size() - 1] = bad;                                                       // the last value read
            CHECK(uv_refusal(r, "the uv of corner 2 of face 3 is not finite or exceeds 2^20") == 1); refusals++;
        }
        rec[0] = nan; rec[4] = inf; rec[rec.size() - 3] = nan;
        CHECK(uv_refusal(rec, "") == 0);
        CHECK(mpt_displace_uv_check_of(nullptr, 0, nullptr, 0) == 0);
        CHECK(mpt_displace_uv_check_of(nullptr, 1, nullptr, 0) == 1);
        CHECK(mpt_displace_uv_check_of(rec.data(), -1, nullptr, 0) == 1);
    }
    std::printf("displace_rule_check: %d tables, %d refusals, %d failures\n", tables, refusals, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

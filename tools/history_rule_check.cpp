// history_rule_check.cpp -- the pure pieces of the film's reprojection (ptina_amd/csrc/history_rule.h: the refusal rule, the
// projection into the kept view and the arithmetic of one resampled pixel) exercised by a stand-alone program, so that they can
// run under the host sanitizers without a GPU and without loading anything into an interpreter:
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/history_rule_check.cpp -o history_rule_check && ./history_rule_check
//
// Every verdict with message buffers of every size from none to ample (the words must be cut, terminated and never written past
// the buffer); the resampled pixel over films whose arrays are exactly nx * ny elements of the heap -- a tap read outside the film
// is the sanitizer's to report -- with motion records at, across and far beyond the film's edges, NaNs and infinities among them.

#include "../ptina_amd/csrc/history_rule.h"
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

struct V4 { float x, y, z, w; };
static bool same_bits(const V4 &a, const V4 &b) { return !std::memcmp(&a, &b, sizeof a); }

static int rule_checks() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float caps[] = { 32.0f, inf, 1e-30f, 0.0f, -1.0f, nan, -inf }, tols[] = { 0.02f, 1e-30f, 0.0f, -0.5f, inf, nan };
    const int sizes[][2] = { { 1, 1 }, { 20, 12 }, { 12, 20 }, { 2147483647, 1 } }, faces[] = { 0, 1, 978, 2147483647 };
    int calls = 0;
    for (int have = 0; have < 2; have++)
        for (const auto &ks : sizes) for (const auto &s : sizes)
            for (int kf : faces) for (int f : faces)
                for (int tree = 0; tree < 2; tree++)
                    for (float cap : caps) for (float tol : tols) {
                        MptHistoryVerdict want = MPT_HISTORY_OK;
                        if (!have) want = MPT_HISTORY_NONE;
                        else if (ks[0] != s[0] || ks[1] != s[1]) want = MPT_HISTORY_SIZE;
                        else if (kf != f) want = MPT_HISTORY_FACES;
                        else if (!tree) want = MPT_HISTORY_STALE_TREE;
                        else if (!(cap > 0.0f)) want = MPT_HISTORY_MAX_HISTORY;
                        else if (!(tol > 0.0f) || !std::isfinite(tol)) want = MPT_HISTORY_DEPTH_TOL;
                        CHECK(mpt_history_rule(have, ks[0], ks[1], s[0], s[1], kf, f, tree, cap, tol, nullptr, 0) == want);
                        CHECK(mpt_history_rule(have, ks[0], ks[1], s[0], s[1], kf, f, tree, cap, tol, nullptr, 64) == want);
                        for (size_t room = 0; room <= 256; room += room < 4 ? 1 : 63) {
                            std::vector<char> why(room, 'x');          // exactly `room` bytes of the heap
                            CHECK(mpt_history_rule(have, ks[0], ks[1], s[0], s[1], kf, f, tree, cap, tol, room ? why.data() : nullptr, room) == want);
                            calls++;
                            if (!room) continue;
                            CHECK(std::memchr(why.data(), 0, room) != nullptr);
                            if (want == MPT_HISTORY_OK) CHECK(why[0] == 0);
                            else if (room >= 256) CHECK(!std::strncmp(why.data(), "reproject: ", 11) && std::strlen(why.data()) > 20);
                        }
                    }
    return calls;
}

static void project_checks() {
    const float eye[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, -1, 0, 0, -1, 0 };        // clip = (x, y, -1, -z): looks down -z from the origin, near plane z = -1
    const float inv[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, -1, 0, 0, -1, 0 };        // its inverse (the matrix is an involution)
    const float a[3] = { -1, -1, -2 }, b[3] = { 1, -1, -2 }, c[3] = { -1, 1, -2 };
    float fx = 0, fy = 0, d = 0;
    CHECK(mpt_history_project(a, b, c, 0.5f, 0.5f, eye, inv, 64, 48, &fx, &fy, &d));   // the point (0, 0, -2): the film's centre
    CHECK(fx == 31.5f && fy == 23.5f && std::fabs(d - 1.0f) < 1e-6f);                  // (the near-plane point of that ray is (0, 0, -1))
    CHECK(mpt_history_project(a, b, c, 0.0f, 0.0f, eye, inv, 64, 48, &fx, &fy, &d));   // corner a: clip (-1/2, -1/2)
    CHECK(fx == 15.5f && fy == 11.5f);
    const float behind[3] = { 0, 0, 3 };
    CHECK(!mpt_history_project(behind, behind, behind, 0.25f, 0.25f, eye, inv, 64, 48, &fx, &fy, &d));
    const float at_eye[3] = { 0, 0, 0 };
    CHECK(!mpt_history_project(at_eye, at_eye, at_eye, 0.25f, 0.25f, eye, inv, 64, 48, &fx, &fy, &d));
    const float nan = std::numeric_limits<float>::quiet_NaN(), bad[3] = { nan, 0, -2 };
    CHECK(!mpt_history_project(bad, b, c, 0.0f, 0.0f, eye, inv, 64, 48, &fx, &fy, &d));   // (a position that is no number has no w that is positive)
}

static long pixel_checks() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::mt19937 rng(20);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    long pixels = 0, outcomes[MPT_OUTCOMES] = {};
    const int films[][2] = { { 1, 1 }, { 1, 7 }, { 16, 16 }, { 20, 12 } };
    for (const auto &fs : films) {
        const int nx = fs[0], ny = fs[1];
        const size_t n = (size_t)nx * ny;
        for (int round = 0; round < 200; round++) {
            std::vector<V4> f(n);
            std::vector<int32_t> face(n), id(n);
            std::vector<float> depth(n);
            for (size_t q = 0; q < n; q++) {
                const float w = rng() % 5 ? (float)(1 + rng() % 64) : 0.0f;
                f[q] = { uni(rng) * w, uni(rng) * w, rng() % 9 ? uni(rng) * w : -0.0f, w };
                face[q] = (int)(rng() % 4) - 1;
                id[q] = face[q] < 0 ? -1 : (int)(rng() % 2);
                depth[q] = 5.0f * (1.0f + (rng() % 3 ? 0.0f : 0.0201f));
            }
            const float special[] = { -1.0f, -0.999f, -0.5f, 0.0f, 0.5f, (float)nx - 1.0f, (float)nx - 0.5f, (float)nx, (float)nx + 0.5f, 1e30f, -1e30f, inf, -inf, nan,
                                      2147483648.0f, -2147483904.0f };
            for (int i = 0; i < nx; i++)
                for (int j = 0; j < ny; j++) {
                    MptMotion m;
                    m.cur_id = (int)(rng() % 3) - 1;
                    m.fx = rng() % 3 ? (float)i + 3.0f * (uni(rng) - 0.5f) : special[rng() % (sizeof special / sizeof *special)];
                    m.fy = rng() % 3 ? (float)j + 3.0f * (uni(rng) - 0.5f) : special[rng() % (sizeof special / sizeof *special)];
                    m.d_exp = rng() % 8 ? 5.0f : nan;
                    m.flags = m.cur_id < 0 ? (rng() % 2 ? MPT_MOTION_BACKGROUND : MPT_MOTION_NONE) : MPT_MOTION_NONE;
                    const float cap = rng() % 2 ? inf : (float)(1 + rng() % 40);
                    V4 out = { 7, 7, 7, 7 };
                    const MptHistoryOutcome o = mpt_history_pixel(f.data(), face.data(), id.data(), depth.data(), nx, ny, i, j, m, cap, 0.02f, &out);
                    CHECK(o >= 0 && o < MPT_OUTCOMES && o != MPT_OUTCOME_STATIC);
                    const bool has = o == MPT_OUTCOME_KEPT || o == MPT_OUTCOME_BACKGROUND_KEPT;
                    CHECK(has == (out.w > 0.0f) && out.w <= cap * 1.000001f);
                    if (!has) CHECK(out.x == 0 && out.y == 0 && out.z == 0 && out.w == 0);
                    outcomes[o]++; pixels++;
                    // the same pixel looking at itself with a matching G-buffer keeps every word, -0 too
                    const size_t q = (size_t)i * ny + j;
                    if (f[q].w > 0.0f) {
                        MptMotion s = { 1, (float)i, (float)j, depth[q], MPT_MOTION_STATIC };
                        const int32_t was = id[q];
                        id[q] = 1;
                        CHECK(mpt_history_pixel(f.data(), face.data(), id.data(), depth.data(), nx, ny, i, j, s, inf, 0.02f, &out) == MPT_OUTCOME_STATIC);
                        CHECK(same_bits(out, f[q]));
                        id[q] = was;
                    }
                }
        }
    }
    for (int o = 0; o < MPT_OUTCOMES; o++)
        if (o != MPT_OUTCOME_STATIC) CHECK(outcomes[o] > 0);
    return pixels;
}

int main() {
    const int calls = rule_checks();
    project_checks();
    const long pixels = pixel_checks();
    std::printf("history_rule_check: %d rule calls with a message buffer, %ld resampled pixels, %d failures\n", calls, pixels, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

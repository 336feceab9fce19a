// scatter_rule_check.cpp -- the rule of a scatter (ptina_amd/csrc/scatter_rule.h: draws, weights, shares, selection, placement)
// exercised by a stand-alone program, so that it can run under the host sanitizers without a GPU and without loading anything into
// an interpreter:
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/scatter_rule_check.cpp -o scatter_rule_check && ./scatter_rule_check
//
// Every table lives on the heap and is exactly as long as the functions may read: a total T near 2^45 (2^21 - 1 faces of the full
// share), faces with q = 0 at either end of a table and in its middle (never chosen), a single face; the frame for N along each
// axis in both directions -- N = (0, 0, -1) is the construction's special case -- and for random unit vectors; the yaw's fallback
// (an instance whose eight pairs all miss the disc, found by search, and the pairs' own admission rule); densities over images
// exactly nx x ny texels large with uvs that wrap on both sides; weights that are not finite; shares at and above the largest.

#include "../ptina_amd/csrc/scatter_rule.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static std::vector<uint64_t> scan(const std::vector<uint32_t> &q) {
    std::vector<uint64_t> cdf(q.size() + 1);
    uint64_t at = 0;
    for (size_t g = 0; g < q.size(); g++) { cdf[g] = at; at += q[g]; }
    cdf[q.size()] = at;
    return cdf;
}

// the face the definition names, by a plain walk
static int64_t face_by_walk(const std::vector<uint64_t> &cdf, uint64_t t) {
    int64_t g = -1;
    for (size_t k = 0; k + 1 < cdf.size(); k++)
        if (cdf[k] <= t) g = (int64_t)k;
    return g;
}

static void check_selection(const std::vector<uint32_t> &q, uint64_t seed, int count) {
    const std::vector<uint64_t> cdf = scan(q);
    const uint64_t key = mpt_scatter_mix(seed), T = cdf.back();
    for (int i = 0; i < count; i++) {
        MptScatterPoint *r = new MptScatterPoint;
        mpt_scatter_select(cdf.data(), (int64_t)q.size(), key, (uint64_t)i, 0.5, 2.0, 1, r);
        const uint64_t t = mpt_scatter_draw(key, (uint64_t)i, 0) % T;
        CHECK(r->face >= 0 && (size_t)r->face < q.size() && q[(size_t)r->face] > 0);
        if (q.size() <= 4096) CHECK(r->face == face_by_walk(cdf, t));
        CHECK(cdf[(size_t)r->face] <= t && t < cdf[(size_t)r->face + 1]);
        CHECK(r->b1 >= 0 && r->b2 >= 0 && r->b1 + r->b2 <= 1.0 + 1e-15);
        CHECK(r->scale >= 0.5 && r->scale <= 2.0);
        CHECK(std::fabs(r->cy * r->cy + r->sy * r->sy - 1.0) < 1e-15);
        delete r;
    }
}

static void check_frame(const double N[3]) {
    double *T0 = new double[3], *B0 = new double[3];
    mpt_scatter_basis(N, T0, B0);
    const double tt = T0[0] * T0[0] + T0[1] * T0[1] + T0[2] * T0[2], bb = B0[0] * B0[0] + B0[1] * B0[1] + B0[2] * B0[2];
    const double tb = T0[0] * B0[0] + T0[1] * B0[1] + T0[2] * B0[2], tn = T0[0] * N[0] + T0[1] * N[1] + T0[2] * N[2], bn = B0[0] * N[0] + B0[1] * N[1] + B0[2] * N[2];
    CHECK(std::fabs(tt - 1) < 1e-14 && std::fabs(bb - 1) < 1e-14 && std::fabs(tb) < 1e-14 && std::fabs(tn) < 1e-14 && std::fabs(bn) < 1e-14);
    // T0 x N = B0: the columns T0, N, B0 are right-handed
    const double c[3] = { T0[1] * N[2] - T0[2] * N[1], T0[2] * N[0] - T0[0] * N[2], T0[0] * N[1] - T0[1] * N[0] };
    for (int k = 0; k < 3; k++) CHECK(std::fabs(c[k] - B0[k]) < 1e-14);
    delete[] T0; delete[] B0;
}

int main() {
    // ---- draws
    CHECK(mpt_scatter_mix(0) == 0xE220A8397B1DCDAFull);
    CHECK(mpt_scatter_unit(0) == 0x1p-54 && mpt_scatter_unit(~0ull) == 1.0 && mpt_scatter_unit(1ull << 62) == 0.25 + 0x1p-54);
    CHECK(mpt_scatter_draw(mpt_scatter_mix(5), 3, 2) == mpt_scatter_mix(mpt_scatter_mix(5) + 50));

    // ---- selection: runs of q = 0 at the beginning, in the middle and at the end; a single face; a single share at either end
    check_selection({ 0, 0, 3, 1, 0, 0, 0, 2, 5, 1, 0, 0 }, 7, 4096);
    check_selection({ 5 }, 1, 64);
    check_selection({ 1, 0, 0, 0 }, 1, 64);
    check_selection({ 0, 0, 0, 1 }, 1, 64);
    check_selection({ 1u << 24, 0, 1, 1u << 24 }, 2, 4096);
    {   // T near 2^45
        std::vector<uint32_t> big(((size_t)1 << 21) - 1, 1u << 24);
        CHECK(scan(big).back() == ((((uint64_t)1 << 21) - 1) << 24));
        check_selection(big, 11, 512);
        big.front() = big.back() = 0;
        check_selection(big, 12, 512);
    }

    // ---- the yaw's fallback: an instance whose eight pairs all miss, by search; without random_yaw every instance has (1, 0)
    {
        const std::vector<uint64_t> cdf = scan({ 7 });
        const uint64_t key = mpt_scatter_mix(99);
        long long found = -1, searched = 0;
        for (uint64_t i = 0; i < 40000000 && found < 0; i++, searched++) {
            bool any = false;
            for (uint32_t j = 0; j < 8 && !any; j++) {
                const double x = 2.0 * mpt_scatter_unit(mpt_scatter_draw(key, i, 4 + 2 * j)) - 1.0, y = 2.0 * mpt_scatter_unit(mpt_scatter_draw(key, i, 5 + 2 * j)) - 1.0;
                any = x * x + y * y > 0x1p-20 && x * x + y * y <= 1.0;
            }
            if (!any) found = (long long)i;
        }
        CHECK(found >= 0);
        if (found >= 0) {
            MptScatterPoint r;
            mpt_scatter_select(cdf.data(), 1, key, (uint64_t)found, 1.0, 1.0, 1, &r);
            CHECK(r.cy == 1.0 && r.sy == 0.0 && r.face == 0);
            std::printf("yaw fallback: instance %lld of seed 99 (searched %lld)\n", found, searched);
        }
        for (uint64_t i = 0; i < 256; i++) {
            MptScatterPoint r;
            mpt_scatter_select(cdf.data(), 1, key, i, 1.0, 1.0, 0, &r);
            CHECK(r.cy == 1.0 && r.sy == 0.0);
        }
    }

    // ---- frames: the axes in both directions, -0 in z, random unit vectors
    {
        const double axes[8][3] = { { 1, 0, 0 }, { -1, 0, 0 }, { 0, 1, 0 }, { 0, -1, 0 }, { 0, 0, 1 }, { 0, 0, -1 }, { 1, 0, -0.0 }, { 0, 1, -0.0 } };
        for (const auto &a : axes) check_frame(a);
        uint64_t s = 1;
        for (int k = 0; k < 4096; k++) {
            double v[3], n[3];
            for (double &x : v) { s = mpt_scatter_mix(s); x = 2.0 * mpt_scatter_unit(s) - 1.0; }
            mpt_scatter_normalise(v, n);
            check_frame(n);
        }
    }

    // ---- placement: the matrix of a point on a face; a collapsed face gives NaN in the frame and a number in the point
    {
        const double P0[3] = { 0, 0, 0 }, P1[3] = { 2, 0, 0 }, P2[3] = { 0, 0, -2 }, up[3] = { 0, 0, -1 };
        MptScatterPoint r{};
        r.b1 = 0.25; r.b2 = 0.5; r.scale = 3.0; r.cy = 1.0; r.sy = 0.0;
        double *W = new double[16];
        mpt_scatter_place(P0, P1, P2, r, 0, up, W);
        CHECK(W[3] == 0.5 && W[7] == 0.0 && W[11] == -1.0 && W[12] == 0 && W[13] == 0 && W[14] == 0 && W[15] == 1);
        CHECK(W[1] == 0.0 && W[5] == 3.0 && W[9] == 0.0);                 // cross((2,0,0), (0,0,-2)) = (0, 4, 0): N = +Y
        mpt_scatter_place(P0, P1, P2, r, 1, up, W);
        CHECK(W[1] == 0.0 && W[5] == 0.0 && W[9] == -3.0);
        mpt_scatter_place(P0, P1, P1, r, 0, up, W);
        CHECK(W[0] != W[0] && W[5] != W[5] && W[10] != W[10] && W[3] == 1.5);
        delete[] W;
    }

    // ---- weights and shares
    {
        const double P0[3] = { 0, 0, 0 }, P1[3] = { 1, 0, 0 }, P2[3] = { 0, 1, 0 }, far[3] = { 1e200, 1e200, 0 };
        const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
        CHECK(mpt_scatter_weight(P0, P1, P2, 1.0) == 0.5 && mpt_scatter_weight(P0, P1, P2, 0.0) == 0.0);
        CHECK(mpt_scatter_weight(P0, P1, P1, 1.0) == 0.0);
        CHECK(mpt_scatter_weight(P0, far, P2, 1.0) == 0.0);             // the area overflows: not finite, counts as 0
        CHECK(mpt_scatter_weight(P0, P1, P2, nan) == 0.0 && mpt_scatter_weight(P0, P1, P2, inf) == 0.0);
        CHECK(mpt_scatter_quantise(0.5, 0.5) == (1u << 24) && mpt_scatter_quantise(0.25, 0.5) == (1u << 23) && mpt_scatter_quantise(0.0, 0.5) == 0);
        CHECK(mpt_scatter_quantise(0x1p-25, 1.0) == 0 && mpt_scatter_quantise(0x1p-24, 1.0) == 1);   // below 2^-24 of the largest: no share
        CHECK(mpt_scatter_quantise(1.0, 0.0) == 0 && mpt_scatter_quantise(nan, 1.0) == 0 && mpt_scatter_quantise(1.0, nan) == 0);
    }

    // ---- density: images exactly nx x ny texels large; uvs that leave the image on both sides; every channel; the clamp; NaN
    for (int nx = 1; nx <= 4; nx++)
        for (int ny = 1; ny <= 3; ny++) {
            std::vector<float> img((size_t)nx * ny * 4);
            for (size_t k = 0; k < img.size(); k++) img[k] = (float)((k * 37 % 11) / 10.0);
            for (int ch = 0; ch <= 4; ch++)
                for (float u = -2.5f; u <= 2.5f; u += 0.625f) {
                    const float uv[3][2] = { { u, -u }, { u + 0.25f, 0.5f * u }, { u - 0.5f, u } };
                    const double d = mpt_scatter_density(img.data(), nx, ny, ch, uv);
                    CHECK(d >= 0.0 && d <= 1.0);
                }
        }
    {
        const float img[2 * 2 * 4] = { 0, 0, 0, 0, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 2, 2, 2, -1 };
        const float at0[3][2] = { { 0, 0 }, { 0, 0 }, { 0, 0 } }, at1[3][2] = { { 1, 1 }, { 1, 1 }, { 1, 1 } };
        const float nanuv[3][2] = { { std::numeric_limits<float>::quiet_NaN(), 0 }, { 0, 0 }, { 0, 0 } };
        CHECK(mpt_scatter_density(img, 2, 2, 0, at0) == 0.0 && mpt_scatter_density(img, 2, 2, 0, at1) == 1.0);   // 2 clamps to 1
        CHECK(mpt_scatter_density(img, 2, 2, 3, at1) == 0.0);                                                   // -1 clamps to 0
        CHECK(mpt_scatter_density(img, 2, 2, 4, at1) == 1.0);
        CHECK(mpt_scatter_density(img, 2, 2, 0, nanuv) == 0.0);
    }

    // ---- a surface's corner: the composition's position, unrounded
    {
        const float rec[3] = { 1.0f, 2.0f, 3.0f };
        const double W[16] = { 2, 0, 0, 1, 0, 2, 0, 1, 0, 0, 2, 1, 0, 0, 0, 2 };
        double P[3];
        mpt_scatter_corner(rec, W, P);
        CHECK(P[0] == 1.5 && P[1] == 2.5 && P[2] == 3.5);
    }

    if (failures) { std::fprintf(stderr, "scatter_rule_check: %d checks failed\n", failures); return 1; }
    std::printf("scatter_rule_check: ok\n");
    return 0;
}

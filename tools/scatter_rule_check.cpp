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
// The elimination of a spaced scatter (`scatter_rule_check space` runs it alone): the greedy pass and its synchronous round count
// against a plain simulation of the rounds on a chain, coincident points, a pair exactly r apart and an f64 closer, NaN and infinite
// coordinates and uniform points; and the device's grid -- edge, cell, bucket -- on boxes from a point to 2^30 r and beyond the
// finite numbers: cells are monotone and inside their counts, and no conflicting pair lies more than a cell apart.

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

// kept flags and rounds by simulating the synchronous rounds over all pairs
static int32_t rounds_by_simulation(const std::vector<double> &pos, double r, std::vector<uint8_t> &kept) {
    const int64_t n = (int64_t)(pos.size() / 3);
    std::vector<int> state((size_t)n, MPT_SPACE_UNDECIDED), next;
    int32_t rounds = 0;
    for (bool open = n > 0; open; rounds++) {
        next = state;
        open = false;
        for (int64_t j = 0; j < n; j++) {
            if (state[(size_t)j] != MPT_SPACE_UNDECIDED) continue;
            bool any_kept = false, any_undecided = false;
            for (int64_t k = 0; k < j; k++) {
                if (!mpt_scatter_conflict(&pos[(size_t)j * 3], &pos[(size_t)k * 3], r * r)) continue;
                any_kept |= state[(size_t)k] == MPT_SPACE_KEPT;
                any_undecided |= state[(size_t)k] == MPT_SPACE_UNDECIDED;
            }
            next[(size_t)j] = mpt_scatter_space_decide(any_kept, any_undecided);
            open |= next[(size_t)j] == MPT_SPACE_UNDECIDED;
        }
        state = next;
    }
    kept.resize((size_t)n);
    for (int64_t j = 0; j < n; j++) kept[(size_t)j] = state[(size_t)j] == MPT_SPACE_KEPT;
    return rounds;
}

static int32_t check_space(const std::vector<double> &pos, double r, std::vector<uint8_t> *out = nullptr) {
    const int64_t n = (int64_t)(pos.size() / 3);
    std::vector<uint8_t> kept((size_t)n), want;
    std::vector<int32_t> t((size_t)n);
    const int32_t rounds = mpt_scatter_space_of(pos.data(), n, r, kept.data(), t.data());
    CHECK(rounds == rounds_by_simulation(pos, r, want));
    CHECK(kept == want);
    // the grid: every point of the box in a cell inside the counts, and conflicting pairs at most a cell apart
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    auto finite = [&](int64_t j) { return std::isfinite(pos[(size_t)j * 3]) && std::isfinite(pos[(size_t)j * 3 + 1]) && std::isfinite(pos[(size_t)j * 3 + 2]); };
    for (int64_t j = 0; j < n; j++)
        for (int k = 0; k < 3 && finite(j); k++) { lo[k] = std::fmin(lo[k], pos[(size_t)j * 3 + k]); hi[k] = std::fmax(hi[k], pos[(size_t)j * 3 + k]); }
    if (lo[0] <= hi[0]) {
        const double h = mpt_space_edge(r, lo, hi);
        CHECK(h > r || !std::isfinite(r));
        std::vector<int32_t> cell((size_t)n * 3, 0);
        for (int64_t j = 0; j < n; j++)
            for (int k = 0; k < 3 && finite(j); k++) {
                const int32_t c = cell[(size_t)j * 3 + k] = mpt_space_cell(pos[(size_t)j * 3 + k], lo[k], h);
                CHECK(c >= 0 && c <= mpt_space_cell(hi[k], lo[k], h) && c <= (1 << 20) + 1 && mpt_space_cell(lo[k], lo[k], h) == 0);
            }
        for (int64_t j = 0; j < n; j++)
            for (int64_t k = 0; k < j; k++) {
                for (int a = 0; a < 3 && finite(j) && finite(k); a++)      // monotone
                    CHECK((pos[(size_t)j * 3 + a] <= pos[(size_t)k * 3 + a]) == (cell[(size_t)j * 3 + a] <= cell[(size_t)k * 3 + a]) ||
                          cell[(size_t)j * 3 + a] == cell[(size_t)k * 3 + a]);
                if (!mpt_scatter_conflict(&pos[(size_t)j * 3], &pos[(size_t)k * 3], r * r)) continue;
                for (int a = 0; a < 3; a++) CHECK(std::abs(cell[(size_t)j * 3 + a] - cell[(size_t)k * 3 + a]) <= 1);
            }
        CHECK(mpt_space_bucket(1 << 20, (1 << 20) + 1, 0, 1023) < 1024 && mpt_space_bucket(0, 0, 0, 0) == 0);
    }
    if (out) *out = kept;
    return rounds;
}

static int space_checks() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<uint8_t> kept;
    {   // a chain 0.6 r apart in index order, and in reverse: every second one, and as many rounds as points
        std::vector<double> chain(40 * 3, 0.0), back(40 * 3, 0.0);
        for (int j = 0; j < 40; j++) { chain[(size_t)j * 3] = 0.6 * j; back[(size_t)j * 3] = 0.6 * (39 - j); }
        CHECK(check_space(chain, 1.0, &kept) == 40);
        for (int j = 0; j < 40; j++) CHECK(kept[(size_t)j] == (j % 2 == 0));
        CHECK(check_space(back, 1.0, &kept) == 40);
        for (int j = 0; j < 40; j++) CHECK(kept[(size_t)j] == (j % 2 == 0));
    }
    {   // coincident points: the first alone; a single point; no point
        std::vector<double> same(64 * 3, 0.25);
        CHECK(check_space(same, 0.5, &kept) == 2 && kept[0] == 1);
        for (int j = 1; j < 64; j++) CHECK(kept[(size_t)j] == 0);
        CHECK(check_space({ 1.0, 2.0, 3.0 }, 0.5, &kept) == 1 && kept[0] == 1);
        CHECK(check_space({}, 0.5) == 0);
        CHECK(check_space(same, 0.0, &kept) == 1 && kept[63] == 1);          // r = 0: nothing conflicts
    }
    {   // exactly r apart: (3, 4, 12) / 16 at r = 13 / 16, every operation exact -- allowed; an f64 closer -- a conflict
        std::vector<double> pair = { 0.25, -0.5, 1.0, 0.25 + 3.0 / 16, -0.5 + 4.0 / 16, 1.0 + 12.0 / 16 };
        CHECK(check_space(pair, 13.0 / 16, &kept) == 1 && kept[1] == 1);
        for (int k = 0; k < 8; k++) pair[3] = std::nextafter(pair[3], -inf);
        CHECK(check_space(pair, 13.0 / 16, &kept) == 2 && kept[1] == 0);
    }
    {   // coordinates that are not finite conflict with nothing; an r whose square overflows conflicts with every finite distance
        std::vector<double> pts = { 0, 0, 0, nan, 0, 0, 0.1, 0, 0, inf, 0, 0, inf, 0, 0, 0, -inf, 0 };
        CHECK(check_space(pts, 0.5, &kept) == 2);
        CHECK(kept[0] == 1 && kept[1] == 1 && kept[2] == 0 && kept[3] == 1 && kept[4] == 1 && kept[5] == 1);
        CHECK(check_space({ 0, 0, 0, 1e150, 0, 0, -1e300, 1e300, 0 }, 1e200, &kept) == 2 && kept[1] == 0 && kept[2] == 1);   // (d2 of the third overflows too)
        CHECK(check_space({ -1e308, 0, 0, 1e308, 0, 0, 1e308, 1.0, 0 }, 2.0, &kept) == 2 && kept[2] == 0);                    // an extent beyond the finite numbers
    }
    {   // uniform points in a unit cube, at distances that reject from a few to nearly all; extents of 2^30 r and of a subnormal r
        uint64_t s = 7;
        for (int n : { 2, 63, 257, 600 })
            for (double r : { 0.02, 0.09, 0.3, 2.0 }) {
                std::vector<double> pts((size_t)n * 3);
                for (double &x : pts) { s = mpt_scatter_mix(s); x = mpt_scatter_unit(s); }
                check_space(pts, r);
                for (int k = 0; k < 3; k++) pts[(size_t)(n - 1) * 3 + k] = 0x1p30 * r;
                pts[0] = pts[(size_t)(n - 1) * 3] - 0.5 * r; pts[1] = pts[2] = 0x1p30 * r;
                check_space(pts, r);
                check_space(pts, 0x1p-1070);
            }
    }
    return 0;
}

int main(int argc, char **argv) {
    space_checks();
    if (argc > 1 && !std::strcmp(argv[1], "space")) {
        if (failures) { std::fprintf(stderr, "scatter_rule_check space: %d checks failed\n", failures); return 1; }
        std::printf("scatter_rule_check space: ok\n");
        return 0;
    }
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

// anim_blend_rule_check.cpp -- the rule of two blended clips and of an object moved by a clip (the additions of DESIGN.md section
// 3.17.2 to ptina_amd/csrc/anim_rule.h) exercised by a stand-alone program, so that it can run under the host sanitizers without a
// GPU and without loading anything into an interpreter:
//
//     c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/anim_blend_rule_check.cpp -o anim_blend_rule_check && ./anim_blend_rule_check
//
// A few fixed skeletons -- 1, 3 and 64 joints and the chain of 256 with T, R and S tracks on every joint of both clips -- in arrays
// that are exactly as long as the rule may read.  Held: the weight of a fade at its corners; at weight 0 the blended pose is clip A's
// alone and at weight 1 clip B's alone, bit for bit; a blend of a clip with itself is finite and, rigid joints, orthonormal; every
// refusal of the two bindings with message buffers of every size; object clips with T, R, S, all and none: the world matrix is
// base . local, and base itself for the identity motion.

#include "../ptina_amd/csrc/anim_rule.h"
#include <cstdlib>
#include <cstring>
#include <limits>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static unsigned long long rng_state = 0x2545F4914F6CDD1Dull;
static unsigned rnd(unsigned n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33) % n;
}
static double unit() { return ((double)rnd(1u << 24) + 0.5) / (double)(1u << 24); }
static void quaternion(float q[4]) {
    double v[4], len = 0;
    for (int c = 0; c < 4; c++) { v[c] = 2.0 * unit() - 1.0; len += v[c] * v[c]; }
    len = std::sqrt(len);
    for (int c = 0; c < 4; c++) q[c] = (float)(v[c] / len);
}

struct Clip {
    std::vector<int32_t> spec; std::vector<float> times, values;
    std::vector<MptAnimTrack> tracks; double t0 = 0, t1 = 0;
};

static void add_track(Clip &c, int target, int path, int nt) {
    const int interp = (int)rnd(3), nkeys = 1 + (int)rnd(9);
    c.spec.insert(c.spec.end(), { target, path, interp, nkeys });
    float t = (float)unit();
    for (int k = 0; k < nkeys; k++) { c.times.push_back(t); t += 0.01f + (float)unit(); }
    const int C = mpt_anim_components(path, nt);
    for (int k = 0; k < nkeys; k++)
        for (int part = 0; part < (interp == MPT_ANIM_CUBICSPLINE ? 3 : 1); part++) {
            const bool value = interp != MPT_ANIM_CUBICSPLINE || part == 1;
            float q[4];
            quaternion(q);
            for (int e = 0; e < C; e++)
                c.values.push_back(!value ? (float)(0.2 * unit() - 0.1) : path == MPT_ANIM_R ? q[e] : path == MPT_ANIM_S ? (float)(0.5 + unit()) : (float)(2.0 * unit() - 1.0));
        }
}

// tracks on every (joint, path <= last) with probability `density` in 256ths, and the weights; checked as a clip of (nj, nt)
static Clip make_clip(int nj, int nt, int last, unsigned density) {
    Clip c;
    for (int j = 0; j < nj; j++)
        for (int path = MPT_ANIM_T; path <= last; path++)
            if (rnd(256) < density) add_track(c, j, path, nt);
    if (nt > 0) add_track(c, -1, MPT_ANIM_W, nt);
    const int n = (int)(c.spec.size() / 4);
    c.spec.shrink_to_fit(); c.times.shrink_to_fit(); c.values.shrink_to_fit();
    CHECK(mpt_clip_rule(nj, nt, n, c.spec.data(), c.times.data(), (int64_t)c.times.size(), c.values.data(), (int64_t)c.values.size(), nullptr, 0) == MPT_CLIP_OK);
    c.tracks.resize((size_t)n);
    mpt_anim_tracks(nt, n, c.spec.data(), c.times.data(), c.tracks.data(), &c.t0, &c.t1);
    return c;
}

static bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

int main() {
    int poses = 0, worlds = 0, refusals = 0;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- the weight
    CHECK(mpt_anim_blend_weight(1.0, 0.25, 0.75, 2.0, 1.0) == 0.25 && mpt_anim_blend_weight(1.0, 0.25, 0.75, 1.0, 0.5) == 0.25);
    CHECK(mpt_anim_blend_weight(1.0, 0.25, 0.75, 0.5, 0.5) == 0.75 && mpt_anim_blend_weight(9.0, 0.25, 0.75, 0.5, 0.5) == 0.75);
    CHECK(mpt_anim_blend_weight(1.0, 0.0, 1.0, 0.5, 2.0) == 0.25 && mpt_anim_blend_weight(1.0, 0.9, 0.2, 0.75, 1.0) == 0.9 + 0.25 * (0.2 - 0.9));
    CHECK(mpt_anim_blend_weight(1.0, 0.125, 0.875, 1.0, 0.0) == 0.875 && mpt_anim_blend_weight(1.0, 0.125, 0.875, 1.5, 0.0) == 0.125);
    // ---- the second binding's refusals
    for (int what = 0; what < 7; what++) {
        double a[6] = { 0.0, 1.0, 0.0, 1.0, 0.0, 1.0 };          // offset speed w0 w1 fade_start fade_duration
        static const int at[7] = { 0, 1, 4, 5, 5, 2, 3 };
        static const MptBlendVerdict want[7] = { MPT_BLEND_NOT_FINITE, MPT_BLEND_NOT_FINITE, MPT_BLEND_NOT_FINITE, MPT_BLEND_NOT_FINITE, MPT_BLEND_DURATION,
                                                 MPT_BLEND_WEIGHT, MPT_BLEND_WEIGHT };
        a[at[what]] = what == 4 ? -1.0 : what == 5 ? -1e-300 : what == 6 ? nan : inf;
        for (size_t cap = 0; cap <= 80; cap += cap < 8 ? 1 : 24) {
            std::vector<char> why(cap, 'x');
            CHECK(mpt_blend_rule(a[0], a[1], a[2], a[3], a[4], a[5], cap ? why.data() : nullptr, cap) == want[what]);
            if (cap) CHECK(std::memchr(why.data(), 0, cap) != nullptr);
            refusals++;
        }
    }
    CHECK(mpt_blend_rule(0.0, -2.0, 0.0, 1.0, -5.0, 0.0, nullptr, 0) == MPT_BLEND_OK);
    // ---- blended poses
    static const int joints[5] = { 1, 3, 64, 256, 0 }, targets[5] = { 0, 3, 1, 0, 64 };
    for (int s = 0; s < 5; s++) {
        const int nj = joints[s], nt = targets[s];
        const bool chain = nj == 256;
        std::vector<int32_t> parents((size_t)nj);
        std::vector<double> rest((size_t)nj * MPT_ANIM_REST), ib((size_t)nj * 12);
        for (int j = 0; j < nj; j++) {
            parents[j] = j == 0 ? -1 : chain ? j - 1 : (int)rnd((unsigned)j + 1) - 1;
            float q[4];
            quaternion(q);
            double *r = rest.data() + (size_t)j * MPT_ANIM_REST;
            for (int k = 0; k < 3; k++) { r[k] = 0.2 * unit() - 0.1; r[7 + k] = 1.0; }
            for (int k = 0; k < 4; k++) r[3 + k] = q[k];
            const double bind[MPT_ANIM_REST] = { unit(), unit(), unit(), q[1], -q[0], q[3], -q[2], 1.0, 1.0, 1.0 };
            mpt_anim_local(bind, ib.data() + (size_t)j * 12);
        }
        if (nj > 0) CHECK(mpt_skeleton_rule(nj, parents.data(), rest.data(), ib.data(), nullptr, 0) == MPT_SKELETON_OK);
        // the chain: T, R and S on every joint of both clips (768 tracks each); the others: T and R on half the joints, so that they stay rigid
        const Clip A = make_clip(nj, nt, chain ? MPT_ANIM_S : MPT_ANIM_R, chain ? 256 : 128), B = make_clip(nj, nt, chain ? MPT_ANIM_S : MPT_ANIM_R, chain ? 256 : 128);
        if (chain) CHECK(A.tracks.size() == 768 && B.tracks.size() == 768);
        const size_t n = (size_t)nt + (size_t)nj * 12;
        std::vector<double> pa(n), pb(n), p(n);
        for (int q = 0; q < 8; q++) {
            const double t = 3.0 * unit() - 0.5;
            const double ta = mpt_anim_local_time(t, 0.25, 1.0, q % 2, A.t0, A.t1), tb = mpt_anim_local_time(t, -0.5, -1.5, 1, B.t0, B.t1);
            mpt_anim_pose(nj, nt, parents.data(), rest.data(), ib.data(), (int)A.tracks.size(), A.tracks.data(), A.times.data(), A.values.data(), ta, pa.data());
            mpt_anim_pose(nj, nt, parents.data(), rest.data(), ib.data(), (int)B.tracks.size(), B.tracks.data(), B.times.data(), B.values.data(), tb, pb.data());
            const double ws[5] = { 0.0, 1.0, 0.5, std::ldexp(1.0, -53), 1.0 - std::ldexp(1.0, -53) };
            for (int k = 0; k < 5; k++) {
                for (double &x : p) x = nan;
                mpt_anim_pose_blend(nj, nt, parents.data(), rest.data(), ib.data(), (int)A.tracks.size(), A.tracks.data(), A.times.data(), A.values.data(), ta,
                                    (int)B.tracks.size(), B.tracks.data(), B.times.data(), B.values.data(), tb, ws[k], p.data());
                for (double x : p) CHECK(std::isfinite(x));
                if (k == 0) CHECK(same_bits(p, pa));
                if (k == 1) CHECK(same_bits(p, pb));
                if (!chain)
                    for (int j = 0; j < nj; j++) {                          // rotations and shifts only, blended: still rigid
                        const double *P = p.data() + nt + (size_t)j * 12;
                        for (int a = 0; a < 3; a++)
                            for (int b = 0; b < 3; b++) CHECK(std::fabs((P[a] * P[b] + P[4 + a] * P[4 + b] + P[8 + a] * P[8 + b]) - (a == b)) < 1e-4);
                    }
                poses++;
            }
        }
    }
    // ---- the nlerp's corners: d < 0 takes the shorter arc; d == 0 keeps b; identical rotations stay; lengths do not matter to the direction
    {
        double a[4] = { 0, 0, 0, 1 };
        const double b[4] = { 0, 0, -0.6, -0.8 };
        mpt_anim_blend_rotation(a, b, 0.5);
        CHECK(a[3] > 0.9 && a[2] > 0.0 && std::fabs(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3] - 1.0) < 1e-14);
        double c[4] = { 0, 0, 0, 1 };
        const double e[4] = { 1, 0, 0, 0 };
        mpt_anim_blend_rotation(c, e, 0.5);
        CHECK(c[0] == c[3] && c[0] > 0.7 && c[0] < 0.71);
        double f[4] = { 0.5, 0.5, 0.5, 0.5 };
        const double g[4] = { 0.5, 0.5, 0.5, 0.5 };
        mpt_anim_blend_rotation(f, g, 0.3);
        CHECK(f[0] == 0.5 && f[1] == 0.5 && f[2] == 0.5 && f[3] == 0.5);
    }
    // ---- the motion binding's refusals
    {
        const double rest_ok[MPT_ANIM_REST] = { 0, 0, 0, 0, 0, 0, 1, 1, 1, 1 };
        double base_ok[16] = { 0 };
        for (int d = 0; d < 4; d++) base_ok[5 * d] = 1.0;
        CHECK(mpt_motion_binding_rule(0.0, 1.0, nullptr, nullptr, nullptr, 0) == MPT_MOTION_OK && mpt_motion_binding_rule(0.0, 1.0, rest_ok, base_ok, nullptr, 0) == MPT_MOTION_OK);
        for (int what = 0; what < 6; what++) {
            std::vector<double> rest(rest_ok, rest_ok + MPT_ANIM_REST), base(base_ok, base_ok + 16);
            double offset = 0.0, speed = 1.0;
            MptMotionVerdict want = MPT_MOTION_NOT_FINITE;
            if (what == 0) offset = nan;
            if (what == 1) speed = inf;
            if (what == 2) { rest[0] = inf; want = MPT_MOTION_REST_NOT_FINITE; }
            if (what == 3) { rest[9] = nan; want = MPT_MOTION_REST_NOT_FINITE; }
            if (what == 4) { rest[6] = 0.0; want = MPT_MOTION_ZERO_ROTATION; }
            if (what == 5) { base[15] = inf; want = MPT_MOTION_BASE_NOT_FINITE; }
            for (size_t cap = 0; cap <= 80; cap += cap < 8 ? 1 : 24) {
                std::vector<char> why(cap, 'x');
                CHECK(mpt_motion_binding_rule(offset, speed, rest.data(), base.data(), cap ? why.data() : nullptr, cap) == want);
                if (cap) CHECK(std::memchr(why.data(), 0, cap) != nullptr);
                refusals++;
            }
        }
    }
    // ---- object clips: subsets of T, R, S on target 0
    for (int mask = 0; mask < 8; mask++)
        for (int round = 0; round < 6; round++) {
            Clip c;
            for (int path = MPT_ANIM_T; path <= MPT_ANIM_S; path++)
                if (mask >> path & 1) add_track(c, 0, path, 0);
            const int n = (int)(c.spec.size() / 4);
            c.spec.shrink_to_fit(); c.times.shrink_to_fit(); c.values.shrink_to_fit();
            CHECK(mpt_clip_rule(1, 0, n, c.spec.data(), c.times.data(), (int64_t)c.times.size(), c.values.data(), (int64_t)c.values.size(), nullptr, 0) == MPT_CLIP_OK);
            c.tracks.resize((size_t)n);
            mpt_anim_tracks(0, n, c.spec.data(), c.times.data(), c.tracks.data(), &c.t0, &c.t1);
            float q[4];
            quaternion(q);
            const double rest[MPT_ANIM_REST] = { unit(), unit(), unit(), q[0], q[1], q[2], q[3], 0.5 + unit(), 0.5 + unit(), 0.5 + unit() };
            double base[16], eye[16] = { 0 };
            for (int k = 0; k < 16; k++) base[k] = 2.0 * unit() - 1.0;
            for (int d = 0; d < 4; d++) eye[5 * d] = 1.0;
            const double tau = mpt_anim_local_time(c.t0 + 3.0 * unit() - 1.0, 0.0, 1.0, round % 2, c.t0, c.t1);
            double trs[MPT_ANIM_REST], trs2[MPT_ANIM_REST], W[16], L16[16], L[12];
            std::memcpy(trs, rest, sizeof trs); std::memcpy(trs2, rest, sizeof trs2);
            mpt_anim_motion(n, c.tracks.data(), c.times.data(), c.values.data(), tau, trs, base, W);
            mpt_anim_motion(n, c.tracks.data(), c.times.data(), c.values.data(), tau, trs2, eye, L16);
            mpt_anim_local(trs, L);
            for (int k = 0; k < 12; k++) CHECK(L16[k] == L[k]);             // under the identity the world is the local matrix ...
            CHECK(L16[12] == 0.0 && L16[13] == 0.0 && L16[14] == 0.0 && L16[15] == 1.0);
            for (int k = 0; k < 16; k++) CHECK(std::isfinite(W[k]));
            for (int r = 0; r < 4; r++)                                     // ... and under any base every row is the one expression
                CHECK(W[4 * r + 3] == ((base[4 * r] * L[3] + base[4 * r + 1] * L[7]) + base[4 * r + 2] * L[11]) + base[4 * r + 3]);
            if (mask == 0)
                for (int k = 0; k < MPT_ANIM_REST; k++) CHECK(trs[k] == rest[k]);
            worlds++;
        }
    {   // a W track, a second joint: no object clip
        const int32_t w[4] = { -1, MPT_ANIM_W, MPT_ANIM_STEP, 1 }, j1[4] = { 1, MPT_ANIM_T, MPT_ANIM_STEP, 1 };
        const float t[1] = { 0.0f }, v[3] = { 0.0f, 0.0f, 0.0f };
        CHECK(mpt_clip_rule(1, 0, 1, w, t, 1, v, 0, nullptr, 0) == MPT_CLIP_NO_TARGETS);
        CHECK(mpt_clip_rule(1, 0, 1, j1, t, 1, v, 3, nullptr, 0) == MPT_CLIP_TARGET);
    }
    std::printf("anim_blend_rule_check: %d blended poses, %d world matrices, %d refusals with a message buffer, %d failures\n", poses, worlds, refusals, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

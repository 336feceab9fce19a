// anim_rule_check.cpp -- the rule of keyframe animation (ptina_amd/csrc/anim_rule.h: the validation of a skeleton's and a clip's
// arrays, local time, the tracks, the hierarchy and the palette) exercised by a stand-alone program, so that it can run under the host
// sanitizers without a GPU and without loading anything into an interpreter:
//
//     c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/anim_rule_check.cpp -o anim_rule_check && ./anim_rule_check
//
// Random skeletons and clips in arrays that are exactly as long as the rule may read: every refusal at the first and the last place
// it can occur, with message buffers of every size (cut, terminated, never overrun); then whole poses at local times before, on,
// between and behind the keys, looped and clamped, with rigid joints: every palette must come out finite and -- rotations and
// translations only -- with orthonormal 3x3 parts.

#include "../ptina_amd/csrc/anim_rule.h"
#include <cstdlib>
#include <cstring>
#include <limits>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
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

struct Clip { std::vector<int32_t> spec; std::vector<float> times, values; };

// a clip over nj joints and nt targets: every (joint, path) with probability 1/2 -- only T and R where `rigid` -- and the weights
static Clip random_clip(int nj, int nt, bool rigid) {
    Clip c;
    auto add = [&](int target, int path) {
        const int interp = (int)rnd(3), nkeys = rnd(3) == 0 ? 1 : 1 + (int)rnd(33);
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
    };
    for (int j = 0; j < nj; j++)
        for (int path = MPT_ANIM_T; path <= (rigid ? MPT_ANIM_R : MPT_ANIM_S); path++)
            if (rnd(2)) add(j, path);
    if (nt > 0 && rnd(2)) add(-1, MPT_ANIM_W);
    return c;
}

static MptClipVerdict check(int nj, int nt, const Clip &c, char *why = nullptr, size_t cap = 0) {
    // copies of exactly the lengths given: a read past an end is the sanitizer's to find
    std::vector<int32_t> spec(c.spec); std::vector<float> times(c.times), values(c.values);
    return mpt_clip_rule(nj, nt, (int)(spec.size() / 4), spec.data(), times.data(), (int64_t)times.size(), values.data(), (int64_t)values.size(), why, cap);
}

int main() {
    int clips = 0, refusals = 0, poses = 0;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int round = 0; round < 60; round++) {
        const int nj = round % 3 == 0 ? 0 : 1 + (int)rnd(round % 5 == 0 ? MPT_DEFORM_MAX_JOINTS : 12), nt = round % 3 == 0 ? 1 + (int)rnd(MPT_DEFORM_MAX_TARGETS) : (int)rnd(4);
        const bool rigid = round % 2 == 0;
        // ---- the skeleton: a chain, a star or a random tree
        std::vector<int32_t> parents((size_t)nj), depth((size_t)nj);
        std::vector<double> rest((size_t)nj * MPT_ANIM_REST), ib((size_t)nj * 12);
        for (int j = 0; j < nj; j++) {
            parents[j] = j == 0 ? -1 : round % 4 == 0 ? j - 1 : round % 4 == 1 ? 0 : (int)rnd((unsigned)j + 1) - 1;
            float q[4];
            quaternion(q);
            double *r = rest.data() + (size_t)j * MPT_ANIM_REST;
            for (int k = 0; k < 3; k++) { r[k] = unit() - 0.5; r[7 + k] = rigid ? 1.0 : 0.5 + unit(); }
            for (int k = 0; k < 4; k++) r[3 + k] = q[k];
            const double bind[MPT_ANIM_REST] = { unit(), unit(), unit(), q[1], -q[0], q[3], -q[2], 1.0, 1.0, 1.0 };
            mpt_anim_local(bind, ib.data() + (size_t)j * 12);
        }
        if (nj > 0) {
            CHECK(mpt_skeleton_rule(nj, parents.data(), rest.data(), ib.data(), nullptr, 0) == MPT_SKELETON_OK);
            const int levels = mpt_anim_depths(nj, parents.data(), depth.data());
            CHECK(levels >= 0 && levels < nj && (round % 4 != 0 || levels == nj - 1) && (round % 4 != 1 || levels == (nj > 1)));
            for (int where = 0; where < 2; where++)
                for (int what = 0; what < 4; what++) {
                    std::vector<int32_t> p(parents); std::vector<double> r(rest), b(ib);
                    const int j = where ? nj - 1 : 0;
                    if (what == 0) p[j] = j;
                    if (what == 1) r[(size_t)j * MPT_ANIM_REST + (where ? 9 : 0)] = nan;
                    if (what == 2) b[(size_t)j * 12 + (where ? 11 : 0)] = inf;
                    if (what == 3) for (int k = 3; k < 7; k++) r[(size_t)j * MPT_ANIM_REST + k] = 0.0;
                    const MptSkeletonVerdict want = what == 0 ? MPT_SKELETON_PARENT : what == 3 ? MPT_SKELETON_ZERO_ROTATION : MPT_SKELETON_NOT_FINITE;
                    for (size_t cap = 0; cap <= 200; cap += cap < 8 ? 1 : 48) {
                        std::vector<char> why(cap, 'x');
                        CHECK(mpt_skeleton_rule(nj, p.data(), r.data(), b.data(), cap ? why.data() : nullptr, cap) == want);
                        if (cap) CHECK(std::memchr(why.data(), 0, cap) != nullptr);
                        if (cap >= 200) CHECK(!std::strncmp(why.data(), "skeleton: ", 10));
                        refusals++;
                    }
                }
        }
        CHECK(mpt_skeleton_rule(MPT_DEFORM_MAX_JOINTS + 1, parents.data(), rest.data(), ib.data(), nullptr, 0) == MPT_SKELETON_NJOINTS);
        CHECK(mpt_skeleton_rule(1, nullptr, rest.data(), ib.data(), nullptr, 0) == MPT_SKELETON_ARGS);
        // ---- the clip
        const Clip clip = random_clip(nj, nt, rigid);
        const int ntracks = (int)(clip.spec.size() / 4);
        CHECK(check(nj, nt, clip) == MPT_CLIP_OK);
        clips++;
        if (ntracks > 0)
            for (int where = 0; where < 2; where++) {
                const int r = where ? ntracks - 1 : 0;
                std::vector<MptAnimTrack> tr((size_t)ntracks);
                double t0, t1;
                mpt_anim_tracks(nt, ntracks, clip.spec.data(), clip.times.data(), tr.data(), &t0, &t1);
                const int nkeys = tr[r].nkeys, kf = mpt_anim_key_floats(tr[r].path, tr[r].interp, nt);
                const size_t last_time = (size_t)tr[r].time_at + (size_t)nkeys - 1, last_value = (size_t)tr[r].value_at + (size_t)nkeys * kf - 1;
                for (int what = 0; what < 9; what++) {
                    Clip c = clip;
                    MptClipVerdict want = MPT_CLIP_OK;
                    if (what == 0) { c.times[last_time] = nan; want = MPT_CLIP_TIME_NOT_FINITE; }
                    if (what == 1) { if (nkeys < 2) continue; c.times[last_time] = c.times[last_time - 1]; want = MPT_CLIP_TIME_ORDER; }
                    if (what == 2) { c.values[last_value] = where ? -inf : nan; want = MPT_CLIP_VALUE_NOT_FINITE; }
                    if (what == 3) { c.spec[4 * r] = tr[r].path == MPT_ANIM_W ? 0 : nj; want = MPT_CLIP_TARGET; }
                    if (what == 4) { c.spec[4 * r + 1] = 4; want = MPT_CLIP_KIND; }
                    if (what == 5) { c.spec[4 * r + 2] = -1; want = MPT_CLIP_KIND; }
                    if (what == 6) { c.spec[4 * r + 3] = 0; want = MPT_CLIP_NKEYS; }
                    if (what == 7) { c.times.pop_back(); want = MPT_CLIP_ARGS; }
                    if (what == 8) {
                        if (tr[r].path != MPT_ANIM_R) continue;
                        const size_t q = (size_t)tr[r].value_at + (size_t)(nkeys - 1) * kf + (tr[r].interp == MPT_ANIM_CUBICSPLINE ? 4 : 0);
                        for (int e = 0; e < 4; e++) c.values[q + e] = e % 2 ? -0.0f : 0.0f;
                        want = MPT_CLIP_ZERO_ROTATION;
                    }
                    for (size_t cap = 0; cap <= 200; cap += cap < 8 ? 1 : 48) {
                        std::vector<char> why(cap, 'x');
                        const MptClipVerdict got = check(nj, nt, c, cap ? why.data() : nullptr, cap);
                        CHECK(got == want || (what == 7 && got != MPT_CLIP_OK));      // (a time short: the last track's refusal, or the lengths')
                        if (cap) CHECK(std::memchr(why.data(), 0, cap) != nullptr);
                        if (cap >= 200) CHECK(!std::strncmp(why.data(), "clip: ", 6));
                        refusals++;
                    }
                }
                Clip twice = clip;                                            // the same (target, path) again, behind everything
                twice.spec.insert(twice.spec.end(), { clip.spec[4 * r], clip.spec[4 * r + 1], MPT_ANIM_STEP, 1 });
                twice.times.push_back(0.0f);
                for (int e = 0; e < mpt_anim_components(clip.spec[4 * r + 1], nt); e++) twice.values.push_back(1.0f);
                CHECK(check(nj, nt, twice) == MPT_CLIP_DUPLICATE);
            }
        if (nt == 0) {
            Clip w;
            w.spec = { -1, MPT_ANIM_W, MPT_ANIM_STEP, 1 }; w.times = { 0.0f };
            CHECK(check(nj, 0, w) == MPT_CLIP_NO_TARGETS);
        }
        // ---- whole poses
        std::vector<MptAnimTrack> tr((size_t)ntracks);
        double t0, t1;
        mpt_anim_tracks(nt, ntracks, clip.spec.data(), clip.times.data(), tr.data(), &t0, &t1);
        CHECK(t0 <= t1);
        std::vector<double> pose((size_t)nt + (size_t)nj * 12);
        const std::vector<float> times(clip.times), values(clip.values);
        for (int q = 0; q < 24; q++) {
            const int loop = q % 2;
            const double picks[6] = { t0, t1, t0 - 1.0 - unit(), t1 + 1.0 + unit(), t0 + unit() * (t1 - t0), times.empty() ? 0.0 : (double)times[rnd((unsigned)times.size())] };
            const double offset = q < 12 ? 0.0 : unit(), speed = q < 12 ? 1.0 : q % 3 == 0 ? 0.0 : 2.0 * unit() - 1.0;
            const double tau = mpt_anim_local_time(picks[q % 6] + offset, offset, speed, loop, t0, t1);
            if (loop && t1 > t0) CHECK(tau >= t0 - 1e-9 && tau <= t1 + 1e-9);
            for (double &x : pose) x = std::numeric_limits<double>::quiet_NaN();
            mpt_anim_pose(nj, nt, parents.data(), rest.data(), ib.data(), ntracks, tr.data(), times.data(), values.data(), tau, pose.data());
            for (double x : pose) CHECK(std::isfinite(x));
            if (rigid)
                for (int j = 0; j < nj; j++) {                              // rotations and shifts only: every palette matrix is a rigid motion
                    const double *P = pose.data() + nt + (size_t)j * 12;
                    for (int a = 0; a < 3; a++)
                        for (int b = 0; b < 3; b++) {
                            const double dot = P[a] * P[b] + P[4 + a] * P[4 + b] + P[8 + a] * P[8 + b];
                            CHECK(std::fabs(dot - (a == b)) < 1e-4);          // (keys and rest rotations are unit to f32 rounding, a chain of 256 deep)
                        }
                }
            poses++;
        }
    }
    // the key search on its own: every tau on and between the keys of a long track finds its interval
    std::vector<float> T(33);
    for (int k = 0; k < 33; k++) T[k] = 0.25f * (float)k;
    for (int k = 0; k < 33; k++)
        for (int part = 0; part < 2; part++) {
            int at; double dt, u;
            const double tau = (double)T[k] + 0.125 * part;
            const int between = mpt_anim_key(T.data(), 33, tau, &at, &dt, &u);
            if (k == 0 && part == 0) CHECK(!between && at == 0);
            else if (k == 32) CHECK(!between && at == 32);
            else CHECK(between && at == k && dt == 0.25 && u == 0.5 * part);
        }
    { int at; double dt, u; CHECK(!mpt_anim_key(T.data(), 33, std::numeric_limits<double>::quiet_NaN(), &at, &dt, &u) && at == 0); }
    std::printf("anim_rule_check: %d clips, %d refusals with a message buffer, %d poses, %d failures\n", clips, refusals, poses, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

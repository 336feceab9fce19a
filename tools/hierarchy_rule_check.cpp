// hierarchy_rule_check.cpp -- the rule of parent bindings (the additions of DESIGN.md section 3.17.3 to ptina_amd/csrc/anim_rule.h)
// exercised by a stand-alone program, so that it can run under the host sanitizers without a GPU and without loading anything into
// an interpreter:
//
//     c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/hierarchy_rule_check.cpp -o hierarchy_rule_check && ./hierarchy_rule_check
//
// Arrays that are exactly as long as the rule may read.  Held: the product against the identity and against a hand sum; a chain of one
// link is the link's local matrix and a chain of two is one product, bit for bit; a joint's entry with an identity palette changes
// nothing; a motion-bound link is mpt_anim_motion's matrix; chains 64 deep stay finite; every refusal of mpt_parent_rule with message
// buffers of every size, on tables of 1 to 66 objects, and a refusal changes nothing it was given.

#include "../ptina_amd/csrc/anim_rule.h"
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd(unsigned n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33) % n;
}
static double unit() { return ((double)rnd(1u << 24) + 0.5) / (double)(1u << 24); }

static std::vector<double> matrix(bool affine) {
    std::vector<double> m(16);
    for (auto &x : m) x = 2.0 * unit() - 1.0;
    if (affine) { m[12] = m[13] = m[14] = 0.0; m[15] = 1.0; }
    return m;
}

static bool same(const double *a, const double *b, int n) { return std::memcmp(a, b, (size_t)n * sizeof(double)) == 0; }

int main() {
    int products = 0, chains = 0, refusals = 0;
    const double eye[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    // ---- the product
    for (int k = 0; k < 200; k++) {
        const std::vector<double> A = matrix(k & 1), B = matrix(k & 2);
        std::vector<double> W(16), V(16);
        mpt_mat4_mul(A.data(), eye, W.data());
        CHECK(same(W.data(), A.data(), 16));
        mpt_mat4_mul(eye, B.data(), W.data());
        CHECK(same(W.data(), B.data(), 16));
        mpt_mat4_mul(A.data(), B.data(), W.data());
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                volatile double s = A[4 * r] * B[c];
                s = s + A[4 * r + 1] * B[4 + c];
                s = s + A[4 * r + 2] * B[8 + c];
                s = s + A[4 * r + 3] * B[12 + c];
                V[4 * r + c] = s;
            }
        CHECK(same(W.data(), V.data(), 16));
        // a joint: the inner product first; the identity entry changes nothing
        std::vector<double> M(A.begin(), A.begin() + 12), M4(A), X(16), J(16);
        M4[12] = M4[13] = M4[14] = 0.0; M4[15] = 1.0;
        mpt_mat4_mul(M4.data(), B.data(), X.data());
        mpt_mat4_mul(W.data(), X.data(), V.data());
        mpt_hier_world(W.data(), M.data(), B.data(), J.data());
        CHECK(same(J.data(), V.data(), 16));
        mpt_hier_world(W.data(), eye, B.data(), J.data());
        mpt_hier_world(W.data(), nullptr, B.data(), V.data());
        CHECK(same(J.data(), V.data(), 16));
        products++;
    }
    // ---- chains: static links, links on joints, motion-bound links
    const int32_t spec[8] = { 0, MPT_ANIM_T, MPT_ANIM_LINEAR, 2, 0, MPT_ANIM_S, MPT_ANIM_STEP, 1 };
    const std::vector<float> times = { 0.0f, 2.0f, 0.5f }, values = { 0.0f, 1.0f, 2.0f, 4.0f, -1.0f, 0.5f, 2.0f, 0.5f, 1.5f };
    CHECK(mpt_clip_rule(1, 0, 2, spec, times.data(), 3, values.data(), 9, nullptr, 0) == MPT_CLIP_OK);
    std::vector<MptAnimTrack> tracks(2);
    double t0, t1;
    mpt_anim_tracks(0, 2, spec, times.data(), tracks.data(), &t0, &t1);
    const std::vector<double> rest = { 0.1, 0.2, 0.3, 0.0, 0.6, 0.0, 0.8, 1.0, 1.0, 1.0 };
    for (int n = 1; n <= MPT_HIER_MAX_DEPTH + 1; n += (n < 4 ? 1 : 15)) {
        std::vector<std::vector<double>> locals, pals;
        std::vector<MptHierLink> links((size_t)n);
        for (int k = 0; k < n; k++) {
            locals.push_back(matrix(k % 3 != 2));
            pals.push_back(std::vector<double>(12));
            for (auto &x : pals.back()) x = 2.0 * unit() - 1.0;
        }
        for (int k = 0; k < n; k++) {
            MptHierLink &ln = links[k];
            ln = MptHierLink{};
            ln.local = locals[k].data(); ln.ntracks = -1;
            if (k > 0 && k % 2 == 0) ln.pal = pals[k].data();
            if (k % 4 == 1) {
                ln.ntracks = 2; ln.tracks = tracks.data(); ln.times = times.data(); ln.values = values.data(); ln.t0 = t0; ln.t1 = t1;
                ln.offset = 0.25; ln.speed = 1.5; ln.loop = k & 2; ln.rest = rest.data();
            }
        }
        std::vector<double> world(16), by_hand(16), L(16), W(16), trs(MPT_ANIM_REST);
        const double t = 0.75;
        mpt_hier_chain(n, links.data(), t, world.data());
        for (int k = 0; k < n; k++) {
            const MptHierLink &ln = links[k];
            if (ln.ntracks >= 0) {
                trs = rest;
                mpt_anim_motion(2, tracks.data(), times.data(), values.data(), mpt_anim_local_time(t, ln.offset, ln.speed, ln.loop, t0, t1), trs.data(), ln.local, L.data());
            } else
                L = locals[k];
            if (k == 0) { by_hand = L; continue; }
            W = by_hand;
            mpt_hier_world(W.data(), ln.pal, L.data(), by_hand.data());
        }
        CHECK(same(world.data(), by_hand.data(), 16));
        for (double x : world) CHECK(std::isfinite(x));
        if (n == 1) CHECK(same(world.data(), locals[0].data(), 16));
        chains++;
    }
    // ---- the refusals of a binding, on tables of every small size, with message buffers of every size
    for (int nobj = 1; nobj <= MPT_HIER_MAX_DEPTH + 2; nobj++) {
        std::vector<int32_t> parents((size_t)nobj), instance((size_t)nobj, 0), njoints((size_t)nobj, 0);
        for (int o = 0; o < nobj; o++) parents[o] = o - 1;             // one chain: object o has depth o
        const std::vector<int32_t> before = parents;
        for (size_t room = 0; room <= 200; room += (room < 4 ? 1 : 49)) {
            std::vector<char> why(room);
            char *w = room ? why.data() : nullptr;
            auto rule = [&](int obj, int parent, int joint) {
                const MptParentVerdict v = mpt_parent_rule(nobj, parents.data(), instance.data(), njoints.data(), obj, parent, joint, w, room);
                if (room) CHECK(std::strlen(w) < room);
                if (room >= 2) CHECK((v == MPT_PARENT_OK) == (w[0] == 0));
                refusals += v != MPT_PARENT_OK;
                return v;
            };
            CHECK(rule(-1, 0, -1) == MPT_PARENT_UNKNOWN && rule(nobj, 0, -1) == MPT_PARENT_UNKNOWN && rule(0, nobj, -1) == MPT_PARENT_UNKNOWN);
            CHECK(rule(0, -2, -1) == MPT_PARENT_UNKNOWN);
            CHECK(rule(0, 0, -1) == MPT_PARENT_CYCLE && rule(0, nobj - 1, -1) == MPT_PARENT_CYCLE);
            CHECK(rule(nobj - 1, -1, -1) == MPT_PARENT_OK && rule(nobj - 1, -1, 5) == MPT_PARENT_OK);
            if (nobj < 2) continue;
            CHECK(rule(nobj - 1, 0, 0) == MPT_PARENT_NO_SKIN);
            CHECK(rule(nobj - 1, 0, -2) == MPT_PARENT_JOINT);
            njoints[0] = 3;
            CHECK(rule(nobj - 1, 0, 3) == MPT_PARENT_JOINT && rule(nobj - 1, 0, 2) == MPT_PARENT_OK && rule(nobj - 1, 0, -1) == MPT_PARENT_OK);
            njoints[0] = 0;
            instance[nobj - 1] = 1;
            CHECK(rule(nobj - 1, 0, -1) == MPT_PARENT_INSTANCE);
            instance[nobj - 1] = 0;
            instance[0] = 1;
            CHECK(rule(nobj - 1, 0, -1) == MPT_PARENT_INSTANCE);
            instance[0] = 0;
            // the table is one chain nobj - 1 deep: the last link holds while that is within the cap
            CHECK((rule(nobj - 1, nobj - 2, -1) == MPT_PARENT_OK) == (nobj - 1 <= MPT_HIER_MAX_DEPTH));
            if (nobj >= 3) {
                // two chains, objects 0 .. h - 1 and h .. nobj - 1: hanging the second under the end of the first gives nobj - 1 again
                const int h = nobj / 2;
                parents[h] = -1;
                CHECK((rule(h, h - 1, -1) == MPT_PARENT_OK) == (nobj - 1 <= MPT_HIER_MAX_DEPTH));
                CHECK(rule(h, 0, -1) == MPT_PARENT_OK || nobj - h > MPT_HIER_MAX_DEPTH);
                parents[h] = h - 1;
            }
            CHECK(parents == before);
        }
    }
    std::printf("hierarchy_rule_check: %d products, %d chains, %d refusals, %d failures\n", products, chains, refusals, failures);
    return failures ? 1 : 0;
}

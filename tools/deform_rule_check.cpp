// deform_rule_check.cpp -- the pure host pieces of mesh deformation (ptina_amd/csrc/deform_rule.h: the run table of a deform launch
// and the validation of a skin's arrays) exercised by a stand-alone program, so that they can run under the host sanitizers
// without a GPU and without loading anything into an interpreter:
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/deform_rule_check.cpp -o deform_rule_check && ./deform_rule_check
//
// The plan over layouts with empty objects, clean objects and runs that end exactly on a chunk boundary, with output tables of
// every capacity from none to ample (never written past `cap`); the skin check over arrays that are exactly as long as it may
// read, each refusal at the first and the last element, with message buffers of every size (cut, terminated, never overrun).

#include "../ptina_amd/csrc/deform_rule.h"
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd(unsigned n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33) % n;
}

int main() {
    const int C = MPT_DEFORM_CHUNK;
    const int sizes[] = { 0, 1, 3, 63, 255, 256, C - 1, C, C + 1, 2 * C, 5 * C + 21 };
    int plans = 0;
    for (int round = 0; round < 400; round++) {
        const int nobj = (int)rnd(9);
        std::vector<int32_t> corners((size_t)nobj), dirty((size_t)nobj);
        for (int o = 0; o < nobj; o++) { corners[o] = sizes[rnd(sizeof sizes / sizeof *sizes)]; dirty[o] = (int32_t)rnd(2); }
        const bool flags = rnd(3) != 0;
        // the answer, restated
        std::vector<int32_t> want_obj; std::vector<int64_t> want_block;
        int64_t at = 0;
        for (int o = 0; o < nobj; o++) {
            if (corners[o] == 0 || (flags && !dirty[o])) continue;
            want_obj.push_back(o); want_block.push_back(at);
            at += (corners[o] + C - 1) / C;
        }
        for (int cap = 0; cap <= nobj + 1; cap++) {
            // tables of exactly `cap` entries on the heap: an entry written past them is the sanitizer's to report
            std::vector<int32_t> run_obj((size_t)cap, -7); std::vector<int64_t> run_block((size_t)cap, -7);
            int64_t blocks = -1;
            const int nr = mpt_deform_plan_of(nobj ? corners.data() : nullptr, flags ? dirty.data() : nullptr, nobj, cap ? run_obj.data() : nullptr,
                                              cap ? run_block.data() : nullptr, cap, &blocks);
            plans++;
            CHECK(nr == (int)want_obj.size() && blocks == at);
            for (int r = 0; r < cap; r++) {
                if (r < nr) CHECK(run_obj[r] == want_obj[r] && run_block[r] == want_block[r]);
                else CHECK(run_obj[r] == -7 && run_block[r] == -7);
            }
        }
        CHECK(mpt_deform_plan_of(nobj ? corners.data() : nullptr, nullptr, nobj, nullptr, nullptr, 0, nullptr) >= 0);
    }
    {
        const int32_t neg[2] = { 5, -1 };
        CHECK(mpt_deform_plan_of(neg, nullptr, 2, nullptr, nullptr, 0, nullptr) == -1);
        CHECK(mpt_deform_plan_of(nullptr, nullptr, 1, nullptr, nullptr, 0, nullptr) == -1);
        CHECK(mpt_deform_plan_of(nullptr, nullptr, -1, nullptr, nullptr, 0, nullptr) == -1);
        std::vector<int32_t> huge(1100, 2147483647);                      // 1100 x 2^21 blocks: past 31 bits
        CHECK(mpt_deform_plan_of(huge.data(), nullptr, (int)huge.size(), nullptr, nullptr, 0, nullptr) == -1);
    }

    int checks = 0;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int64_t n : { (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)257 })
        for (int nj : { -1, 0, 1, 5, MPT_DEFORM_MAX_JOINTS, MPT_DEFORM_MAX_JOINTS + 1 }) {
            std::vector<uint16_t> joints((size_t)n * 4); std::vector<float> weights((size_t)n * 4);
            const bool nj_ok = nj >= 1 && nj <= MPT_DEFORM_MAX_JOINTS;
            for (size_t k = 0; k < joints.size(); k++) { joints[k] = (uint16_t)(nj_ok ? rnd((unsigned)nj) : 0); weights[k] = 0.25f * (float)rnd(5); }
            for (int what = 0; what < 5; what++)                              // nothing wrong | index | NaN | infinity | negative
                for (int where = 0; where < 2; where++) {
                    if (what && (n == 0 || !nj_ok)) continue;
                    std::vector<uint16_t> j = joints; std::vector<float> w = weights;
                    const size_t at = where ? j.size() - 1 : 0;
                    if (what == 1) j[at] = (uint16_t)nj;
                    if (what == 2) w[at] = nan;
                    if (what == 3) w[at] = where ? -inf : inf;
                    if (what == 4) w[at] = -0.5f;
                    const MptSkinVerdict want = !nj_ok ? MPT_SKIN_NJOINTS : what == 0 ? MPT_SKIN_OK : what == 1 ? MPT_SKIN_INDEX
                                              : what == 4 ? MPT_SKIN_NEGATIVE : MPT_SKIN_NOT_FINITE;
                    CHECK(mpt_skin_rule(j.data(), w.data(), n, nj, nullptr, 0) == want);
                    CHECK(mpt_skin_rule(j.data(), w.data(), n, nj, nullptr, 64) == want);
                    for (size_t cap = 0; cap <= 200; cap += cap < 8 ? 1 : 37) {
                        std::vector<char> why(cap, 'x');
                        CHECK(mpt_skin_rule(j.data(), w.data(), n, nj, cap ? why.data() : nullptr, cap) == want);
                        checks++;
                        if (!cap) continue;
                        CHECK(std::memchr(why.data(), 0, cap) != nullptr);
                        if (want == MPT_SKIN_OK) CHECK(why[0] == 0);
                        else if (cap >= 200) {
                            CHECK(!std::strncmp(why.data(), "skin: ", 6));
                            char idx[48];
                            std::snprintf(idx, sizeof idx, "[%lld][%lld]", (long long)(at / 4), (long long)(at % 4));
                            if (want != MPT_SKIN_NJOINTS) CHECK(std::strstr(why.data(), idx) != nullptr);
                            CHECK(std::strstr(why.data(), want == MPT_SKIN_INDEX ? "joints[" : want == MPT_SKIN_NJOINTS ? "njoints" : "weights[") != nullptr);
                        }
                    }
                }
        }
    CHECK(mpt_skin_rule(nullptr, nullptr, 1, 4, nullptr, 0) == MPT_SKIN_ARGS);
    CHECK(mpt_skin_rule(nullptr, nullptr, -1, 4, nullptr, 0) == MPT_SKIN_ARGS);
    CHECK(mpt_skin_rule(nullptr, nullptr, 0, 4, nullptr, 0) == MPT_SKIN_OK);
    std::printf("deform_rule_check: %d plans, %d skin checks with a message buffer, %d failures\n", plans, checks, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

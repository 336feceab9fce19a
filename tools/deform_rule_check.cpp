// deform_rule_check.cpp -- the pure host piece of mesh deformation (ptina_amd/csrc/deform_rule.h: the validation of a skin's arrays;
// the run table of a deform launch is tools/run_table_check.cpp's) exercised by a stand-alone program, so that it can run under the
// host sanitizers without a GPU and without loading anything into an interpreter:
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/deform_rule_check.cpp -o deform_rule_check && ./deform_rule_check
//
// The skin check over arrays that are exactly as long as it may read, each refusal at the first and the last element, with message
// buffers of every size (cut, terminated, never overrun).

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
    std::printf("deform_rule_check: %d skin checks with a message buffer, %d failures\n", checks, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

// refit_rule_check.cpp -- the pure host pieces of mpt_refit_tree (ptina_amd/csrc/refit_rule.h: the permission rule and the
// growth figure) exercised by a stand-alone program, so that they can run under the host sanitizers without a GPU and
// without loading anything into an interpreter:
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/refit_rule_check.cpp -o refit_rule_check && ./refit_rule_check
//
// Every verdict over every state and a range of face counts, with message buffers of every size from none to ample (the
// words must be cut, terminated and never written past the buffer), and the growth arithmetic at its edges.

#include "../ptina_amd/csrc/refit_rule.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static bool ends_with(const char *s, const char *tail) {
    const size_t a = std::strlen(s), b = std::strlen(tail);
    return a >= b && !std::strcmp(s + a - b, tail);
}

int main() {
    const int faces[] = { 0, 1, 2, 33, 34, 8192, 8193, 2147483647, -1 };
    int calls = 0;
    for (int state = -2; state <= MPT_TOPO_STATES + 1; state++)
        for (int built : faces)
            for (int dev = 0; dev < 2; dev++)
                for (int now : faces) {
                    MptRefitVerdict want = MPT_REFIT_OK;
                    if (state <= MPT_TOPO_NONE || state >= MPT_TOPO_STATES) want = MPT_REFIT_NO_TREE;
                    else if (state == MPT_TOPO_OPTION) want = MPT_REFIT_OPTION;
                    else if (state == MPT_TOPO_BUILD_FAILED) want = MPT_REFIT_BUILD_FAILED;
                    else if (!dev) want = MPT_REFIT_HOST_BUILD;
                    else if (now != built) want = MPT_REFIT_FACES;
                    CHECK(mpt_refit_rule(state, built, dev, now, nullptr, 0) == want);
                    CHECK(mpt_refit_rule(state, built, dev, now, nullptr, 64) == want);
                    for (size_t cap = 0; cap <= 200; cap += cap < 8 ? 1 : 37) {
                        // the buffer is exactly `cap` bytes of the heap: a byte written past it is the sanitizer's to report
                        std::vector<char> why(cap, 'x');
                        CHECK(mpt_refit_rule(state, built, dev, now, cap ? why.data() : nullptr, cap) == want);
                        calls++;
                        if (!cap) continue;
                        CHECK(std::memchr(why.data(), 0, cap) != nullptr);
                        if (want == MPT_REFIT_OK) CHECK(why[0] == 0);
                        else if (cap >= 200) {
                            CHECK(ends_with(why.data(), "call build_tree()"));
                            if (want == MPT_REFIT_FACES) {
                                char both[64];
                                std::snprintf(both, sizeof both, "%d faces, the tree was built for %d", now, built);
                                CHECK(std::strstr(why.data(), both) != nullptr);
                            }
                        }
                    }
                }
    CHECK(mpt_refit_growth_of(0, 0) == 1.0);
    CHECK(mpt_refit_growth_of(0, UINT64_MAX) == 1.0);
    CHECK(mpt_refit_growth_of(1, 0) == 0.0);
    CHECK(mpt_refit_growth_of(UINT64_MAX, UINT64_MAX) == 1.0);
    CHECK(mpt_refit_growth_of((uint64_t)1 << 40, (uint64_t)3 << 39) == 1.5);
    CHECK(std::isfinite(mpt_refit_growth_of(1, UINT64_MAX)));
    for (uint64_t a = 1; a < ((uint64_t)1 << 62); a = a * 3 + 1)
        for (uint64_t b = 1; b < ((uint64_t)1 << 62); b = b * 5 + 2) {
            const double g = mpt_refit_growth_of(a, b);
            CHECK(g > 0.0 && std::isfinite(g) && (g > 1.0) == ((double)b > (double)a));
        }
    std::printf("refit_rule_check: %d rule calls with a message buffer, %d failures\n", calls, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

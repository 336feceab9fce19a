// run_table_check.cpp -- the run table of a launch (ptina_amd/csrc/run_table.h: the plan behind mpt_deform_plan and mpt_subdiv_plan,
// and as the launches take it) exercised by a stand-alone program, so that it can run under the host sanitizers without a GPU and
// without loading anything into an interpreter:
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/run_table_check.cpp -o run_table_check && ./run_table_check
//
// Over the chunks of deform.hip and subdiv.hip and two more: layouts with empty items, clean items and runs that end exactly on a
// chunk boundary, against the answer restated, with output tables of every capacity from none to ample on the heap (never written
// past `cap`); the table of runs a launch uploads, exactly as long as the items; the arguments that name no launch.

#include "../ptina_amd/csrc/run_table.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd(unsigned n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33) % n;
}

int main() {
    int plans = 0;
    for (const int C : { 1, MPT_SUBDIV_CHUNK, 1000, MPT_DEFORM_CHUNK }) {
        const int sizes[] = { 0, 1, 3, 63, 255, 256, C - 1, C, C + 1, 2 * C, 9600, 5 * C + 21 };
        for (int round = 0; round < 400; round++) {
            const int n = (int)rnd(9);
            std::vector<int32_t> items((size_t)n), dirty((size_t)n);
            for (int o = 0; o < n; o++) { items[o] = sizes[rnd(sizeof sizes / sizeof *sizes)]; dirty[o] = (int32_t)rnd(2); }
            const bool flags = rnd(3) != 0;
            // the answer, restated
            std::vector<int32_t> want_item; std::vector<int64_t> want_block;
            int64_t at = 0;
            for (int o = 0; o < n; o++) {
                if (items[o] == 0 || (flags && !dirty[o])) continue;
                want_item.push_back(o); want_block.push_back(at);
                at += (items[o] + C - 1) / C;
            }
            const int32_t *ip = n ? items.data() : nullptr, *dp = flags ? dirty.data() : nullptr;
            for (int cap = 0; cap <= n + 1; cap++) {
                // tables of exactly `cap` entries on the heap: an entry written past them is the sanitizer's to report
                std::vector<int32_t> run_item((size_t)cap, -7); std::vector<int64_t> run_block((size_t)cap, -7);
                int64_t blocks = -1;
                const int nr = mpt_run_plan_of(ip, dp, n, C, cap ? run_item.data() : nullptr, cap ? run_block.data() : nullptr, cap, &blocks);
                plans++;
                CHECK(nr == (int)want_item.size() && blocks == at);
                for (int r = 0; r < cap; r++) {
                    if (r < nr) CHECK(run_item[r] == want_item[r] && run_block[r] == want_block[r]);
                    else CHECK(run_item[r] == -7 && run_block[r] == -7);
                }
            }
            CHECK(mpt_run_plan_of(ip, nullptr, n, C, nullptr, nullptr, 0, nullptr) >= 0);
            // as a launch takes it: a run per item at the most
            std::vector<MptRun> runs((size_t)n, MptRun{ -7, -7 });
            int blocks = -1;
            const int nr = mpt_run_plan_into(ip, dp, n, C, runs.data(), &blocks);
            plans++;
            CHECK(nr == (int)want_item.size() && blocks == (int)at);
            for (int r = 0; r < n; r++) {
                if (r < nr) CHECK(runs[r].item == want_item[r] && runs[r].block == (int32_t)want_block[r]);
                else CHECK(runs[r].item == -7 && runs[r].block == -7);
            }
        }
        const int32_t neg[2] = { 5, -1 };
        CHECK(mpt_run_plan_of(neg, nullptr, 2, C, nullptr, nullptr, 0, nullptr) == -1);
        CHECK(mpt_run_plan_of(nullptr, nullptr, 1, C, nullptr, nullptr, 0, nullptr) == -1);
        CHECK(mpt_run_plan_of(nullptr, nullptr, -1, C, nullptr, nullptr, 0, nullptr) == -1);
        CHECK(mpt_run_plan_of(neg, nullptr, 1, 0, nullptr, nullptr, 0, nullptr) == -1);
        // past 31 bits of blocks: C + 1 items of 2^31 - 1 are more than 2^31 - 1 chunks of C, one of them is not
        std::vector<int32_t> huge((size_t)C + 1, 2147483647);
        int64_t blocks = -1;
        CHECK(mpt_run_plan_of(huge.data(), nullptr, C + 1, C, nullptr, nullptr, 0, &blocks) == -1 && blocks == -1);
        CHECK(mpt_run_plan_of(huge.data(), nullptr, 1, C, nullptr, nullptr, 0, &blocks) == 1 && blocks == (2147483647LL + C - 1) / C);
        std::vector<MptRun> runs((size_t)C + 1);
        int b = 0;
        CHECK(mpt_run_plan_into(huge.data(), nullptr, C + 1, C, runs.data(), &b) == -1);
    }
    std::printf("run_table_check: %d plans, %d failures\n", plans, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}

// run_table.h -- the run table of a launch whose blocks each lie in one row of a table (mpt_types.h MptRun): the plan that makes it,
// a pure function of the host side, and the lookup a block of the launch does in it.  deform.hip and subdiv.hip launch by it
// (scene_deform.cpp, scene_subdiv.cpp; the C ABI has the plan as mpt_deform_plan and mpt_subdiv_plan, each with its chunk), and
// compose.hip's partial launch looks its runs of output workgroups up the same way (their plan is mpt_compose_plan, another rule).
// Plain C++17 with nothing of HIP outside the guarded block at the end and no context (as refit_rule.h): tools/run_table_check.cpp
// runs the plan under the host sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include "mpt_types.h"         // MptRun (plain structures and constants)

// The blocks of one launch: every item of the table with a count whose flag is set (dirty null: all) takes ceil(count / chunk)
// consecutive blocks, in table order, so a block lies in exactly one item.  An item that sits a launch out has a count of 0 there.
// put(r, item, block) is handed run r.  The sum of the blocks goes to *blocks (may be null; an int holds it).  Returns the number
// of runs; -1 for arguments that name no launch (a negative count, no chunk, more than 2^31 - 1 blocks).
template <class Put, class Blocks>
inline int mpt_run_plan_each(const int32_t *items, const int32_t *dirty, int n, int chunk, Put put, Blocks *blocks) {
    if (n < 0 || chunk < 1 || (n > 0 && !items)) return -1;
    int nr = 0;
    long long at = 0;
    for (int o = 0; o < n; o++) {
        if (items[o] < 0) return -1;
        if (items[o] == 0 || (dirty && !dirty[o])) continue;
        put(nr++, o, at);
        at += ((long long)items[o] + chunk - 1) / chunk;
    }
    if (at > 0x7fffffffLL) return -1;
    if (blocks) *blocks = (Blocks)at;
    return nr;
}

// ... as the C ABI hands it out: the first `cap` runs go to run_item / run_block (either may be null)
inline int mpt_run_plan_of(const int32_t *items, const int32_t *dirty, int n, int chunk, int32_t *run_item, int64_t *run_block, int cap,
                           int64_t *blocks) {
    return mpt_run_plan_each(items, dirty, n, chunk, [&](int r, int item, long long at) {
        if (r >= cap) return;
        if (run_item) run_item[r] = item;
        if (run_block) run_block[r] = at;
    }, blocks);
}

// ... and as a launch takes it: runs[n] (there is at most a run per item) as they are uploaded, and the launch's blocks
inline int mpt_run_plan_into(const int32_t *items, const int32_t *dirty, int n, int chunk, MptRun *runs, int *blocks) {
    return mpt_run_plan_each(items, dirty, n, chunk, [&](int r, int item, long long at) { runs[r] = { item, (int32_t)at }; }, blocks);
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

// the run this block belongs to (uniform): the last one that begins at or before it
static __device__ __forceinline__ int mpt_run_of(const MptRun *__restrict__ runs, int nruns) {
    int a = 0, b = nruns - 1;
    while (a < b) { const int m = (a + b + 1) >> 1; if (runs[m].block <= (int)blockIdx.x) a = m; else b = m - 1; }
    return a;
}
#endif

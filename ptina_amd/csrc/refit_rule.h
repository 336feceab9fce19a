// refit_rule.h -- the two pure pieces of mpt_refit_tree: when a refit is allowed, and the growth figure it returns.  Plain C++17
// with nothing of HIP and no context (as mpt_options.h), so that a stand-alone program can run them under a sanitizer
// (tools/refit_rule_check.cpp); the C ABI has them as mpt_refit_allowed and mpt_refit_growth.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

// what became of the topology the node records hold
enum MptTopoState {
    MPT_TOPO_NONE = 0,        // no tree was ever built
    MPT_TOPO_HELD,            // the records hold the topology of the last successful mpt_build_tree
    MPT_TOPO_OPTION,          // ... until an option that steers the build was set
    MPT_TOPO_BUILD_FAILED,    // ... until a later build failed (it may have replaced or half-written the records)
    MPT_TOPO_STATES
};

enum MptRefitVerdict { MPT_REFIT_OK = 0, MPT_REFIT_NO_TREE, MPT_REFIT_OPTION, MPT_REFIT_BUILD_FAILED, MPT_REFIT_HOST_BUILD, MPT_REFIT_FACES };

// May the records built for `built_faces` faces (by the device build: built_on_device != 0) be fitted to a model of `nfaces`
// faces?  A refusal writes its words to `why` (always terminated; every one ends by naming build_tree()).
inline MptRefitVerdict mpt_refit_rule(int state, int built_faces, int built_on_device, int nfaces, char *why, size_t why_size) {
    auto say = [&](MptRefitVerdict v, const char *fmt, int a, int b) {
        if (why && why_size) snprintf(why, why_size, fmt, a, b);
        return v;
    };
    if (why && why_size) why[0] = 0;
    if (state <= MPT_TOPO_NONE || state >= MPT_TOPO_STATES)
        return say(MPT_REFIT_NO_TREE, "refit: no tree was ever built: call build_tree()", 0, 0);
    if (state == MPT_TOPO_OPTION)
        return say(MPT_REFIT_OPTION, "refit: an option that steers the tree build was set since the tree was built: call build_tree()", 0, 0);
    if (state == MPT_TOPO_BUILD_FAILED)
        return say(MPT_REFIT_BUILD_FAILED, "refit: the last tree build failed and left no tree to fit: call build_tree()", 0, 0);
    if (!built_on_device)
        return say(MPT_REFIT_HOST_BUILD, "refit: the tree was built on the host (gpu_build = 0), which keeps no hierarchy on the device: call build_tree()", 0, 0);
    if (nfaces != built_faces)
        return say(MPT_REFIT_FACES, "refit: the model has %d faces, the tree was built for %d: call build_tree()", nfaces, built_faces);
    return MPT_REFIT_OK;
}

// cost_now / cost_built of two sums in 2^-40 fixed point; 1 when there is nothing to compare (a tree without nodes)
inline double mpt_refit_growth_of(uint64_t cost_built, uint64_t cost_now) {
    if (cost_built == 0) return 1.0;
    return (double)cost_now / (double)cost_built;
}

// tree_refit.cpp -- mpt_refit_tree and its companions: the trees of the last mpt_build_tree kept as they
// are, and everything that build derived from vertex positions and material ids written again from the model as it is on the
// device now (lbvh_build.hip mpt_lbvh_refit, refit.hip).  When that is allowed and the growth figure are refit_rule.h's.

#include "miptina_ctx.h"

extern "C" int mpt_refit_allowed(int state, int built_faces, int built_on_device, int nfaces, char *why, int why_size) {
    return (int)mpt_refit_rule(state, built_faces, built_on_device, nfaces, why, why_size > 0 ? (size_t)why_size : 0);
}

extern "C" double mpt_refit_growth(uint64_t cost_built, uint64_t cost_now) { return mpt_refit_growth_of(cost_built, cost_now); }

extern "C" int mpt_refit_tree(mpt_ctx *c) {
    if (use(c)) return 1;
    auto &rf = c->refit;
    char why[200];
    if (mpt_refit_rule(rf.topo, rf.faces, rf.on_device, c->nfaces, why, sizeof why) != MPT_REFIT_OK) return fail("%s", why);
    const int n = c->nfaces, ni = n > 1 ? n - 1 : 0, nw = c->wide_nodes;
    const int64_t fetches_before = c->compose.stats.host_fetches;
    // as the build: whatever still reads the records (a render of the ring: the main stream waits for each) has finished
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n > 0 && c->d_model_stale) {                 // the model was loaded, not composed: it travels as for build_tree_gpu
        if ((size_t)n > c->dmodel.cap) return fail("refit: the device model has room for %zu faces, not %d: call build_tree()", c->dmodel.cap, n);
        HIP_TRY(hipMemcpyAsync(c->dmodel.d_verts, c->verts.data(), (size_t)n * 24 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dmodel.d_mtlids, c->mtlids.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    c->d_model_stale = false;
    c->tree_valid = false;                           // until every record is fitted
    if (rf.cost.reserve(2)) return 1;
    if (!rf.linked && ni > 0 && (rf.bin_parent.reserve((size_t)ni) || rf.wide_parent.reserve((size_t)std::max(nw, 1)))) return 1;
    const bool first = rf.refits == 0;               // of this build: the records are still the build's, whose cost is taken now
    {
        MptTimedSpan span(rf.timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(hipMemsetAsync(rf.cost, 0, 2 * sizeof(unsigned long long), c->stream));
        if (ni > 0 && !rf.linked) HIP_TRY(mpt_refit_link(c->nodes.fnode, ni, c->wnode, nw, rf.bin_parent, rf.wide_parent, c->stream));
        rf.linked = true;
        if (first) HIP_TRY(mpt_refit_cost(c->nodes.fnode, ni, rf.cost, c->stream));
        MptLbvhBuffers b{};
        b.verts = c->dmodel.d_verts; b.mtlids = c->dmodel.d_mtlids; b.n = n;
        b.child = c->lbvh.d_child; b.parent = c->lbvh.d_parent; b.leaf = c->lbvh.d_leaf;
        b.bmin = c->lbvh.d_bmin; b.bmax = c->lbvh.d_bmax; b.arrive = c->lbvh.d_arrive; b.depth = c->lbvh.d_depth;
        b.snode = c->nodes.snode; b.tgeo = c->tris.tgeo; b.tshade = c->tris.tshade;
        HIP_TRY(mpt_lbvh_refit(&b, c->stream));
        HIP_TRY(mpt_launch_derive_tfast(c->tris.tgeo, c->tfast, n, c->stream));
        HIP_TRY(hipMemsetAsync(c->tfast + (size_t)n * 3, 0xff, 3 * sizeof(MptVec4), c->stream));       // record n: NaNs, as the build leaves it
        HIP_TRY(mpt_refit_fit(c->dmodel.d_verts, c->lbvh.d_leaf, n, c->nodes.fnode, rf.bin_parent, c->wnode, c->qnode, nw, rf.wide_parent,
                              c->lbvh.d_arrive, c->stream));
        HIP_TRY(mpt_refit_cost(c->nodes.fnode, ni, rf.cost + 1, c->stream));
        HIP_TRY(span.end());
    }
    unsigned long long cost[2] = { 0ull, 0ull };
    HIP_TRY(hipMemcpyAsync(cost, rf.cost, sizeof cost, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (first) rf.cost_built = cost[0];
    rf.cost_now = cost[1];
    rf.refits++;
    rf.host_fetches += c->compose.stats.host_fetches - fetches_before;
    c->tree_valid = true;
    c->host_tree_valid = false;
    return 0;
}

extern "C" int mpt_refit_stats(mpt_ctx *c, mpt_refit_info *out) {
    if (!c || !out) return fail("null argument");
    const auto &rf = c->refit;
    const bool held = rf.topo == MPT_TOPO_HELD;
    out->faces = held ? rf.faces : -1;
    out->wide_nodes = held ? c->wide_nodes : 0;
    out->refits = held ? rf.refits : 0;
    out->host_fetches = rf.host_fetches;
    out->allowed = mpt_refit_rule(rf.topo, rf.faces, rf.on_device, c->nfaces, nullptr, 0) == MPT_REFIT_OK;
    out->cost_built = held && rf.refits ? (double)rf.cost_built / 1099511627776.0 : 0.0;
    out->cost_now = held && rf.refits ? (double)rf.cost_now / 1099511627776.0 : 0.0;
    out->growth = held && rf.refits ? mpt_refit_growth_of(rf.cost_built, rf.cost_now) : 1.0;
    return 0;
}

extern "C" int mpt_refit_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->refit.timer, ms, nullptr, launches);
}

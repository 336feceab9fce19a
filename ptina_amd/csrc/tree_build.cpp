// tree_build.cpp -- BVH construction behind mpt_build_tree: the glue around the host passes (tree_host.h: the reference LBVH,
// its SAH re-partition for the fast build, the 4-wide collapse) and around the device passes (lbvh_build.hip, sah_build.hip,
// wide_build.hip) -- the model and the records up and down, the fallbacks, the limits.

#include "miptina_ctx.h"
#include "tri_records.h"
#include "tree_host.h"

// phase clock of mpt_build_tree (option "build_phases": synchronise at every mark, so a phase's time is its device work too)
struct BuildClock {
    mpt_ctx *c;
    std::chrono::steady_clock::time_point t0, t;
    explicit BuildClock(mpt_ctx *ctx) : c(ctx) {
        for (double &v : c->build_phase_us) v = 0.0;
        t0 = t = std::chrono::steady_clock::now();
    }
    void mark(int k) {
        if (c->opt.build_phases) (void)hipStreamSynchronize(c->stream);
        const auto now = std::chrono::steady_clock::now();
        c->build_phase_us[k] += std::chrono::duration<double, std::micro>(now - t).count();
        c->build_phase_us[5] = std::chrono::duration<double, std::micro>(now - t0).count();
        t = now;
    }
};

// Device room for the node and triangle records of a tree over n faces.  The caller has synchronised the stream.
static int reserve_records(mpt_ctx *c, int n) {
    return c->nodes.reserve(std::max(n - 1, 1)) || c->tris.reserve(std::max(n, 1));
}

// The whole build on the host (gpu_build = 0): the passes of tree_host.h over the model, then the records go up
static int build_tree_host(mpt_ctx *c) {
    if (model_on_host(c)) return 1;
    const int n = c->nfaces, ni = n > 1 ? n - 1 : 0;
    const float *V = c->verts.data();
    HostLbvh t;
    if (const char *why = host_lbvh(V, n, t)) return fail("%s", why);
    c->tree_depth = t.depth;
    if (t.depth + 2 > 64) return fail("LBVH depth %d exceeds the 64-entry traversal stack", t.depth);
    std::vector<MptVec4> snode, fnode;
    pack_snode(t, n, snode);
    // the tree the fast build walks
    if (c->opt.tree == 1 && ni > 0) {
        SahBuild sb;
        sb.run(V, t.leaf.data(), n, c->opt.sah_exact_max);
        c->fast_depth = sb.depth;
        if (sb.depth + 2 > 64) return fail("BVH depth %d exceeds the 64-entry traversal stack", sb.depth);
        pack_fnode(V, t.leaf.data(), n, sb.child, sb.blo, sb.bhi, fnode);
    } else {
        c->fast_depth = t.depth;
        pack_fnode(V, t.leaf.data(), n, lbvh_fast_ids(t, n), t.bmin, t.bmax, fnode);
    }
    std::vector<MptVec4> tgeo((size_t)std::max(n, 1) * 4), tshade((size_t)std::max(n, 1) * 4);
    for (int slot = 0; slot < n; slot++) {
        const int f = t.leaf[slot];
        const float *p0 = vpos(V, f, 0), *p1 = vpos(V, f, 1), *p2 = vpos(V, f, 2);
        // hoisted terms of Face.intersect, geometries.py:120-122,134-136,140 (same f32 operations: tri_records.h)
        tri_make_tgeo(p0, p1, p2, &tgeo[(size_t)slot * 4]);
        tri_make_tshade(p0, p1, p2, asf(c->mtlids[f]), &tshade[(size_t)slot * 4]);
    }
    c->h_child.swap(t.child); c->h_leaf.swap(t.leaf); c->h_mc.swap(t.mc); c->h_bmin.swap(t.bmin); c->h_bmax.swap(t.bmax);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (reserve_records(c, n)) return 1;
    HIP_TRY(hipMemcpyAsync(c->nodes.snode, snode.data(), snode.size() * sizeof(MptVec4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->nodes.fnode, fnode.data(), fnode.size() * sizeof(MptVec4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->tris.tgeo, tgeo.data(), tgeo.size() * sizeof(MptVec4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->tris.tshade, tshade.data(), tshade.size() * sizeof(MptVec4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tree_valid = true;
    c->host_tree_valid = true;
    return 0;
}

extern "C" int mpt_sah_workspace(int n, int64_t nseg, int64_t out[4]) {
    if (n < 1 || nseg < 0 || !out) return 1;
    int nb = 0;
    out[0] = (int64_t)mpt_sah_seg_capacity(n);
    out[1] = (int64_t)mpt_sah_part_words(n);
    out[2] = (int64_t)mpt_sah_level_words(n, (size_t)nseg, &nb);
    out[3] = nb;
    return 0;
}

// workspace of mpt_sah_build: one device allocation carved into the arrays of MptSahBuffers
static int build_sah_device(mpt_ctx *c) {
    const int n = c->nfaces;
    const size_t SC = mpt_sah_seg_capacity(n), CC = mpt_sah_chunk_capacity(n), TC = mpt_sah_task_capacity(n), PW = mpt_sah_part_words(n);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t SW = mpt_sah_segbin_words(n);
    const size_t total = 2 * al((size_t)n * 32) + 2 * al(SC * 64) + al(SC * 32) + al(2 * CC * 4) + al(CC * 4) + al(PW * 4) + al(SW * 4) + al(TC * 32) + al(64);
    if (total > c->sah_ws.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->sah_ws.reserve(total)) return 1;
    }
    char *q = (char *)c->sah_ws;
    auto take = [&](size_t b) { char *r = q; q += al(b); return r; };
    MptSahBuffers B{};
    B.verts = c->dmodel.d_verts; B.leaf = c->lbvh.d_leaf; B.n = n;
    for (int k = 0; k < 2; k++) B.prim[k] = (MptVec4 *)take((size_t)n * 32);
    for (int k = 0; k < 2; k++) B.seg[k] = (int *)take(SC * 64);
    B.seg_cap = SC;
    B.dec = (int *)take(SC * 32);
    B.ch_seg = (int *)take(2 * CC * 4); B.ch_left = (int *)take(CC * 4); B.chunk_cap = CC;
    B.part = (int *)take(PW * 4); B.part_words = PW;
    B.segbins = (int *)take(SW * 4); B.segbin_words = SW;
    B.tasks = (int *)take(TC * 32); B.task_cap = TC;
    B.meta = (int *)take(64);
    B.stats = &c->sah_stats;
    B.mail_host = c->sah_mail.host; B.mail_dev = c->sah_mail.dev;
    B.fnode = c->nodes.fnode;
    int depth = 0;
    hipError_t e = mpt_sah_build(&B, &depth, c->stream);
    // Neither is fatal: the caller falls back to the host pass, which re-packs c->nodes.fnode from the LBVH leaf order (a failed
    // device pass may have overwritten part of it) and has its own depth handling (round-3 ADVICE)
    if (c->opt.sah_inject_fail) e = hipErrorInvalidValue;       // test door: the device pass ran (and wrote c->nodes.fnode), then "failed"
    if (e != hipSuccess) { (void)hipGetLastError(); c->sah_fallback = 1; return 2; }
    if (depth + 2 > 64) { c->sah_fallback = 2; return 2; }
    c->fast_depth = depth;
    return 0;
}

// SAH re-partition of the leaves for the fast build: host pass over the leaf order (exact sweep up to sah_exact_max leaves)
static int build_sah_host(mpt_ctx *c) {
    const int n = c->nfaces, ni = n - 1;
    if (model_on_host(c)) return 1;
    c->h_leaf.resize(n);
    HIP_TRY(hipMemcpy(c->h_leaf.data(), c->lbvh.d_leaf, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    SahBuild sb;
    sb.run(c->verts.data(), c->h_leaf.data(), n, c->opt.sah_exact_max);
    if (sb.depth + 2 > 64) return fail("BVH depth %d exceeds the 64-entry traversal stack", sb.depth);
    std::vector<MptVec4> fnode;
    pack_fnode(c->verts.data(), c->h_leaf.data(), n, sb.child, sb.blo, sb.bhi, fnode);
    HIP_TRY(hipMemcpy(c->nodes.fnode, fnode.data(), (size_t)ni * 4 * sizeof(MptVec4), hipMemcpyHostToDevice));
    c->fast_depth = sb.depth;
    return 0;
}

// lbvh.py:297-305 entirely on the device (lbvh_build.hip); only the depth (4 bytes) comes back,
// plus the leaf order when the fast build wants its SAH re-partition (a host pass today)
static int build_tree_gpu(mpt_ctx *c, BuildClock &clk) {
    const int n = c->nfaces;
    const int ni = n > 1 ? n - 1 : 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->dmodel.reserve(std::max(n, 1), &c->d_model_stale)) return 1;      // replaced: the next lines upload the model again
    if (c->lbvh.reserve(std::max(n, 1)) || reserve_records(c, n)) return 1;
    // the model travels to the device once per ModelPool.load (the reference's load is that copy too, model.py:71-86): a rebuild of
    // the tree -- another option, another tree kind -- finds it there (1.8 of 5.5 ms at a million triangles)
    if (n > 0 && c->d_model_stale) {
        HIP_TRY(hipMemcpyAsync(c->dmodel.d_verts, c->verts.data(), (size_t)n * 24 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dmodel.d_mtlids, c->mtlids.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    c->d_model_stale = false;
    clk.mark(0);
    MptLbvhBuffers b{};
    b.verts = c->dmodel.d_verts; b.mtlids = c->dmodel.d_mtlids; b.n = n;
    b.cen = c->lbvh.d_cen; b.bounds = c->lbvh.d_bounds; b.keys_in = c->lbvh.d_keys_in; b.keys_out = c->lbvh.d_keys_out;
    b.sort_tmp = c->lbvh.d_sort_tmp; b.sort_tmp_bytes = c->lbvh.d_sort_bytes;
    b.child = c->lbvh.d_child; b.parent = c->lbvh.d_parent; b.leaf = c->lbvh.d_leaf; b.mc = c->lbvh.d_mc;
    b.bmin = c->lbvh.d_bmin; b.bmax = c->lbvh.d_bmax; b.arrive = c->lbvh.d_arrive; b.depth = c->lbvh.d_depth;
    b.snode = c->nodes.snode; b.fnode = c->nodes.fnode; b.tgeo = c->tris.tgeo; b.tshade = c->tris.tshade;
    HIP_TRY(mpt_lbvh_build(&b, c->stream));
    int depth = 0;
    if (ni > 0) HIP_TRY(hipMemcpyAsync(&depth, c->lbvh.d_depth, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (depth + 2 > 64) return fail("LBVH depth %d exceeds the 64-entry traversal stack", depth);
    clk.mark(1);
    c->tree_depth = depth;
    c->fast_depth = depth;
    c->host_tree_valid = false;
    // auto: the host pass up to 8192 faces (all of its splits are exact sweeps there and it costs a millisecond or two: the trees
    // of the small scenes stay what they were), the device pass above (exact sweeps up to 512 triangles, up to 1024 bins per
    // axis above: sah_build.hip)
    const bool sah_on_device = c->opt.sah_build == 1 || (c->opt.sah_build < 0 && n > 8192);
    c->sah_fallback = 0;
    if (c->opt.tree == 1 && ni > 0 && n <= c->opt.sah_max) {
        // SAH re-partition of the leaves: on the device (sah_build.hip: nothing comes back but the depth), or the host pass --
        // also when the device pass gives up (workspace, level or depth limits): both start from the LBVH's leaf order
        int r = (sah_on_device && n >= 2) ? build_sah_device(c) : 2;
        if (r == 1) return 1;
        if (r == 2 && build_sah_host(c)) return 1;
    }
    clk.mark(2);
    c->tree_valid = true;
    return 0;
}

// The two limits of the collapse, outside which the gather kernel keeps walking the binary tree.  A step pushes up to three
// entries: 3 x depth + sentinel must fit the LDS levels plus the spill strip (40 + 88); and the kernel addresses the records
// with 32-bit byte offsets.
static int wide_stack_bound(int depth) { return 3 * depth + 2; }
static bool wide_fits(int depth, size_t nw) { return wide_stack_bound(depth) <= 128 && nw * 8 * sizeof(MptVec4) < ((size_t)1 << 31); }

// device room for nw 4-wide nodes, exact and quantised
static int reserve_wide(mpt_ctx *c, size_t nw) { return c->wnode.reserve(nw * 8) || c->qnode.reserve(nw * 4); }

// The collapse as a host pass over the downloaded records (1 M triangles: 64 MB down, ~0.1 s, 64 MB up), off the render path
static int make_wide_host(mpt_ctx *c) {
    c->wide_nodes = 0; c->wide_depth = 0; c->wide_stack = 0;
    const int n = c->nfaces, ni = n > 1 ? n - 1 : 0;
    if (ni < 1) return 0;
    std::vector<MptVec4> fnode((size_t)ni * 4);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(fnode.data(), c->nodes.fnode, fnode.size() * sizeof(MptVec4), hipMemcpyDeviceToHost));
    HostWide w;
    host_collapse(fnode.data(), n, w);
    const size_t nw = (size_t)w.nodes;
    if (!wide_fits(w.depth, nw)) return 0;
    if (reserve_wide(c, nw)) return 1;
    HIP_TRY(hipMemcpy(c->wnode, w.wnode.data(), nw * 8 * sizeof(MptVec4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->qnode, w.qnode.data(), nw * 4 * sizeof(MptVec4), hipMemcpyHostToDevice));
    c->wide_nodes = w.nodes; c->wide_depth = w.depth;
    c->wide_stack = wide_stack_levels(w.wnode.data() + WNODE_ID_ROW, 8, nw, n);
    c->wide_ratio = w.area_bin > 0.0 ? (float)(w.area_wide / w.area_bin) : 1.f;
    return 0;
}

// The same collapse on the device (wide_build.hip): nothing is downloaded, one integer per level comes back.  Produces the
// host pass's bytes (tests/test_parity_gpu.py::test_device_wide_collapse_equals_the_host_pass).
static int make_wide_device(mpt_ctx *c) {
    c->wide_nodes = 0; c->wide_depth = 0; c->wide_stack = 0;
    const int n = c->nfaces, ni = n > 1 ? n - 1 : 0;
    if (ni < 1) return 0;
    if (!wide_fits(0, (size_t)ni)) return 0;                // (at most one wide node per binary node)
    if (reserve_wide(c, (size_t)ni) || c->wb.reserve((size_t)ni)) return 1;
    int nw = 0, depth = 0;
    double area[2] = { 0.0, 0.0 };
    HIP_TRY(mpt_wide_build(c->nodes.fnode, n, c->wnode, c->qnode, c->wb.bin_of, c->wb.ncount, c->wb.scan, c->wb.scan_bytes,
                           c->wb.area, &nw, &depth, area, c->stream, c->sah_mail.host, c->sah_mail.dev));
    if (!wide_fits(depth, (size_t)nw)) return 0;
    c->wide_nodes = nw; c->wide_depth = depth;
    c->wide_stack = wide_stack_bound(depth);   // the bound ...
    if (nw > 0 && nw <= 4096) {             // ... and for a tree that may be walked out of LDS the exact count, from its id vectors (64 KiB at most)
        std::vector<MptVec4> ids((size_t)nw);
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy2D(ids.data(), sizeof(MptVec4), c->wnode + WNODE_ID_ROW, 8 * sizeof(MptVec4), sizeof(MptVec4), (size_t)nw, hipMemcpyDeviceToHost));
        c->wide_stack = std::min(c->wide_stack, wide_stack_levels(ids.data(), 1, (size_t)nw, n));
    }
    c->wide_ratio = area[1] > 0.0 ? (float)(area[0] / area[1]) : 1.f;
    return 0;
}

static int make_wide(mpt_ctx *c) { return c->opt.wide_build ? make_wide_device(c) : make_wide_host(c); }

// test / inspection: the 4-wide records the gather kernels walk -- wnode [nw][8] float4 (exact boxes), qnode [nw][4] float4
// (8-bit boxes); any pointer may be NULL; *nw = number of wide nodes (0: not built)
extern "C" int mpt_get_wide(mpt_ctx *c, float *wnode, float *qnode, int cap_nodes, int *nw) {
    if (use_ro(c)) return 1;
    if (!c->tree_valid) return fail("BVH not built: call build_tree() after load_model()");
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int k = std::min(cap_nodes, c->wide_nodes);
    if (wnode && k > 0) HIP_TRY(hipMemcpy(wnode, c->wnode, (size_t)k * 8 * sizeof(MptVec4), hipMemcpyDeviceToHost));
    if (qnode && k > 0) HIP_TRY(hipMemcpy(qnode, c->qnode, (size_t)k * 4 * sizeof(MptVec4), hipMemcpyDeviceToHost));
    if (nw) *nw = c->wide_nodes;
    return 0;
}

// test / inspection: the records every kernel of both builds fetches, as they lie on the device -- snode [n-1][2] float4,
// fnode [n-1][4], tgeo [n][4], tshade [n][4], tfast [n+1][3] (record n: the all-ones record of mpt_build_tree); any pointer
// may be NULL; *nfaces = n.  Room for fewer than n faces: refused before anything is written.  Reads only
extern "C" int mpt_get_records(mpt_ctx *c, float *snode, float *fnode, float *tgeo, float *tshade, float *tfast, int cap_faces,
                               int *nfaces) {
    if (use_ro(c)) return 1;
    if (!c->tree_valid) return fail("BVH not built: call build_tree() after load_model()");
    const int n = c->nfaces, ni = n > 1 ? n - 1 : 0;
    if (nfaces) *nfaces = n;
    struct { const char *name; float *out; const MptVec4 *dev; size_t held, rows; } part[5] = {
        { "snode", snode, c->nodes.snode, c->nodes.snode.cap, (size_t)ni * 2 }, { "fnode", fnode, c->nodes.fnode, c->nodes.fnode.cap, (size_t)ni * 4 },
        { "tgeo", tgeo, c->tris.tgeo, c->tris.tgeo.cap, (size_t)n * 4 },        { "tshade", tshade, c->tris.tshade, c->tris.tshade.cap, (size_t)n * 4 },
        { "tfast", tfast, c->tfast, c->tfast.cap, ((size_t)n + 1) * 3 } };
    for (const auto &p : part) {
        if (!p.out) continue;
        if (cap_faces < n) return fail("mpt_get_records: room for %d faces, the records hold %d", cap_faces, n);
        if (p.rows && (!p.dev || p.held < p.rows)) return fail("mpt_get_records: the context holds no %s records for %d faces", p.name, n);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const auto &p : part)
        if (p.out && p.rows) HIP_TRY(hipMemcpy(p.out, p.dev, p.rows * sizeof(MptVec4), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mpt_build_tree(mpt_ctx *c) {
    if (use(c)) return 1;
    BuildClock clk(c);
    c->refit.lose(MPT_TOPO_BUILD_FAILED);        // until this build has succeeded: it may replace or half-write the records
    if (c->opt.gpu_build ? build_tree_gpu(c, clk) : build_tree_host(c)) return 1;
    clk.mark(2);
    // the production kernels' 48-byte triangle records, from the reference-order ones
    // (+ 1: record n is all NaNs -- the leaf an unused slot of a 4-wide node names; no ray can hit it)
    const size_t nt = (size_t)std::max(c->nfaces, 1) + 1;
    if (nt * 3 > c->tfast.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->tfast.reserve(nt * 3)) return 1;
    }
    HIP_TRY(mpt_launch_derive_tfast(c->tris.tgeo, c->tfast, c->nfaces, c->stream));
    HIP_TRY(hipMemsetAsync(c->tfast + (size_t)c->nfaces * 3, 0xff, 3 * sizeof(MptVec4), c->stream));   // 0xffffffff: a NaN
    clk.mark(3);
    if (make_wide(c)) return 1;
    clk.mark(4);
    // the records hold a topology for nfaces faces: what mpt_refit_tree (tree_refit.cpp) keeps
    c->refit.topo = MPT_TOPO_HELD; c->refit.faces = c->nfaces; c->refit.on_device = c->opt.gpu_build != 0;
    c->refit.linked = false; c->refit.refits = 0; c->refit.cost_built = c->refit.cost_now = 0;
    c->tree_seq++;                               // a new leaf order (tree_query.cpp keeps its tables by it)
    return 0;
}

int download_tree(mpt_ctx *c) {
    if (c->host_tree_valid) return 0;
    const int n = c->nfaces, ni = n > 1 ? n - 1 : 0;
    c->h_child.assign((size_t)std::max(ni, 1) * 2, 0); c->h_leaf.assign(std::max(n, 1), 0); c->h_mc.assign(std::max(n, 1), 0);
    c->h_bmin.assign((size_t)std::max(ni, 1) * 3, 0.f); c->h_bmax.assign((size_t)std::max(ni, 1) * 3, 0.f);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n > 0) {
        HIP_TRY(hipMemcpy(c->h_leaf.data(), c->lbvh.d_leaf, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c->h_mc.data(), c->lbvh.d_mc, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    if (ni > 0) {
        HIP_TRY(hipMemcpy(c->h_child.data(), c->lbvh.d_child, (size_t)ni * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c->h_bmin.data(), c->lbvh.d_bmin, (size_t)ni * 3 * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c->h_bmax.data(), c->lbvh.d_bmax, (size_t)ni * 3 * sizeof(float), hipMemcpyDeviceToHost));
    }
    c->host_tree_valid = true;
    return 0;
}

extern "C" int mpt_get_tree(mpt_ctx *c, int32_t *child, int32_t *leaf, float *bmin, float *bmax, int32_t *mc,
                            int32_t *depth) {
    if (!c) return fail("null context");
    if (!c->tree_valid) return fail("BVH not built: call build_tree() after load_model()");
    if (download_tree(c)) return 1;
    int n = c->nfaces, ni = n > 1 ? n - 1 : 0;
    if (child) memcpy(child, c->h_child.data(), (size_t)ni * 2 * sizeof(int32_t));
    if (leaf) memcpy(leaf, c->h_leaf.data(), (size_t)n * sizeof(int32_t));
    if (bmin) memcpy(bmin, c->h_bmin.data(), (size_t)ni * 3 * sizeof(float));
    if (bmax) memcpy(bmax, c->h_bmax.data(), (size_t)ni * 3 * sizeof(float));
    if (mc) memcpy(mc, c->h_mc.data(), (size_t)n * sizeof(int32_t));
    if (depth) *depth = c->tree_depth;
    return 0;
}

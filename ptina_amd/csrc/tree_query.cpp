// tree_query.cpp -- batch ray queries on the built tree (mpt_query_closest, mpt_query_occluded; query_kernel.hip),
// and the test door that sends a batch of rays through the production walks (mpt_walk_trace; walk_eval.hip):
// the reference's LinearBVH.intersect(ray, avoid), lbvh.py:314-347, for n rays of a host array at once, through the tracer of the
// context's build.  The shape is mpt_mlt_trace's (engines.cpp): launched at the call on the main stream, behind everything enqueued
// before, and waited for.  Rays travel in chunks, so the device memory a call takes is bounded whatever n is; the chunk buffers
// belong to the context and are reused.
//
// A query reads the tree and the object table and writes buffers of its own: the film passes, the sampler, the counters, the
// selection, the mark, last_kernel and the launch ring are not touched, and the main stream is not marked -- the next render
// launch has nothing of a query's to wait for.

#include "miptina_ctx.h"

enum { MPT_QUERY_CHUNK = 1 << 22 };      // rays per launch by default: 40 bytes of input and 24 of answers each

// slot -> face and face -> slot of the tree as built: the tracers name a triangle by its leaf slot, callers by its face.  A refit
// keeps the leaf order, a build makes a new one (mpt_ctx::tree_seq).  (Also film_history.cpp's: its kernels name faces too.)
int query_tables(mpt_ctx *c) {
    auto &q = c->query;
    if (q.tables_seq == c->tree_seq && q.leaf.p) return 0;
    if (download_tree(c)) return 1;
    const size_t n = (size_t)c->nfaces;
    std::vector<int32_t> slot_of(std::max<size_t>(n, 1), -1);
    for (size_t s = 0; s < n; s++) {
        const int32_t f = c->h_leaf[s];
        if (f < 0 || (size_t)f >= n) return fail("mpt_query: leaf slot %zu names face %d of %zu", s, f, n);
        slot_of[f] = (int32_t)s;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));              // (a launch may still read the old tables)
    if (q.leaf.reserve(std::max<size_t>(n, 1)) || q.slot_of.reserve(std::max<size_t>(n, 1))) return 1;
    if (n > 0) {
        HIP_TRY(hipMemcpy(q.leaf, c->h_leaf.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(q.slot_of, slot_of.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    q.tables_seq = c->tree_seq;
    return 0;
}

// what both calls share up to the launch: the entry checks, the flush, the parameters, the tables, the chunk size and buffers
static int query_entry(mpt_ctx *c, const char *who, int n, const float *o, const float *d, int chunk, MptRenderParams &p, int *per) {
    if (n < 0 || chunk < 0) return fail("%s: bad arguments: n %d and chunk %d must be >= 0", who, n, chunk);
    if (use_ro(c)) return 1;
    if (n > 0 && (!o || !d)) return fail("%s: bad arguments: %d rays, origins %s, directions %s", who, n, o ? "given" : "null", d ? "given" : "null");
    if (mpt_flush(c)) return 1;                            // a deferred render lands first
    if (n == 0) return 0;
    if (fill_params(c, p, 1)) return 1;                    // (refuses a tree that is not built for the model as it stands, like a render)
    if (query_tables(c)) return 1;
    const long long want = chunk > 0 ? chunk : MPT_QUERY_CHUNK;
    *per = (int)std::min<long long>((want + MPT_BLOCK - 1) / MPT_BLOCK * MPT_BLOCK, 1ll << 30);
    const size_t rays = (size_t)std::min(n, *per);
    if (rays > c->query.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->query.reserve(rays)) return 1;
    }
    return 0;
}

// a chunk's rays to the device; the arguments every launch of the call shares
static int query_upload(mpt_ctx *c, MptQueryArgs &a, size_t at, int m, const float *o, const float *d, const float *dis, const int32_t *avoid) {
    auto &q = c->query;
    HIP_TRY(hipMemcpy(q.o, o + at * 3, (size_t)m * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(q.d, d + at * 3, (size_t)m * 3 * sizeof(float), hipMemcpyHostToDevice));
    if (dis) HIP_TRY(hipMemcpy(q.dis, dis + at, (size_t)m * sizeof(float), hipMemcpyHostToDevice));
    if (avoid) HIP_TRY(hipMemcpy(q.avoid, avoid + at, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice));
    a.o = q.o; a.d = q.d; a.dis = dis ? q.dis.p : nullptr; a.avoid = avoid ? q.avoid.p : nullptr;
    a.leaf = q.leaf; a.slot_of = q.slot_of;
    a.n = m;
    return 0;
}

template <class Launcher>
static int query_launch(mpt_ctx *c, Launcher launch, const MptRenderParams &p, const MptQueryArgs &a) {
    MptTimedSpan span(c->query.timer, c->stream);
    HIP_TRY(span.begun);
    HIP_TRY(launch(&p, &a, gather_stack_levels(c), c->stream));
    HIP_TRY(span.end());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

template <class T>
static int query_fetch(T *out, const T *dev, size_t at, int m) {
    if (out) HIP_TRY(hipMemcpy(out + at, dev, (size_t)m * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mpt_query_closest(mpt_ctx *c, int n, const float *o, const float *d, const int32_t *avoid, int32_t *hit, float *depth,
                                 int32_t *index, float *u, float *v, int32_t *object, int chunk) {
    MptRenderParams p;
    int per = 0;
    if (query_entry(c, "mpt_query_closest", n, o, d, chunk, p, &per)) return 1;
    if (n == 0) return 0;
    auto &q = c->query;
    const size_t cap = q.cap;
    // the object table of the model as composed (scene_compose.cpp): none where mpt_load_model brought the model
    const bool table = c->compose.out_valid && c->compose.out_objs > 0;
    for (size_t at = 0; at < (size_t)n; at += (size_t)per) {
        const int m = (int)std::min<size_t>((size_t)per, (size_t)n - at);
        MptQueryArgs a{};
        if (query_upload(c, a, at, m, o, d, nullptr, avoid)) return 1;
        a.first = table ? c->compose.bufs.first.p : nullptr; a.nobj = table ? c->compose.out_objs : 0;
        a.hit = hit ? q.out_i.p : nullptr; a.index = index ? q.out_i + cap : nullptr; a.object = object ? q.out_i + 2 * cap : nullptr;
        a.depth = depth ? q.out_f.p : nullptr; a.u = u ? q.out_f + cap : nullptr; a.v = v ? q.out_f + 2 * cap : nullptr;
        if (query_launch(c, MPT_LAUNCHER(c, mpt_launch_query_closest), p, a)) return 1;
        if (query_fetch(hit, a.hit, at, m) || query_fetch(index, a.index, at, m) || query_fetch(object, a.object, at, m) ||
            query_fetch(depth, a.depth, at, m) || query_fetch(u, a.u, at, m) || query_fetch(v, a.v, at, m)) return 1;
    }
    return 0;
}

extern "C" int mpt_query_occluded(mpt_ctx *c, int n, const float *o, const float *d, const float *dis, const int32_t *avoid, int32_t *occ,
                                  int chunk) {
    MptRenderParams p;
    int per = 0;
    if (c && n > 0 && !occ) return fail("mpt_query_occluded: bad arguments: %d rays and no place for the answers", n);
    if (query_entry(c, "mpt_query_occluded", n, o, d, chunk, p, &per)) return 1;
    if (n == 0) return 0;
    for (size_t at = 0; at < (size_t)n; at += (size_t)per) {
        const int m = (int)std::min<size_t>((size_t)per, (size_t)n - at);
        MptQueryArgs a{};
        if (query_upload(c, a, at, m, o, d, dis, avoid)) return 1;
        a.occ = c->query.out_i;
        if (query_launch(c, MPT_LAUNCHER(c, mpt_launch_query_occluded), p, a)) return 1;
        if (query_fetch(occ, a.occ, at, m)) return 1;
    }
    return 0;
}

// ---------------------------------------------------------------- test door through the production walks (walk_eval.hip)
// n rays through one of the five walk types the PathEngine kernels traverse with, set up and stepped by the render kernels' own code.
// The contract is a query's (above): deferred frames land first, nothing a render reads or writes is touched, rays travel in chunks.
// It refuses -- an error, never another walk -- a strict-mode context, a tree that is not built for the model as it stands, a 4-wide
// walk where the collapse was not built, and an LDS walk for a scene that lds_layout.h says does not fit.
enum { MPT_WALK_CHUNK = 1 << 16 };       // rays per launch at most: a 4-wide gather walk's lane owns 512 bytes of the spill strip

extern "C" int mpt_walk_trace(mpt_ctx *c, int walk, int n, const float *o, const float *d, const int32_t *avoid, const float *dis, int32_t *hit,
                              float *depth, int32_t *index, float *u, float *v, int chunk) {
    static const char *const names[MPT_WALK_COUNT] = { "binary gather", "LDS binary", "4-wide gather exact", "4-wide gather 8-bit", "LDS 4-wide" };
    if (n < 0 || chunk < 0) return fail("mpt_walk_trace: bad arguments: n %d and chunk %d must be >= 0", n, chunk);
    if (use_ro(c)) return 1;
    if (walk < 0 || walk >= MPT_WALK_COUNT) return fail("mpt_walk_trace: bad arguments: walk %d is none of 0 .. %d", walk, MPT_WALK_COUNT - 1);
    if (c->opt.mode != MPT_MODE_FAST) return fail("mpt_walk_trace: the walks are the production build's: the context is in strict mode");
    if (n > 0 && (!o || !d)) return fail("mpt_walk_trace: bad arguments: %d rays, origins %s, directions %s", n, o ? "given" : "null", d ? "given" : "null");
    if (n > 0 && dis && !hit) return fail("mpt_walk_trace: bad arguments: %d shadow rays and no place for the verdicts", n);
    if (mpt_flush(c)) return 1;                            // a deferred render lands first
    MptRenderParams p;
    if (fill_params(c, p, 1)) return 1;                    // (refuses a tree that is not built for the model as it stands, like a render)
    p.lds_nmats = c->max_mtlid + 1;                        // (as mpt_flush sets it for render_kernel_lds4)
    size_t lds_bytes = 0;
    switch (walk) {
    case MPT_WALK_LDS:
        lds_bytes = (size_t)mpt_lds_fit_bytes(c->nfaces, c->caps.max_materials, c->fast_depth);
        if (!lds_bytes) return fail("mpt_walk_trace: the %s walk cannot serve this scene: %d faces do not fit a CU's LDS", names[walk], c->nfaces);
        break;
    case MPT_WALK_LDS4:
        if (c->wnode) lds_bytes = (size_t)mpt_lds4_fit_bytes(c->nfaces, c->wide_nodes, c->wide_stack, c->max_mtlid + 1);
        if (!lds_bytes) return fail("mpt_walk_trace: the %s walk cannot serve this scene: %d faces in %d 4-wide nodes do not fit a CU's LDS", names[walk], c->nfaces, c->wide_nodes);
        break;
    case MPT_WALK_WIDE_EXACT: case MPT_WALK_WIDE_QUANT:
        if (c->wide_nodes <= 0 || !(walk == MPT_WALK_WIDE_EXACT ? c->wnode.p : c->qnode.p))
            return fail("mpt_walk_trace: the %s walk cannot serve this scene: the 4-wide tree was not built", names[walk]);
        break;
    default: break;
    }
    if (n == 0) return 0;
    fill_t_scale(c, p, o, n);                              // no origin of the batch farther than 1 / t_scale from the scene (LdsWalk4::T_SCALED)
    if (query_tables(c)) return 1;
    const long long want = chunk > 0 ? std::min<long long>(chunk, MPT_WALK_CHUNK) : MPT_WALK_CHUNK;
    const int per = (int)((want + MPT_LDS_LANES - 1) / MPT_LDS_LANES * MPT_LDS_LANES);   // whole workgroups of either kind
    auto &q = c->query;
    const size_t rays = (size_t)std::min(n, per);
    const bool wide = walk == MPT_WALK_WIDE_EXACT || walk == MPT_WALK_WIDE_QUANT;
    const size_t strip = wide ? (rays + MPT_BLOCK - 1) / MPT_BLOCK * MPT_BLOCK * 128 : 0;      // >= GatherWalk4::SPILL entries per lane of the grid
    if (rays > q.cap || strip > q.walk_spill.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (q.reserve(rays) || q.walk_spill.reserve(strip)) return 1;
    }
    p.stack_spill = wide ? q.walk_spill.p : nullptr;
    const size_t cap = q.cap;
    for (size_t at = 0; at < (size_t)n; at += (size_t)per) {
        const int m = (int)std::min<size_t>((size_t)per, (size_t)n - at);
        MptQueryArgs a{};
        if (query_upload(c, a, at, m, o, d, dis, avoid)) return 1;
        a.hit = hit ? q.out_i.p : nullptr; a.index = index && !dis ? q.out_i + cap : nullptr;
        a.depth = depth && !dis ? q.out_f.p : nullptr; a.u = u && !dis ? q.out_f + cap : nullptr; a.v = v && !dis ? q.out_f + 2 * cap : nullptr;
        HIP_TRY(mpt_launch_walk_eval(&p, &a, walk, gather_stack_levels(c), lds_bytes, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        // (render_kernel_lds4's check that its dynamic LDS starts at address 0, which its node ids count from)
        if (walk == MPT_WALK_LDS4 && __atomic_exchange_n(c->watchdog.host.p, 0u, __ATOMIC_ACQ_REL))
            return fail("mpt_walk_trace: the %s walk's dynamic LDS does not start at LDS address 0", names[walk]);
        if (query_fetch(hit, a.hit, at, m)) return 1;
        if (!dis && (query_fetch(index, a.index, at, m) || query_fetch(depth, a.depth, at, m) || query_fetch(u, a.u, at, m) ||
                     query_fetch(v, a.v, at, m))) return 1;        // (a shadow batch writes the verdicts alone)
    }
    return 0;
}

extern "C" int mpt_query_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->query.timer, ms, nullptr, launches);
}

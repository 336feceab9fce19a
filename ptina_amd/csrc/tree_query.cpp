// tree_query.cpp -- batch ray queries on the built tree (mpt_query_closest, mpt_query_occluded; query_kernel.hip):
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
// keeps the leaf order, a build makes a new one (mpt_ctx::tree_seq)
static int query_tables(mpt_ctx *c) {
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

extern "C" int mpt_query_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->query.timer, ms, nullptr, launches);
}

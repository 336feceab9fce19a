// engines.cpp -- the engines that launch at the call, on the main stream: PreviewEngine (mpt_render_preview), the Metropolis
// engine (mpt_mlt_*), BruteEngine (mpt_render_brute) and adaptive sampling's list pass (mpt_render_selected).  Their kernels have
// one shape -- one lane per item, the lane's traversal stack in LDS, walked through make_block_tracer (path_common.h) -- and their
// launchers one form: MPT_LAUNCHER(c, name)(parameters ..., gather_stack_levels(c), stream).
//
// Ordering.  use() has flushed the PathEngine frames and Metropolis iterations enqueued before (the main stream waits for their
// render streams) and marked the main stream (main_dirty), and the next PathEngine launch waits for what is enqueued here
// (main_dirty -> ev_main): frames of every engine add to film pass 0 in call order.

#include "miptina_ctx.h"

// A call's frames, in launches of at most `per`: each gets the parameters and the sampler's points of its B frames -- one chunk --
// and then launch(p, B) runs.  What launches nothing (an empty share, an empty selection) still moves the sampler.
template <class Launch>
static int batches(mpt_ctx *c, int nframes, int per, Launch launch) {
    while (nframes > 0) {
        const int B = std::min(nframes, per);
        MptRenderParams p;
        if (fill_params(c, p, B)) return 1;
        if (sobol_advance(c, B, B)) return 1;
        p.chunk = B; p.nchunks = 1;
        if (launch(p, B)) return 1;
        nframes -= B;
    }
    return 0;
}

// What closes a launch that added to film pass 0: an early image of an earlier PathEngine launch is stale, and the next PathEngine
// launch waits for this one.  (A call under use() that launched nothing has the main stream marked already.)
static void pass0_changed(mpt_ctx *c) {
    c->film_version++;
    c->main_dirty = true;
}

extern "C" int mpt_render_preview(mpt_ctx *c, int nframes) {                   // preview.py:18-41
    if (use(c)) return 1;
    return batches(c, nframes, MPT_MAX_BATCH, [c](const MptRenderParams &p, int) {
        if (p.ntiles) HIP_TRY(MPT_LAUNCHER(c, mpt_launch_preview)(&p, p.ntiles, gather_stack_levels(c), c->stream));
        return 0;
    });
}

// ------------------------------------------------------------------ Metropolis engine (MLTPathEngine, engine/mltpath.py)
// Everything runs on the main stream, which every PathEngine launch is ordered behind (mpt_flush) and which the next one waits
// for (main_dirty -> ev_main), so PathEngine frames and Metropolis iterations add to film pass 0 in call order.
enum { MPT_MLT_SLAB_RECORDS = 1 << 24 };      // splat records per launch (20 B each, twice for the sort): larger requests are split

static int mlt_check(mpt_ctx *c) {
    if (c->mlt.n <= 0) return fail("Metropolis engine not reset: call mpt_mlt_reset first");
    return 0;
}

// launch the enqueued iterations: chain kernel + splat pass per slab-sized piece, in iteration order
int mlt_flush(mpt_ctx *c) {
    int n = c->mlt.pending;
    c->mlt.pending = 0;
    if (n <= 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    MptRenderParams p;
    if (fill_params(c, p, 1)) return 1;
    const int nch = c->mlt.n;
    const int kmax = std::max(1, (int)(MPT_MLT_SLAB_RECORDS / nch));
    const int K0 = std::min(n, kmax);
    const size_t recs = (size_t)K0 * nch, npix = (size_t)c->nx * c->ny;
    if (recs > c->mlt.slab.cap || npix > c->mlt.slab.runs_cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->mlt.slab.reserve(recs, npix)) return 1;
    }
    while (n > 0) {
        const int K = std::min(n, kmax);
        MptMltArgs a;
        a.X = c->mlt.X; a.L = c->mlt.L; a.bit = c->mlt.bit; a.keys = c->mlt.slab.keys; a.vals = c->mlt.slab.vals;
        a.nchains = nch; a.t0 = c->mlt.iter; a.K = K; a.seed = c->mlt.seed; a.lsp = c->mlt.lsp; a.sigma = c->mlt.sigma;
        MptTimedSpan span(c->mlt.timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(MPT_LAUNCHER(c, mpt_launch_mlt_chain)(&p, &a, gather_stack_levels(c), c->stream));
        HIP_TRY(span.mark());
        HIP_TRY(mpt_launch_mlt_splat(c->fb.film[0], c->mlt.slab.keys, c->mlt.slab.vals, c->mlt.slab.keys_sorted, c->mlt.slab.vals_sorted,
                                     c->mlt.slab.tmp, c->mlt.slab.tmp.cap, c->mlt.slab.runs, K * nch, (int)npix, c->stream));
        HIP_TRY(span.end());
        c->mlt.iter += K;
        n -= K;
    }
    pass0_changed(c);
    return 0;
}

extern "C" int mpt_mlt_reset(mpt_ctx *c, int nchains, uint32_t seed) {         // mltpath.py:31-37
    if (use(c)) return 1;
    if (nchains <= 0 || nchains > (1 << 24)) return fail("nchains %d outside [1, 2^24]", nchains);
    if (nchains != c->mlt.n) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->mlt.X.release(); c->mlt.L.release(); c->mlt.bit.release(); c->mlt.n = 0;
        if (c->mlt.X.reserve((size_t)nchains * 2 * 32) || c->mlt.L.reserve((size_t)nchains * 3) || c->mlt.bit.reserve((size_t)nchains)) return 1;
        c->mlt.n = nchains;
    }
    c->mlt.seed = seed; c->mlt.iter = 0; c->mlt.pending = 0;
    HIP_TRY(mpt_launch_mlt_reset(c->mlt.X, c->mlt.L, c->mlt.bit, nchains, seed, c->stream));
    return 0;
}

extern "C" int mpt_mlt_set_param(mpt_ctx *c, float lsp, float sigma) {       // mltpath.py:18-27: LSP[None], Sigma[None]
    if (use(c)) return 1;                   // iterations enqueued so far run with the parameters they were enqueued under
    c->mlt.lsp = lsp; c->mlt.sigma = sigma;
    return 0;
}

extern "C" int mpt_mlt_render(mpt_ctx *c, int iterations) {                    // mltpath.py:85-87
    if (!c) return fail("null context");
    if (iterations < 0) return fail("iterations must be >= 0");
    if (mlt_check(c)) return 1;
    if (c->nx <= 0) return fail("film size not set: call set_size() first");
    if (!c->tree_valid) return fail("BVH not built: call build_tree() after load_model()");
    if (c->stripe_w != 0 || c->x0 != 0 || c->x1 != c->nx || c->comm)
        return fail("the Metropolis engine renders the whole film on one GPU: no slab / stripe split or communicator may be set");
    if ((long long)c->mlt.iter + c->mlt.pending + iterations >= (1ll << 31)) return fail("Metropolis iteration counter would overflow");
    if (c->pending && mpt_flush(c)) return 1;      // PathEngine frames enqueued before go first
    c->mlt.pending += iterations;
    return 0;
}

extern "C" int mpt_mlt_get_state(mpt_ctx *c, float *X, float *L, int *iteration) {
    if (use_ro(c)) return 1;
    if (mpt_flush(c)) return 1;
    if (mlt_check(c)) return 1;
    const size_t n = (size_t)c->mlt.n;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (X) {
        std::vector<float> both(n * 2 * 32);
        std::vector<int32_t> bit(n);
        HIP_TRY(hipMemcpy(both.data(), c->mlt.X, both.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(bit.data(), c->mlt.bit, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) memcpy(X + i * 32, both.data() + ((size_t)(bit[i] & 1) * n + i) * 32, 32 * sizeof(float));
    }
    if (L) HIP_TRY(hipMemcpy(L, c->mlt.L, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (iteration) *iteration = c->mlt.iter;
    return 0;
}

extern "C" int mpt_mlt_set_state(mpt_ctx *c, const float *X, const float *L, int iteration) {
    if (use(c)) return 1;
    if (mlt_check(c)) return 1;
    if (!X || !L || iteration < 0) return fail("mpt_mlt_set_state: X and L must be given and iteration >= 0");
    const size_t n = (size_t)c->mlt.n;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->mlt.X, X, n * 32 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->mlt.L, L, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->mlt.bit, 0, n * sizeof(int32_t)));
    HIP_TRY(hipDeviceSynchronize());
    c->mlt.iter = iteration;
    return 0;
}

extern "C" int mpt_mlt_trace(mpt_ctx *c, const float *X, float *rgb, int n) {
    if (use_ro(c)) return 1;
    if (mpt_flush(c)) return 1;
    if (n < 0 || (n > 0 && (!X || !rgb))) return fail("mpt_mlt_trace: bad arguments");
    if (n == 0) return 0;
    MptRenderParams p;
    if (fill_params(c, p, 1)) return 1;
    DevBuf<float> dX, drgb;
    if (dX.reserve((size_t)n * 32) || drgb.reserve((size_t)n * 3)) return 1;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(dX, X, (size_t)n * 32 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = MPT_LAUNCHER(c, mpt_launch_mlt_trace)(&p, dX, drgb, n, gather_stack_levels(c), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(rgb, drgb, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail("mpt_mlt_trace: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int mpt_mlt_kernel_time(mpt_ctx *c, double *chain_ms, double *splat_ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->mlt.timer, chain_ms, splat_ms, launches);
}

// ------------------------------------------------------------------ brute-force engine (BruteEngine, engine/brute.py)
extern "C" int mpt_render_brute(mpt_ctx *c, int nframes) {                     // brute.py:24-26
    if (render_entry(c, nframes)) return 1;
    if (use(c)) return 1;
    return batches(c, nframes, MPT_MAX_BATCH, [c](const MptRenderParams &p, int) {
        if (!p.ntiles) return 0;
        MptTimedSpan span(c->brute_timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(MPT_LAUNCHER(c, mpt_launch_brute)(&p, p.ntiles, gather_stack_levels(c), c->stream));
        HIP_TRY(span.end());
        pass0_changed(c);
        return 0;
    });
}

extern "C" int mpt_brute_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->brute_timer, ms, nullptr, launches);
}

// ------------------------------------------------------------------ adaptive sampling: the list pass (PathEngine.render_selected)
// nframes samples for the pixels of the selection only (mpt_adapt_select / mpt_adapt_set_list, film_read.cpp): the list render
// kernel leaves every sample in fb.adapt_samples, the fold adds them to pass 0 in frame order.
enum : size_t { MPT_ADAPT_SAMPLE_BYTES = (size_t)64 << 20 };   // a launch's samples stay under this: a call's frames are split to fit

// the launches of a call: `per` frames at most each; the first fold moves the mark (remark).  An empty selection launches
// nothing, and the sampler still advances by the call's frames
static int selected_launches(mpt_ctx *c, int nframes, int remark, int per) {
    const int count = c->adapt.count;
    return batches(c, nframes, per, [c, count, &remark](const MptRenderParams &p, int B) {
        if (count <= 0) return 0;
        HIP_TRY(MPT_LAUNCHER(c, mpt_launch_adapt_render)(&p, c->fb.adapt.list, count, c->fb.adapt_samples, gather_stack_levels(c), c->stream));
        HIP_TRY(mpt_launch_adapt_fold(c->fb.film[0], remark ? c->fb.mark.p : nullptr, c->fb.adapt.list, count, c->fb.adapt_samples, B, remark,
                                      c->stream));
        remark = 0;
        return 0;
    });
}

extern "C" int mpt_render_selected(mpt_ctx *c, int nframes, int remark) {
    if (render_entry(c, nframes)) return 1;
    if (!c->adapt.selected)
        return fail("mpt_render_selected: no selection: call mpt_adapt_select() or mpt_adapt_set_list() first (mpt_clear and mpt_set_size drop the selection)");
    if (remark && !c->noise.marked)
        return fail("mpt_render_selected: no mark: call mpt_film_mark() first (mpt_clear and mpt_set_size drop the mark)");
    if (use(c)) return 1;
    const int count = c->adapt.count;
    int per = MPT_MAX_BATCH;
    if (count > 0) per = (int)std::min<size_t>(MPT_MAX_BATCH, std::max<size_t>(1, (MPT_ADAPT_SAMPLE_BYTES - 1) / (sizeof(MptVec4) * (size_t)count)));
    if (count <= 0 || nframes == 0) return selected_launches(c, nframes, 0, per);
    const size_t need = (size_t)count * (size_t)std::min(nframes, per);
    if (need > c->fb.adapt_samples.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));          // (a launch may still read the old buffer)
        if (c->fb.adapt_samples.reserve(need)) return 1;
    }
    MptTimedSpan span(c->adapt.render_timer, c->stream);
    HIP_TRY(span.begun);
    if (selected_launches(c, nframes, remark ? 1 : 0, per)) return 1;
    HIP_TRY(span.end());
    pass0_changed(c);
    return 0;
}

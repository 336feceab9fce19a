// film_history.cpp -- the film's reprojection behind the C ABI of include/miptina.h (mpt_history_*): a
// context remembers one rendered view -- its camera, the model's positions and a G-buffer of what every pixel's centre ray saw
// (history_kernel.hip) -- and, after the camera or the model changed, resamples film pass 0 into the new view (history.hip), pixel
// by pixel, following where each visible surface point lay in the remembered one.  When that is allowed and the arithmetic of a
// pixel are history_rule.h's.
//
// Everything here runs on the main stream behind what is enqueued, like the read-backs (film_read.cpp).  keep writes buffers of its
// own and nothing a render reads; reproject replaces pass 0 (it resamples into a second buffer and swaps the two: no film is
// copied), zeroes passes 1 and 2 and drops the mark and the selection, as mpt_clear does.

#include "miptina_ctx.h"

static bool whole_film(const mpt_ctx *c) { return c->x0 == 0 && c->x1 == c->nx && c->stripe_w == 0; }

// before a launch reads c->dmodel.d_verts: the model as it stands is there (uploaded as for build_tree_gpu if mpt_load_model
// brought it and no device build has taken it yet; a composed model lives there)
static int model_on_device(mpt_ctx *c) {
    const int n = c->nfaces;
    if ((size_t)std::max(n, 1) > c->dmodel.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->dmodel.reserve(std::max(n, 1), &c->d_model_stale)) return 1;
    }
    if (n > 0 && c->d_model_stale) {
        HIP_TRY(hipMemcpyAsync(c->dmodel.d_verts, c->verts.data(), (size_t)n * 24 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dmodel.d_mtlids, c->mtlids.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    c->d_model_stale = false;
    return 0;
}

// what both tracing launches share: the tables that name a hit's face and object
static void history_tables(const mpt_ctx *c, MptHistoryArgs &a) {
    const bool table = c->compose.out_valid && c->compose.out_objs > 0;      // none where mpt_load_model brought the model
    a.leaf = c->query.leaf;
    a.first = table ? c->compose.bufs.first.p : nullptr;
    a.nobj = table ? c->compose.out_objs : 0;
}

// the parameters of a call: the defaults of include/miptina.h, or the caller's
static void history_params(const mpt_history_params *params, mpt_history_params &hp) {
    hp = { 32.0f, 0.02f };
    if (params) hp = *params;
}

extern "C" int mpt_history_allowed(int have_history, int kept_nx, int kept_ny, int nx, int ny, int kept_faces, int nfaces, int tree_valid,
                                   float max_history, float depth_tol, char *why, int why_size) {
    return (int)mpt_history_rule(have_history, kept_nx, kept_ny, nx, ny, kept_faces, nfaces, tree_valid, max_history, depth_tol, why,
                                 why_size > 0 ? (size_t)why_size : 0);
}

extern "C" int mpt_history_keep(mpt_ctx *c) {
    if (!c) return fail("mpt_history_keep: null context");
    if (use_ro(c) || mpt_flush(c)) return 1;               // a deferred render lands first
    MptRenderParams p;
    if (fill_params(c, p, 1)) return 1;                    // (refuses a tree that is not built for the model as it stands, like a render)
    if (check_pass(c, 0) || query_tables(c) || model_on_device(c)) return 1;
    auto &h = c->history;
    const int n = c->nfaces;
    const size_t npix = (size_t)c->nx * c->ny, floats = (size_t)std::max(n, 1) * 9;
    if (c->fb.hist.cap < c->fb.cap || h.verts.cap < floats) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        h.forget();
        if (c->fb.reserve_history() || h.verts.reserve(floats)) return 1;
    }
    if (!h.stats.dev && h.stats.create(1)) return 1;
    h.forget();                                            // (until the launches below are enqueued)
    MptHistoryBufs &b = c->fb.hist;
    MptHistoryArgs a{};
    history_tables(c, a);
    a.face = b.face; a.id = b.id; a.depth = b.depth;
    {
        MptTimedSpan span(h.keep_timer, c->stream);
        HIP_TRY(span.begun);
        if (!whole_film(c)) {                              // the pixels the kernel does not visit: (-1, -1, 0)
            HIP_TRY(hipMemsetAsync(b.face, 0xff, npix * sizeof(int32_t), c->stream));
            HIP_TRY(hipMemsetAsync(b.id, 0xff, npix * sizeof(int32_t), c->stream));
            HIP_TRY(hipMemsetAsync(b.depth, 0, npix * sizeof(float), c->stream));
        }
        HIP_TRY(mpt_launch_history_verts(c->dmodel.d_verts, h.verts, n, c->stream));
        HIP_TRY(MPT_LAUNCHER(c, mpt_launch_history_gbuffer)(&p, &a, gather_stack_levels(c), c->stream));
        HIP_TRY(span.end());
    }
    memcpy(h.v2w, c->v2w, sizeof h.v2w);
    memcpy(h.w2v, c->w2v, sizeof h.w2v);
    h.nx = c->nx; h.ny = c->ny; h.faces = n;
    h.have = h.gbuffer = true;
    return 0;
}

extern "C" int mpt_history_reproject(mpt_ctx *c, const mpt_history_params *params, mpt_history_stats *stats) {
    if (!c) return fail("mpt_history_reproject: null context");
    if (use_ro(c) || mpt_flush(c)) return 1;
    auto &h = c->history;
    mpt_history_params hp;
    history_params(params, hp);
    char why[256];
    if (mpt_history_rule(h.have, h.nx, h.ny, c->nx, c->ny, h.faces, c->nfaces, c->tree_valid, hp.max_history, hp.depth_tol, why, sizeof why) != MPT_HISTORY_OK)
        return fail("%s", why);
    if (!h.gbuffer) return fail("reproject: no history: the film's buffers were made again since keep_history(): call keep_history() first");
    MptRenderParams p;
    if (fill_params(c, p, 1)) return 1;
    if (check_pass(c, 0) || query_tables(c) || model_on_device(c)) return 1;
    if (use(c)) return 1;                                  // from here on the film changes: the next render launch waits for this call's work
    const size_t npix = (size_t)c->nx * c->ny;
    MptHistoryBufs &b = c->fb.hist;
    MptHistoryArgs a{};
    history_tables(c, a);
    a.same_camera = !memcmp(h.v2w, c->v2w, sizeof h.v2w) && !memcmp(h.w2v, c->w2v, sizeof h.w2v);
    a.kept_verts = h.verts; a.cur_verts = c->dmodel.d_verts;
    memcpy(a.kept_w2v, h.w2v, sizeof a.kept_w2v);
    memcpy(a.kept_v2w, h.v2w, sizeof a.kept_v2w);
    a.motion = b.motion;
    MptResampleArgs r{};
    r.f_old = c->fb.film[0]; r.f_new = b.f_new;
    r.face = b.face; r.id = b.id; r.depth = b.depth; r.motion = b.motion;
    r.nx = c->nx; r.ny = c->ny; r.x0 = c->x0; r.x1 = c->x1;
    r.stripe_w = c->stripe_w; r.stripe_idx = c->stripe_idx; r.stripe_mod = c->stripe_mod;
    r.max_history = hp.max_history; r.depth_tol = hp.depth_tol;
    h.motion = false;
    {
        MptTimedSpan span(h.reproject_timer, c->stream);
        HIP_TRY(span.begun);
        if (!whole_film(c)) HIP_TRY(hipMemsetAsync(b.motion, 0xff, npix * sizeof(MptMotion), c->stream));   // the pixels the kernel does not visit
        HIP_TRY(MPT_LAUNCHER(c, mpt_launch_history_motion)(&p, &a, gather_stack_levels(c), c->stream));
        HIP_TRY(mpt_launch_history_resample(&r, b.part, h.stats.dev, c->stream));
        for (int pass = 1; pass < 3; pass++)
            if (c->fb.film[pass]) HIP_TRY(hipMemsetAsync(c->fb.film[pass], 0, npix * sizeof(MptVec4), c->stream));
        HIP_TRY(span.end());
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->fb.film[0].swap(b.f_new);                           // the resampled film is pass 0; the old one is the next call's room
    c->film_version++;
    c->noise.marked = false;                               // as mpt_clear: the samples the mark counted are not these
    c->adapt.selected = false; c->adapt.count = 0;
    h.have = false; h.motion = true;                       // the history is spent; its G-buffer and the motion records stay readable
    if (stats) memcpy(stats, (const void *)h.stats.host.p, sizeof *stats);
    return check_watchdog(c);
}

extern "C" int mpt_history_drop(mpt_ctx *c) {
    if (!c) return fail("mpt_history_drop: null context");
    if (use_ro(c) || mpt_flush(c)) return 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->history.forget();
    c->fb.hist.release();
    c->history.verts.release();
    return 0;
}

extern "C" int mpt_history_get_motion(mpt_ctx *c, mpt_history_motion *out) {
    if (!c) return fail("mpt_history_get_motion: null context");
    if (use_ro(c)) return 1;
    if (!out) return fail("mpt_history_get_motion: null output");
    if (!c->history.motion) return fail("mpt_history_get_motion: no motion records: call mpt_history_reproject() first (keep, drop and a larger film drop them)");
    if (c->nx != c->history.nx || c->ny != c->history.ny)
        return fail("mpt_history_get_motion: the film is %dx%d, the records are of a film of %dx%d", c->nx, c->ny, c->history.nx, c->history.ny);
    if (mpt_flush(c)) return 1;
    return read_back(c, out, c->fb.hist.motion, (size_t)c->history.nx * c->history.ny * sizeof(MptMotion));
}

extern "C" int mpt_history_get_gbuffer(mpt_ctx *c, int32_t *face, int32_t *id, float *depth) {
    if (!c) return fail("mpt_history_get_gbuffer: null context");
    if (use_ro(c)) return 1;
    if (!c->history.gbuffer) return fail("mpt_history_get_gbuffer: no G-buffer: call mpt_history_keep() first (drop and a larger film drop it)");
    if (c->nx != c->history.nx || c->ny != c->history.ny)
        return fail("mpt_history_get_gbuffer: the film is %dx%d, the G-buffer is of a film of %dx%d", c->nx, c->ny, c->history.nx, c->history.ny);
    if (mpt_flush(c)) return 1;
    const size_t npix = (size_t)c->history.nx * c->history.ny;
    const MptHistoryBufs &b = c->fb.hist;
    if (face && read_back(c, face, b.face, npix * sizeof(int32_t))) return 1;
    if (id && read_back(c, id, b.id, npix * sizeof(int32_t))) return 1;
    if (depth && read_back(c, depth, b.depth, npix * sizeof(float))) return 1;
    return 0;
}

// test door: the same resample launch on the caller's arrays, the whole film as the share, in buffers of its own (no film pass and
// nothing of the context's history)
extern "C" int mpt_history_eval(mpt_ctx *c, const mpt_history_params *params, const float *f_old, const int32_t *face, const int32_t *id,
                                const float *depth, const mpt_history_motion *motion, int nx, int ny, float *f_new, mpt_history_stats *stats) {
    if (!c) return fail("mpt_history_eval: null context");
    if (use_ro(c)) return 1;
    if (!f_old || !face || !id || !depth || !motion) return fail("mpt_history_eval: null input");
    if (!f_new && !stats) return fail("mpt_history_eval: null outputs");
    mpt_history_params hp;
    history_params(params, hp);
    char why[256];
    if (mpt_history_rule(1, nx, ny, nx, ny, 0, 0, 1, hp.max_history, hp.depth_tol, why, sizeof why) != MPT_HISTORY_OK) return fail("mpt_history_eval: %s", why);
    if (nx < 1 || ny < 1 || (long long)nx * ny > (long long)c->caps.max_filmsize)
        return fail("mpt_history_eval: film %dx%d outside 1 .. max_filmsize=%d pixels", nx, ny, c->caps.max_filmsize);
    auto &h = c->history;
    const size_t npix = (size_t)nx * ny;
    MptHistoryBufs &b = h.bufs;
    if (npix > c->door.cap || npix > b.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->door.reserve(npix) || b.reserve(npix)) return 1;
    }
    if (!h.stats.dev && h.stats.create(1)) return 1;
    HIP_TRY(hipMemcpyAsync(c->door.acc[0], f_old, npix * sizeof(MptVec4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.face, face, npix * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.id, id, npix * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.depth, depth, npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.motion, motion, npix * sizeof(MptMotion), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));              // (the arrays are pageable: the copies are staged, the caller's arrays are free again)
    MptResampleArgs r{};
    r.f_old = c->door.acc[0]; r.f_new = b.f_new;
    r.face = b.face; r.id = b.id; r.depth = b.depth; r.motion = b.motion;
    r.nx = nx; r.ny = ny; r.x0 = 0; r.x1 = nx; r.stripe_w = 0; r.stripe_idx = 0; r.stripe_mod = 1;
    r.max_history = hp.max_history; r.depth_tol = hp.depth_tol;
    HIP_TRY(mpt_launch_history_resample(&r, b.part, h.stats.dev, c->stream));
    if (f_new) { if (read_back(c, f_new, b.f_new, npix * sizeof(MptVec4))) return 1; }
    else HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats) memcpy(stats, (const void *)h.stats.host.p, sizeof *stats);
    return 0;
}

extern "C" int mpt_history_kernel_time(mpt_ctx *c, double *keep_ms, double *reproject_ms, int *launches) {
    if (!c) return fail("mpt_history_kernel_time: null context");
    int keeps = 0, reprojects = 0;
    if (use_ro(c) || timer_readout(c, c->history.keep_timer, keep_ms, nullptr, &keeps) ||
        timer_readout(c, c->history.reproject_timer, reproject_ms, nullptr, &reprojects)) return 1;
    if (launches) *launches = keeps + reprojects;
    return 0;
}

// film_read.cpp -- the film's read-backs behind the C ABI of include/miptina.h: clear, resolve, the image and its hint, export, the
// raw passes; the denoised image (denoise.hip), the 8-bit display image (display.hip), the mark and the noise estimate (noise.hip),
// adaptive sampling's selection (adapt_select.hip), the four test doors and the four features' kernel timers.  Everything here runs on the main stream behind what is enqueued: of the
// launch ring (miptina.cpp) it takes mpt_flush, read_back, caller_alias and timer_readout, and it knows the early image only in
// mpt_hint_image and mpt_get_image.

#include "miptina_ctx.h"

// ------------------------------------------------------------------ what the entries share
// An argument that must be finite and positive or, with zero_ok, finite and not negative: `who` is the caller's prefix, `note` what
// the message adds to the rule
static int finite_arg(const char *who, const char *name, float v, bool zero_ok = false, const char *note = "") {
    if (std::isfinite(v) && (zero_ok ? v >= 0.0f : v > 0.0f)) return 0;
    return fail("%s: %s must be finite and %s%s, got %g", who, name, zero_ok ? "not negative" : "positive", note, (double)v);
}

int check_pass(mpt_ctx *c, int pass) {
    if (pass < 0 || pass >= 3) return fail("film pass %d out of range", pass);
    if (!c->fb.film[pass]) return fail("film size not set: call set_size() first");
    return 0;
}

// In front of an entry's work on film pass `pass`: what is enqueued is launched (the main stream then waits for the render
// launches), and the pass must be there
static int film_ready(mpt_ctx *c, int pass) { return mpt_flush(c) || check_pass(c, pass); }

// ... and the whole bracket of a read-back: film_ready, the entry's own launches and copies, which leave the main stream
// synchronised, and the look at the watchdog's flag
template <class Body>
static int film_read(mpt_ctx *c, int pass, Body body) {
    if (film_ready(c, pass) || body()) return 1;
    return check_watchdog(c);
}

// The test doors work on a film of the caller's, in buffers of their own: its size ...
static int door_film(const mpt_ctx *c, const char *who, int nx, int ny) {
    if (nx < 1 || ny < 1 || (long long)nx * ny > (long long)c->caps.max_filmsize)
        return fail("%s: film %dx%d outside 1 .. max_filmsize=%d pixels", who, nx, ny, c->caps.max_filmsize);
    return 0;
}

// ... and its accumulators on the device: room for npix of them and for what the kernels write (`bufs`), then the caller's arrays
// (acc1 may be null) into c->door.acc, and `more` of them into buffers of `bufs`
template <class Bufs>
static int door_stage(mpt_ctx *c, size_t npix, Bufs &bufs, const float *acc0, const float *acc1,
                      std::initializer_list<std::pair<DevBuf<MptVec4> *, const float *>> more = {}) {
    if (npix > c->door.cap || npix > bufs.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->door.reserve(npix) || bufs.reserve(npix)) return 1;
    }
    HIP_TRY(hipMemcpyAsync(c->door.acc[0], acc0, npix * sizeof(MptVec4), hipMemcpyHostToDevice, c->stream));
    if (acc1) HIP_TRY(hipMemcpyAsync(c->door.acc[1], acc1, npix * sizeof(MptVec4), hipMemcpyHostToDevice, c->stream));
    for (const auto &m : more) HIP_TRY(hipMemcpyAsync(m.first->p, m.second, npix * sizeof(MptVec4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                      // (the arrays are pageable: the copies are staged, the caller's arrays are free again)
    return 0;
}

// ------------------------------------------------------------------ the passes and the image
extern "C" int mpt_clear(mpt_ctx *c, int pass) {                               // filmtable.py:44-45: every pass, `id` ignored
    (void)pass;
    if (use(c)) return 1;
    size_t npix = (size_t)c->nx * c->ny;
    for (int p = 0; p < 3; p++)
        if (c->fb.film[p]) HIP_TRY(hipMemsetAsync(c->fb.film[p], 0, npix * sizeof(MptVec4), c->stream));
    c->film_version++;
    c->noise.marked = false;                     // the samples the mark counted are gone
    c->adapt.selected = false; c->adapt.count = 0;   // ... and a selection is made against a mark
    return 0;
}

extern "C" int mpt_resolve(mpt_ctx *c, int pass) {
    if (use_ro(c)) return 1;
    if (film_ready(c, pass)) return 1;
    HIP_TRY(mpt_launch_resolve(c->fb.film[pass], c->fb.resolved, (size_t)c->nx * c->ny, c->stream));
    return 0;
}

extern "C" int mpt_hint_image(mpt_ctx *c, int pass, float *out) {
    if (use_ro(c)) return 1;
    if (pass != 0) return 0;                   // only the path pass is finalised inside the render launch
    if (c->early.hint == out) return 0;
    // the old array may be the one a launch in flight is writing its image into: the caller is free to let go of it after this call
    if (c->early.ptr && c->early.ptr == c->early.hint) HIP_TRY(hipStreamSynchronize(c->stream));
    c->early.hint = out;
    c->early.ptr = nullptr;
    return 0;
}

extern "C" int mpt_get_image(mpt_ctx *c, int pass, float *out) {               // filmtable.py:47-63
    if (use_ro(c)) return 1;                   // validates the handle and makes the context's device current (round-3 ADVICE)
    const size_t bytes = (size_t)c->nx * c->ny * sizeof(MptVec4);
    if (pass == 0) {
        // The launch that rendered the frames may have written this very image already (tail finalisation, mpt_hint_image): then
        // there is nothing left to do but wait for it.  The hint is spent either way: the array is the caller's from here on.
        if (mpt_flush(c)) return 1;
        const bool early = out && c->early.ptr == out && c->early.version == c->film_version;
        if (c->early.hint == out || c->early.ptr == out) {
            if (!early && c->early.ptr == out) HIP_TRY(hipStreamSynchronize(c->stream));    // (a stale image still being written)
            c->early.hint = nullptr; c->early.ptr = nullptr;
        }
        if (early) {
            if (check_pass(c, pass)) return 1;
            // the launch's own stream: one completion signal (the main stream, which waits for the same launch before anything else
            // it is given, would add a cross-stream hop in front of the host's wake-up)
            // ... and polled, for a while, instead of slept on: the runtime's blocking wait returned 18 us after the kernel's end
            // (HIP trace), a query loop sees the completion signal within a few; a launch that runs longer than the poll window
            // falls back to the blocking wait (option "spin_us", 0 = always block)
            if (c->opt.spin_us > 0) {
                const auto t0 = std::chrono::steady_clock::now();
                for (;;) {
                    const hipError_t q = hipStreamQuery(c->early.stream);
                    if (q == hipSuccess) return check_watchdog(c);
                    if (q != hipErrorNotReady) HIP_TRY(q);
                    if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > (double)c->opt.spin_us) break;
                }
            }
            HIP_TRY(hipStreamSynchronize(c->early.stream));
            return check_watchdog(c);
        }
    }
    if (void *mapped = caller_alias(c, out, bytes)) {
        // the caller's array is page-locked memory of ours: the resolve pass writes the image straight into it over PCIe,
        // instead of into a device buffer that a DMA then copies (one dependent hop and the copy engine's start-up less)
        return film_read(c, pass, [&] {
            HIP_TRY(mpt_launch_resolve(c->fb.film[pass], (MptVec4 *)mapped, (size_t)c->nx * c->ny, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            return 0;
        });
    }
    if (mpt_resolve(c, pass)) return 1;
    if (read_back(c, out, c->fb.resolved, bytes)) return 1;
    return check_watchdog(c);
}

extern "C" int mpt_fast_export_image(mpt_ctx *c, int pass, float *out) {       // filmtable.py:66-79
    if (use_ro(c)) return 1;
    return film_read(c, pass, [&] {
        HIP_TRY(mpt_launch_export(c->fb.film[pass], c->fb.exported, c->nx, c->ny, c->stream));
        return read_back(c, out, c->fb.exported, (size_t)c->nx * c->ny * 3 * sizeof(float));
    });
}

extern "C" int mpt_get_film_raw(mpt_ctx *c, int pass, float *out) {
    if (use_ro(c)) return 1;
    return film_read(c, pass, [&] { return read_back(c, out, c->fb.film[pass], (size_t)c->nx * c->ny * sizeof(MptVec4)); });
}

// ------------------------------------------------------------------ denoised read-back (denoise.hip)
// Film pass 0 filtered by the edge-avoiding A-Trous wavelet, guided by passes 1 and 2, read back like mpt_get_image.  Reads the
// three passes, writes only the context's working buffers, and knows nothing of mpt_hint_image's array.
static int denoise_params(const mpt_denoise_params *params, mpt_denoise_params &p) {
    p = { 5, 1.0f, 0.1f, 0.3f, 1 };
    if (params) p = *params;
    if (p.iterations < 0 || p.iterations > 8) return fail("denoise: iterations must be in 0..8, got %d", p.iterations);
    return finite_arg("denoise", "sigma_color", p.sigma_color) || finite_arg("denoise", "sigma_albedo", p.sigma_albedo) ||
           finite_arg("denoise", "sigma_normal", p.sigma_normal);
}

// the buffers the filter's launches work in: the film owner's (the read-backs) or the door's
struct DnWork { MptVec4 *e[2], *a, *n; float *v[2]; };

// The filter's launches on the main stream for the accumulators f[0..2] of an nx x ny film; sigma_variance > 0: guided by the
// variance from `mark`.  *img = the working buffer that holds the image behind them; var (the door, guided): *var = the one that
// holds v_final
static int denoise_launches(mpt_ctx *c, const mpt_denoise_params &p, float sigma_variance, const MptVec4 *const f[3], const MptVec4 *mark,
                            int nx, int ny, const DnWork &w, const MptVec4 **img, const float **var = nullptr) {
    const size_t npix = (size_t)nx * ny;
    const bool guided = sigma_variance > 0.0f;
    const int demodulate = p.demodulate ? 1 : 0;
    if (p.iterations == 0) {
        // nothing to filter: the resolve pass itself, so that the image is mpt_get_image(0)'s bit for bit
        HIP_TRY(mpt_launch_resolve(f[0], w.e[0], npix, c->stream));
        *img = w.e[0];
        if (var) {                                                         // v_final is v_0: the prologue beside it
            HIP_TRY(mpt_launch_denoise_prologue(f[0], f[1], f[2], w.e[1], w.a, w.n, npix, demodulate, mark, w.v[0], c->stream));
            *var = w.v[0];
        }
        return 0;
    }
    HIP_TRY(mpt_launch_denoise_prologue(f[0], f[1], f[2], w.e[0], w.a, w.n, npix, demodulate, guided ? mark : nullptr,
                                        guided ? w.v[0] : nullptr, c->stream));
    const float ka = 1.0f / (p.sigma_albedo * p.sigma_albedo), kn = 1.0f / (p.sigma_normal * p.sigma_normal);
    for (int i = 0; i < p.iterations; i++) {
        const float sc = p.sigma_color * std::ldexp(1.0f, -i);             // the colour edge-stopping narrows as the stencil widens
        // (guided: every pixel's own tolerance, from sigma_variance^2 and the variance around it; the variance narrows by itself)
        HIP_TRY(mpt_launch_denoise_atrous(w.e[i & 1], w.e[(i + 1) & 1], w.a, w.n, nx, ny, 1 << i, guided ? sigma_variance * sigma_variance : 1.0f / (sc * sc),
                                          ka, kn, c->opt.denoise_lds, guided ? w.v[i & 1] : nullptr, guided ? w.v[(i + 1) & 1] : nullptr, c->stream));
    }
    const int last = p.iterations & 1;
    HIP_TRY(mpt_launch_denoise_epilogue(w.e[last], w.a, w.e[last ^ 1], npix, demodulate, c->stream));
    *img = w.e[last ^ 1];
    if (var) *var = w.v[last];
    return 0;
}

// mpt_get_denoised and mpt_get_display's denoised source.  In front of everything else: the guided filter needs a mark ...
static int denoise_mark(const mpt_ctx *c, const char *who) {
    if (c->denoise_variance > 0.0f && !c->noise.marked)
        return fail("%s: no mark: call mpt_film_mark() first (mpt_clear and mpt_set_size drop the mark)", who);
    return 0;
}

// ... and, once the film is ready and before the timed span, its two variance planes
static int denoise_planes(mpt_ctx *c) { return c->denoise_variance > 0.0f ? c->fb.reserve_variance() : 0; }

static int film_denoise(mpt_ctx *c, const mpt_denoise_params &p, const MptVec4 **img) {
    const MptVec4 *const f[3] = { c->fb.film[0], c->fb.film[1], c->fb.film[2] };
    const DnWork w = { { c->fb.dn_e[0], c->fb.dn_e[1] }, c->fb.dn_a, c->fb.dn_n, { c->fb.dn_v[0], c->fb.dn_v[1] } };
    return denoise_launches(c, p, c->denoise_variance, f, c->fb.mark, c->nx, c->ny, w, img);
}

extern "C" int mpt_denoise_set_variance(mpt_ctx *c, float sigma_variance) {
    if (use_ro(c)) return 1;                   // (no render launch reads it)
    if (finite_arg("mpt_denoise_set_variance", "sigma_variance", sigma_variance, true, " (0 = off)")) return 1;
    c->denoise_variance = sigma_variance;
    return 0;
}

extern "C" int mpt_denoise_get_variance(mpt_ctx *c, float *out) {
    if (use_ro(c)) return 1;
    if (!out) return fail("mpt_denoise_get_variance: null output");
    *out = c->denoise_variance;
    return 0;
}

extern "C" int mpt_get_denoised(mpt_ctx *c, const mpt_denoise_params *params, float *out) {
    if (use_ro(c)) return 1;
    mpt_denoise_params p;
    if (!out) return fail("mpt_get_denoised: null output");
    if (denoise_params(params, p) || denoise_mark(c, "mpt_get_denoised")) return 1;
    return film_read(c, 0, [&] {
        const MptVec4 *img = nullptr;
        if (denoise_planes(c)) return 1;
        MptTimedSpan span(c->denoise_timer, c->stream);
        HIP_TRY(span.begun);
        if (film_denoise(c, p, &img)) return 1;
        HIP_TRY(span.end());
        return read_back(c, out, img, (size_t)c->nx * c->ny * sizeof(MptVec4));
    });
}

// test door: the same launches on the caller's accumulators, in buffers of its own (no film pass, not the context's mark, not its
// variance setting and no film-owner buffer is touched)
extern "C" int mpt_denoise_eval(mpt_ctx *c, const mpt_denoise_params *params, float sigma_variance, const float *f0, const float *f1,
                                const float *f2, const float *mark, int nx, int ny, float *out, float *var_out) {
    if (use_ro(c)) return 1;
    mpt_denoise_params p;
    if (!out || !f0 || !f1 || !f2) return fail("mpt_denoise_eval: null %s", out ? "input" : "output");
    if (denoise_params(params, p) || finite_arg("mpt_denoise_eval", "sigma_variance", sigma_variance, true, " (0 = off)")) return 1;
    const bool guided = sigma_variance > 0.0f;
    if (guided != (mark != nullptr)) return fail("mpt_denoise_eval: the mark must be given when sigma_variance > 0 and only then");
    if (var_out && !guided) return fail("mpt_denoise_eval: var_out needs sigma_variance > 0");
    if (door_film(c, "mpt_denoise_eval", nx, ny)) return 1;
    const size_t npix = (size_t)nx * ny;
    MptDenoiseBufs &b = c->denoise_bufs;
    if (door_stage(c, npix, b, f0, mark, { { &b.f1, f1 }, { &b.f2, f2 } })) return 1;
    const MptVec4 *const f[3] = { c->door.acc[0], b.f1, b.f2 };
    const DnWork w = { { b.e[0], b.e[1] }, b.a, b.n, { b.v[0], b.v[1] } };
    const MptVec4 *img = nullptr;
    const float *var = nullptr;
    if (denoise_launches(c, p, sigma_variance, f, c->door.acc[1], nx, ny, w, &img, var_out ? &var : nullptr)) return 1;
    if (read_back(c, out, img, npix * sizeof(MptVec4))) return 1;
    if (var_out && read_back(c, var_out, var, npix * sizeof(float))) return 1;
    return 0;
}

extern "C" int mpt_denoise_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->denoise_timer, ms, nullptr, launches);
}

// ------------------------------------------------------------------ 8-bit display read-back (display.hip)
// The source tone-mapped, transfer-encoded, dithered and packed to RGBA8 on the device, read back like mpt_get_image: straight into an
// mpt_host_alloc array through its mapped pointer (option "zero_copy"), else into the film owner's image and one copy.  Reads film
// passes, writes only the context's working buffers.
static int display_params(const mpt_display_params *params, mpt_display_params &p, MptDisplayArgs &a) {
    p = { 0, MPT_TONE_ACES, MPT_TRANSFER_SRGB, MPT_LAYOUT_FILM, 1, 0.0f, 0.18f, 4.0f, 2.2f };
    if (params) p = *params;
    if (p.op < MPT_TONE_LINEAR || p.op > MPT_TONE_ACES) return fail("display: unknown op %d", p.op);
    if (p.transfer != MPT_TRANSFER_SRGB && p.transfer != MPT_TRANSFER_GAMMA) return fail("display: unknown transfer %d", p.transfer);
    if (p.layout != MPT_LAYOUT_FILM && p.layout != MPT_LAYOUT_DISPLAY) return fail("display: unknown layout %d", p.layout);
    if (finite_arg("display", "exposure", p.exposure, true, " (0 = auto)") || finite_arg("display", "key", p.key) ||
        finite_arg("display", "white", p.white) || finite_arg("display", "gamma", p.gamma)) return 1;
    a = { p.op, p.transfer, p.layout, p.dither ? 1 : 0, p.exposure, p.white * p.white, 1.0f / p.gamma };
    return 0;
}

// metering (auto exposure only) and conversion of `src` [nx*ny] into `dst` on the main stream; `dst` may be a mapped host pointer
static int display_launches(mpt_ctx *c, const mpt_display_params &p, const MptDisplayArgs &a, const MptVec4 *src, int nx, int ny,
                            MptDisplayBufs &b, uint32_t *dst) {
    const float *e_dev = nullptr;
    if (p.exposure == 0.0f) {
        HIP_TRY(mpt_launch_display_meter(src, (size_t)nx * ny, b.part, p.key, b.exposure, c->display.exposure.dev, c->stream));
        e_dev = b.exposure;
    }
    HIP_TRY(mpt_launch_display_convert(src, dst, nx, ny, &a, e_dev, c->stream));
    return 0;
}

// the bytes to the caller (zero-copy: they are there once the stream is idle) and the exposure used
static int display_finish(mpt_ctx *c, const mpt_display_params &p, bool direct, uint8_t *out, const uint32_t *dev, size_t npix, float *exposure_used) {
    if (direct) HIP_TRY(hipStreamSynchronize(c->stream));
    else if (read_back(c, out, dev, npix * 4)) return 1;
    if (exposure_used) *exposure_used = p.exposure == 0.0f ? *(volatile float *)c->display.exposure.host.p : p.exposure;
    return 0;
}

extern "C" int mpt_get_display(mpt_ctx *c, const mpt_display_params *params, const mpt_denoise_params *denoise, uint8_t *out, float *exposure_used) {
    if (use_ro(c)) return 1;
    mpt_display_params p;
    MptDisplayArgs a;
    mpt_denoise_params dp;
    if (!out) return fail("mpt_get_display: null output");
    if (display_params(params, p, a)) return 1;
    const bool denoised = p.source == MPT_DISPLAY_DENOISED;
    if (!denoised && (p.source < 0 || p.source >= 3)) return fail("display: film pass %d out of range", p.source);
    if (denoised && (denoise_params(denoise, dp) || denoise_mark(c, "mpt_get_display"))) return 1;
    return film_read(c, denoised ? 0 : p.source, [&] {
        const size_t npix = (size_t)c->nx * c->ny;
        if (denoised && denoise_planes(c)) return 1;
        void *const direct = caller_alias(c, out, npix * 4);
        const MptVec4 *src = denoised ? nullptr : c->fb.film[p.source].p;
        MptTimedSpan span(c->display.timer, c->stream);
        HIP_TRY(span.begun);
        if (denoised && film_denoise(c, dp, &src)) return 1;           // the float image stays on the device
        if (display_launches(c, p, a, src, c->nx, c->ny, c->fb.disp, direct ? (uint32_t *)direct : c->fb.disp.rgba8.p)) return 1;
        HIP_TRY(span.end());
        return display_finish(c, p, direct != nullptr, out, c->fb.disp.rgba8, npix, exposure_used);
    });
}

extern "C" int mpt_display_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->display.timer, ms, nullptr, launches);
}

// test door: the same launches on the caller's accumulators, in buffers of its own (no film pass, no film-owner buffer is touched)
extern "C" int mpt_display_eval(mpt_ctx *c, const mpt_display_params *params, const float *raw, int nx, int ny, uint8_t *out, float *exposure_used) {
    if (use_ro(c)) return 1;
    mpt_display_params p;
    MptDisplayArgs a;
    if (!out || !raw) return fail("mpt_display_eval: null %s", out ? "input" : "output");
    if (display_params(params, p, a)) return 1;
    if (door_film(c, "mpt_display_eval", nx, ny)) return 1;
    const size_t npix = (size_t)nx * ny;
    MptDisplayBufs &b = c->display.bufs;
    if (door_stage(c, npix, b, raw, nullptr)) return 1;
    if (display_launches(c, p, a, c->door.acc[0], nx, ny, b, b.rgba8)) return 1;
    return display_finish(c, p, false, out, b.rgba8, npix, exposure_used);
}

// ------------------------------------------------------------------ noise estimate (noise.hip)
// The mark is a device copy of film pass 0; the estimate compares the film with it.  Reads pass 0, writes only the mark and the
// context's working buffers, and knows nothing of mpt_hint_image's array.
extern "C" int mpt_film_mark(mpt_ctx *c) {
    if (use_ro(c)) return 1;
    if (film_ready(c, 0)) return 1;
    if (c->fb.reserve_mark()) return 1;
    HIP_TRY(hipMemcpyAsync(c->fb.mark, c->fb.film[0], (size_t)c->nx * c->ny * sizeof(MptVec4), hipMemcpyDeviceToDevice, c->stream));
    c->noise.marked = true;
    return 0;
}

// the map and the statistics of the launches just enqueued to the caller (each may be null)
static int noise_finish(mpt_ctx *c, const MptNoiseBufs &b, size_t npix, float *map, mpt_noise_stats *stats) {
    if (map) { if (read_back(c, map, b.map, npix * sizeof(float))) return 1; }
    else HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats) memcpy(stats, (const void *)c->noise.stats.host.p, sizeof *stats);
    return 0;
}

extern "C" int mpt_get_noise(mpt_ctx *c, float threshold, int remark, float *map, mpt_noise_stats *stats) {
    if (use_ro(c)) return 1;
    if (!map && !stats) return fail("mpt_get_noise: null map and null statistics");
    if (finite_arg("mpt_get_noise", "threshold", threshold, true)) return 1;
    if (!c->noise.marked) return fail("mpt_get_noise: no mark: call mpt_film_mark() first (mpt_clear and mpt_set_size drop the mark)");
    return film_read(c, 0, [&] {
        const size_t npix = (size_t)c->nx * c->ny;
        MptTimedSpan span(c->noise.timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(mpt_launch_noise(c->fb.film[0], c->fb.mark, npix, threshold, remark ? 1 : 0, map ? c->fb.noise.map.p : nullptr, c->fb.noise.part,
                                 c->noise.stats.dev, c->stream));
        HIP_TRY(span.end());
        return noise_finish(c, c->fb.noise, npix, map, stats);
    });
}

extern "C" int mpt_get_mark(mpt_ctx *c, float *out) {
    if (use_ro(c)) return 1;
    if (!out) return fail("mpt_get_mark: null output");
    if (!c->noise.marked) return fail("mpt_get_mark: no mark: call mpt_film_mark() first (mpt_clear and mpt_set_size drop the mark)");
    if (mpt_flush(c)) return 1;
    return read_back(c, out, c->fb.mark, (size_t)c->nx * c->ny * sizeof(MptVec4));
}

extern "C" int mpt_noise_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->noise.timer, ms, nullptr, launches);
}

// test door: the same launches on the caller's film and mark, in buffers of its own (no film pass and not the context's mark)
extern "C" int mpt_noise_eval(mpt_ctx *c, float threshold, const float *film_raw, const float *mark_raw, int nx, int ny, float *map,
                              float *new_mark, mpt_noise_stats *stats) {
    if (use_ro(c)) return 1;
    if (!film_raw || !mark_raw) return fail("mpt_noise_eval: null input");
    if (finite_arg("mpt_noise_eval", "threshold", threshold, true)) return 1;
    if (door_film(c, "mpt_noise_eval", nx, ny)) return 1;
    const size_t npix = (size_t)nx * ny;
    MptNoiseBufs &b = c->noise.bufs;
    if (door_stage(c, npix, b, film_raw, mark_raw)) return 1;
    MptVec4 *const film = c->door.acc[0], *const mark = c->door.acc[1];
    HIP_TRY(mpt_launch_noise(film, mark, npix, threshold, new_mark ? 1 : 0, map ? b.map.p : nullptr, b.part, c->noise.stats.dev, c->stream));
    if (noise_finish(c, b, npix, map, stats)) return 1;
    if (new_mark && read_back(c, new_mark, mark, npix * sizeof(MptVec4))) return 1;
    return 0;
}

// ------------------------------------------------------------------ adaptive sampling: the selection (adapt_select.hip)
// Which pixels of pass 0 still need samples, as a list the context keeps (fb.adapt.list) for mpt_render_selected (miptina.cpp).
// Reads pass 0 and the mark, writes neither.
static int adapt_args(const char *who, float threshold, int dilate) {
    if (finite_arg(who, "threshold", threshold, true)) return 1;
    if (dilate != 0 && dilate != 1) return fail("%s: dilate must be 0 or 1, got %d", who, dilate);
    return 0;
}

// the statistics (noise.hip's own launches: its shape of the sum gives its bits) and the list of one film and mark; the main
// stream is synchronised and the host's record read into *r
static int adapt_launches(mpt_ctx *c, const MptVec4 *film, MptVec4 *mark, int nx, int ny, float threshold, int dilate, const MptAdaptBufs &b,
                          MptTimedSpan *span, mpt_ctx::MptAdaptRecord *r) {
    mpt_ctx::MptAdaptRecord *const rec = c->adapt.rec.dev;
    HIP_TRY(mpt_launch_noise(film, mark, (size_t)nx * ny, threshold, 0, nullptr, b.part, &rec->stats, c->stream));
    HIP_TRY(mpt_launch_adapt_select(film, mark, nx, ny, threshold, dilate, b.ballot, b.count, b.list, &rec->count, c->stream));
    if (span) HIP_TRY(span->end());
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(r, (const void *)c->adapt.rec.host.p, sizeof *r);
    if (r->count < 0 || r->count > (long long)nx * ny) return fail("adaptive selection: the device counted %lld pixels of %lld", r->count, (long long)nx * ny);
    return 0;
}

extern "C" int mpt_adapt_select(mpt_ctx *c, float threshold, int dilate, mpt_noise_stats *stats, int *count) {
    if (use_ro(c)) return 1;
    if (adapt_args("mpt_adapt_select", threshold, dilate)) return 1;
    if (!c->noise.marked) return fail("mpt_adapt_select: no mark: call mpt_film_mark() first (mpt_clear and mpt_set_size drop the mark)");
    return film_read(c, 0, [&] {
        if (c->fb.reserve_adapt()) return 1;
        c->adapt.selected = false; c->adapt.count = 0;       // (the list is about to be rewritten)
        mpt_ctx::MptAdaptRecord r;
        MptTimedSpan span(c->adapt.select_timer, c->stream);
        HIP_TRY(span.begun);
        if (adapt_launches(c, c->fb.film[0], c->fb.mark, c->nx, c->ny, threshold, dilate, c->fb.adapt, &span, &r)) return 1;
        c->adapt.selected = true; c->adapt.count = (int)r.count;
        if (stats) *stats = r.stats;
        if (count) *count = (int)r.count;
        return 0;
    });
}

static int adapt_selected(const mpt_ctx *c, const char *who) {
    if (!c->adapt.selected)
        return fail("%s: no selection: call mpt_adapt_select() or mpt_adapt_set_list() first (mpt_clear and mpt_set_size drop the selection)", who);
    return 0;
}

extern "C" int mpt_adapt_get_list(mpt_ctx *c, int32_t *out, int cap, int *count) {
    if (use_ro(c)) return 1;
    if (adapt_selected(c, "mpt_adapt_get_list")) return 1;
    if (!out && !count) return fail("mpt_adapt_get_list: null list and null count");
    if (count) *count = c->adapt.count;
    if (!out) return 0;
    if (cap < c->adapt.count) return fail("mpt_adapt_get_list: room for %d indices, the selection holds %d", cap, c->adapt.count);
    if (mpt_flush(c)) return 1;
    if (c->adapt.count == 0) return 0;
    return read_back(c, out, c->fb.adapt.list, (size_t)c->adapt.count * sizeof(int32_t));
}

// is column x of the film one this context renders?
static bool own_column(const mpt_ctx *c, int x) {
    if (x < c->x0 || x >= c->x1) return false;
    return c->stripe_w == 0 || (x / c->stripe_w) % c->stripe_mod == c->stripe_idx;
}

extern "C" int mpt_adapt_set_list(mpt_ctx *c, const int32_t *pix, int count) {
    if (use_ro(c)) return 1;
    if (count < 0 || (count > 0 && !pix)) return fail("mpt_adapt_set_list: %s", count < 0 ? "count must be >= 0" : "null list");
    if (film_ready(c, 0)) return 1;
    const long long npix = (long long)c->nx * c->ny;
    for (int k = 0; k < count; k++) {
        if (pix[k] < 0 || pix[k] >= npix) return fail("mpt_adapt_set_list: entry %d = %d outside the film's [0, %lld)", k, pix[k], npix);
        if (k > 0 && pix[k] <= pix[k - 1])
            return fail("mpt_adapt_set_list: entry %d = %d after %d: the list must be strictly ascending", k, pix[k], pix[k - 1]);
        if (!own_column(c, pix[k] / c->ny))
            return fail("mpt_adapt_set_list: entry %d = %d lies in column %d, outside this context's slab or stripes", k, pix[k], pix[k] / c->ny);
    }
    if (c->fb.reserve_adapt()) return 1;
    c->adapt.selected = false; c->adapt.count = 0;
    if (count > 0) HIP_TRY(hipMemcpyAsync(c->fb.adapt.list, pix, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                      // (the caller's array is free again)
    c->adapt.selected = true; c->adapt.count = count;
    return 0;
}

// test door: the same launches on the caller's film and mark, in buffers of its own (no film pass, not the context's mark, not its
// selection); not timed
extern "C" int mpt_adapt_eval(mpt_ctx *c, float threshold, int dilate, const float *film_raw, const float *mark_raw, int nx, int ny,
                              int32_t *list_out, int cap, int *count, mpt_noise_stats *stats) {
    if (use_ro(c)) return 1;
    if (!film_raw || !mark_raw) return fail("mpt_adapt_eval: null input");
    if (!list_out && !count && !stats) return fail("mpt_adapt_eval: null outputs");
    if (adapt_args("mpt_adapt_eval", threshold, dilate)) return 1;
    if (door_film(c, "mpt_adapt_eval", nx, ny)) return 1;
    const size_t npix = (size_t)nx * ny;
    MptAdaptBufs &b = c->adapt.bufs;
    if (door_stage(c, npix, b, film_raw, mark_raw)) return 1;
    mpt_ctx::MptAdaptRecord r;
    if (adapt_launches(c, c->door.acc[0], c->door.acc[1], nx, ny, threshold, dilate, b, nullptr, &r)) return 1;
    if (count) *count = (int)r.count;
    if (stats) *stats = r.stats;
    if (!list_out) return 0;
    if (cap < r.count) return fail("mpt_adapt_eval: room for %d indices, the selection holds %lld", cap, r.count);
    return r.count ? read_back(c, list_out, b.list, (size_t)r.count * sizeof(int32_t)) : 0;
}

extern "C" int mpt_adapt_kernel_time(mpt_ctx *c, double *select_ms, double *render_ms, int *launches) {
    int selections = 0, passes = 0;
    if (use_ro(c) || timer_readout(c, c->adapt.select_timer, select_ms, nullptr, &selections) ||
        timer_readout(c, c->adapt.render_timer, render_ms, nullptr, &passes)) return 1;
    if (launches) *launches = selections + passes;
    return 0;
}

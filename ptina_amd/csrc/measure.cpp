// measure.cpp -- the measurement and test doors of the C ABI: the kernels' counters, the lane histogram and the launch timeline, the
// probe kernel, the stress copies, one device function of the hot path on rows of inputs (mpt_unit_eval), and the PathEngine
// launches' kernel time.  The engines' own timers are read where the engines are (engines.cpp, film_read.cpp).

#include "miptina_ctx.h"

// the struct is the device's twenty counters in the device's order (render_kernel.hip flush_counters)
static_assert(sizeof(mpt_counters) == 20 * sizeof(unsigned long long), "mpt_counters is read back as the device's 20 counters");
extern "C" int mpt_get_counters(mpt_ctx *c, mpt_counters *out) {
    if (use_ro(c)) return 1;
    if (mpt_flush(c)) return 1;
    HIP_TRY(hipMemcpyAsync(out, c->d_counters, sizeof *out, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// diagnostics (option "lane_hist" = 1 and "count" = 1): out[0 .. 3 x 65) = issued NODE / LEAF / SHADE stages by the number of lanes
// that took part; out[195 ..) = [stage][depth 0 .. 5][closest, shadow] lane-steps; out[231 .. 255) = the gather kernels' NODE
// lane-steps by the bucket of the node's number (0 | 1 | 2-3 | 4-7 | ...).  Zeroed by mpt_reset_counters
extern "C" int mpt_get_lane_hist(mpt_ctx *c, unsigned long long *out, int n) {
    if (use_ro(c)) return 1;
    if (!out || n < MPT_HIST_WORDS) return fail("mpt_get_lane_hist: the buffer must hold %d words", (int)MPT_HIST_WORDS);
    if (mpt_flush(c)) return 1;
    HIP_TRY(hipMemcpyAsync(out, c->d_counters + MPT_HIST_BASE, MPT_HIST_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// diagnostics: out[wave][4] = {start, scene ready, queue empty, exit} of the last LDS-kernel launch, 100 MHz ticks
extern "C" int mpt_get_timeline(mpt_ctx *c, unsigned long long *out, int cap_waves, int *nwaves) {
    if (use_ro(c)) return 1;
    if (mpt_synchronize(c)) return 1;
    if (!c->d_timeline) return fail("no timeline recorded: set option 'timeline' and render with the LDS kernel");
    int n = std::min(cap_waves, c->timeline_waves);
    if (out && n > 0)
        HIP_TRY(hipMemcpy(out, c->d_timeline, (size_t)n * MPT_TIMELINE_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (nwaves) *nwaves = c->timeline_waves;
    return 0;
}

// diagnostics: wall time from the launch of a one-workgroup kernel (threads lanes, lds_bytes of LDS) on a
// stream of its own to its completion, with whatever render launches are in flight left running -- how long
// a small foreign kernel (RCCL's) waits for a CU next to the persistent workgroups
extern "C" int mpt_probe_kernel(mpt_ctx *c, int threads, int lds_bytes, double *usec) {
    if (use_ro(c)) return 1;
    if (threads < 64 || threads > 1024 || lds_bytes < 4 * threads || lds_bytes > 64 * 1024)
        return fail("probe: threads in 64..1024, lds_bytes in 4*threads..65536");
    if (c->probe_stream.create()) return 1;
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(mpt_launch_probe(c->d_scratch + 1, threads, (size_t)lds_bytes, c->probe_stream));
    HIP_TRY(hipStreamSynchronize(c->probe_stream));
    auto t1 = std::chrono::steady_clock::now();
    if (usec) *usec = std::chrono::duration<double, std::micro>(t1 - t0).count();
    return 0;
}

// test door (tools/soak.py, the tail finalisation's soak test): `count` device-to-device copies of `mbytes` MiB enqueued on a stream
// of their own -- HBM and L2 traffic beside the render launches, whose hand-off of samples between XCDs must not care.  Returns
// at once; count = 0 waits for the copies enqueued so far.
extern "C" int mpt_stress_copies(mpt_ctx *c, int mbytes, int count) {
    if (use_ro(c)) return 1;
    if (mbytes < 1 || mbytes > 4096 || count < 0 || count > 100000) return fail("stress_copies: mbytes in 1..4096, count in 0..100000");
    if (c->stress_stream.create()) return 1;
    if (count == 0) { HIP_TRY(hipStreamSynchronize(c->stress_stream)); return 0; }
    const size_t bytes = (size_t)mbytes << 20;
    if (bytes != c->stress_bytes) {
        HIP_TRY(hipStreamSynchronize(c->stress_stream));
        c->stress_buf.release(); c->stress_bytes = 0;
        if (c->stress_buf.reserve(2 * bytes)) return 1;
        HIP_TRY(hipMemsetAsync(c->stress_buf, 0x5a, 2 * bytes, c->stress_stream));
        c->stress_bytes = bytes;
    }
    for (int k = 0; k < count; k++)
        HIP_TRY(hipMemcpyAsync(c->stress_buf + ((k & 1) ? 0 : bytes), c->stress_buf + ((k & 1) ? bytes : 0), bytes, hipMemcpyDeviceToDevice, c->stress_stream));
    return 0;
}

// test door: one device function of the hot path on rows of inputs (include/miptina.h, unit_eval.hip)
extern "C" int mpt_unit_eval(mpt_ctx *c, int kind, const void *in, int in_cols, void *out, int out_cols, int n) {
    if (use_ro(c)) return 1;
    static const int cols[MPT_UNIT_KINDS][2] = {
        { 1, 1 }, { 3, 1 }, { 2, 1 }, { 2, 1 }, { 2, 1 }, { 3, 3 }, { 3, 3 }, { 6, 3 }, { 2, 3 }, { 3, 2 }, { 6, 3 }, { 7, 4 },
        { 12, 3 }, { 30, 9 }, { 10, 1 }, { 15, 4 }, { 24, 3 }, { 24, 7 }, { 2, 1 }, { 1, 1 }, { 2, 1 },
        { 6, 6 }, { 6, 8 }, { 3, 4 }, { 3, 3 }, { 3, 22 }, { 2, 6 }, { 14, 4 },
        { 24, 3 }, { 24, 7 }, { 24, 3 }, { 24, 7 } };
    if (kind < 0 || kind >= MPT_UNIT_KINDS) return fail("unit kind %d outside [0, %d)", kind, (int)MPT_UNIT_KINDS);
    if (kind >= MPT_UNIT_DISNEY_BRDF_PLAIN && kind <= MPT_UNIT_DISNEY_BOUNCE_LEAN && c->opt.mode != MPT_MODE_FAST)
        return fail("unit kind %d is an instantiation of the production SHADE: the strict build has none (set mode to fast)", kind);
    if (in_cols != cols[kind][0] || out_cols != cols[kind][1])
        return fail("unit kind %d takes %d input and %d output columns, got %d and %d", kind, cols[kind][0], cols[kind][1],
                    in_cols, out_cols);
    if (n < 0 || (n > 0 && (!in || !out))) return fail("bad unit_eval arguments");
    if (n == 0) return 0;
    // the scene as a render launch would see it (the scene-free kinds ignore it); film, sampler and tree stay unset
    MptRenderParams p;
    memset(&p, 0, sizeof p);
    p.world_tex = -1;
    // MPT_UNIT_FACE_SIDE: one tshade record (mpt_types.h) per row, material id -1, packed HERE -- the kind tests the normal flip of
    // get_geometries only; mpt_load_model's packing of tshade is covered by the render-level tests, not by this door
    std::vector<MptVec4> shade;
    if (kind >= MPT_UNIT_LIGHT_HIT) {
        const float *rows = (const float *)in;
        if (fill_scene_params(c, p)) return 1;
        if (kind == MPT_UNIT_IMAGE_SAMPLE)
            for (int i = 0; i < n; i++) {
                const float id = rows[(size_t)i * in_cols];
                if (!(id >= 0.f && id < (float)c->h_images.size() && id == (float)(int)id))
                    return fail("unit_eval: row %d samples image %g, and %d images are loaded", i, (double)id, (int)c->h_images.size());
            }
        if (kind == MPT_UNIT_MATERIAL_GET) {
            if (c->max_mat_tex >= (int)c->h_images.size())
                return fail("unit_eval: a material names texture %d, and %d images are loaded", c->max_mat_tex, (int)c->h_images.size());
            for (int i = 0; i < n; i++) {
                const float id = rows[(size_t)i * in_cols];
                if (!(id >= -1.f && id < (float)c->nmats && id == (float)(int)id))
                    return fail("unit_eval: row %d asks for material %g outside [-1, %d), the records loaded", i, (double)id, c->nmats);
            }
        }
        if (kind == MPT_UNIT_FACE_SIDE) {
            shade.resize((size_t)n * 4);
            const int none = -1;
            for (int i = 0; i < n; i++) {
                const float *vn = rows + (size_t)i * in_cols + 3;
                MptVec4 *s = &shade[(size_t)i * 4];
                s[0] = { vn[0], vn[1], vn[2], vn[3] }; s[1] = { vn[4], vn[5], vn[6], vn[7] };
                s[2] = { vn[8], 0.f, 0.f, 0.f }; s[3] = { 0.f, 0.f, 0.f, 0.f };
                memcpy(&s[3].w, &none, 4);
            }
        }
    }
    DevBuf<float> d_in, d_out;
    DevBuf<MptVec4> d_shade;
    if (d_in.reserve((size_t)n * in_cols) || d_out.reserve((size_t)n * out_cols) || d_shade.reserve(shade.size())) return 1;
    hipError_t e = hipMemcpyAsync(d_in, in, (size_t)n * in_cols * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && d_shade) e = hipMemcpyAsync(d_shade, shade.data(), shade.size() * sizeof(MptVec4), hipMemcpyHostToDevice, c->stream);
    p.tshade = d_shade;
    if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, (size_t)n * out_cols * 4, c->stream);
    if (e == hipSuccess) e = MPT_LAUNCHER(c, mpt_launch_unit_eval)(&p, kind, d_in, in_cols, d_out, out_cols, n, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * out_cols * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail("mpt_unit_eval: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int mpt_reset_counters(mpt_ctx *c) {
    if (use(c)) return 1;
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, MPT_COUNTER_WORDS * sizeof(unsigned long long), c->stream));
    return 0;
}

extern "C" int mpt_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->render_timer, ms, nullptr, launches, true);
}

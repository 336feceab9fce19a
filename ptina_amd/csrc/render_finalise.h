// render_finalise.h -- production build of render_kernel.hip (its only includer): the tail finalisation of a launch.
#pragma once

// ---------------------------------------------------------------- tail finalisation
// A launch ends with a drain: the queues are dry, waves finish their last paths and leave one by one (a third of a millisecond
// on the benchmark film), and only then could the combine pass, the resolve pass and the read-back start -- 0.14 ms more per
// step.  With p.fin_counter set, a wave that has nothing left to trace turns to the film instead: it takes the next tile of the
// share (tiles finish in the order their items were issued, so all but the last few are complete), waits until every sample of
// it carries this launch's tag, adds the frames to the film in frame order (film_ops.h: the combine pass's arithmetic), and writes
// the resolved pixels to the caller's image as well when the host knows where get_image() will want them.  The slab entries were
// stored write-through (store_sample) and are read here with sc1 loads (L1 bypassed, re-read every pass: R2 of the guide).
// Nothing waits for a finishing wave, and what IT waits for is in the hands of waves that are running (every item has been pulled
// before the first wave gets here), so the loop ends; a bounded spin raises the watchdog instead of hanging if it ever does not.
DEV mpt_u4 slab_load_sc1(const MptVec4 *frame_base, unsigned frame_bytes, unsigned byte_off) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)frame_base, (short)0, (int)frame_bytes, 0x00020000);
#ifndef MPT_FIN_AUX
#define MPT_FIN_AUX 16       // cache bits of the slab loads: 16 = sc1 (A/B: 18 = sc1 nt)
#endif
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, MPT_FIN_AUX);      // aux 16 = sc1
}

#ifndef MPT_FIN_SLEEP
#define MPT_FIN_SLEEP 32     // units of 64 cycles between two looks at a tile that is not complete yet
#endif
#ifndef MPT_FIN_GROUP_LDS
#define MPT_FIN_GROUP_LDS 8       // slab loads in flight per lane: the LDS-resident kernel has 128 VGPRs to lend ...
#define MPT_FIN_GROUP_GATHER 6    // ... the gather kernels 96 (with eight the function needs 102 and they would lose their fifth wave per SIMD)
#endif
// Out of line: inlined into the render kernels the finalisation moved their register allocation and the traversal loop ran
// 3 % slower (MI355X, same box: 3.21 against 3.13 ms per launch, profiles/r04_ab_experiments.json); as a function of its own it
// leaves them alone, at the price of its registers counting for every kernel that calls it (MPT_FIN_GROUP_*).
// what finalise_tiles reads of the launch parameters.  Out of line, its arguments arrive in vector registers: the ones a buffer
// descriptor is made of are made scalar again (readfirstlane; they are wave-uniform)
struct FinArgs {
    MptVec4 *partial, *film0, *image_out;
    unsigned int *fin_counter, *watchdog;
    int tile_w_shift, tile_h_shift, ny, nitems, nchunks, nframes, partial_stride, stripe_w, stripe_pitch, x0, x1;
    unsigned slab_tag;
};
DEV int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <class T> DEV T *uniform_p(T *ptr) {
    const unsigned long long v = (unsigned long long)ptr;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (T *)(((unsigned long long)hi << 32) | lo);
}
// (individual parameters, not a struct by value: that one would travel through scratch memory)
template <int GROUP>
__device__ __attribute__((noinline)) int finalise_tiles_impl(
        MptVec4 *a_partial, MptVec4 *a_film0, MptVec4 *a_image_out, unsigned int *a_fin_counter, unsigned int *a_watchdog,
        int a_tws, int a_ths, int a_ny, int a_nitems, int a_nchunks, int a_nframes, int a_partial_stride, int a_stripe_w,
        int a_stripe_pitch, int a_x0, int a_x1, unsigned a_slab_tag) {
    FinArgs p;
    p.partial = a_partial; p.film0 = a_film0; p.image_out = a_image_out; p.fin_counter = a_fin_counter; p.watchdog = a_watchdog;
    p.tile_w_shift = a_tws; p.tile_h_shift = a_ths; p.ny = a_ny; p.nitems = a_nitems; p.nchunks = a_nchunks; p.nframes = a_nframes;
    p.partial_stride = a_partial_stride; p.stripe_w = a_stripe_w; p.stripe_pitch = a_stripe_pitch; p.x0 = a_x0; p.x1 = a_x1;
    p.slab_tag = a_slab_tag;
    p.partial = uniform_p(p.partial); p.partial_stride = uniform_i(p.partial_stride); p.nframes = uniform_i(p.nframes);
    p.tile_w_shift = uniform_i(p.tile_w_shift); p.tile_h_shift = uniform_i(p.tile_h_shift);
    const int lane = threadIdx.x & 63;
    const int tws = p.tile_w_shift, ths = p.tile_h_shift, tps = tws + ths;
    const int t8y = (p.ny + (1 << ths) - 1) >> ths;
    const int ntile = p.nitems / p.nchunks;                 // items are tile-major: nchunks per tile
    const int B = p.nframes;
    const unsigned frame_bytes = (unsigned)p.partial_stride * 16u;      // (a frame of the slab is far below 4 GiB: the film's cap is 2^26 pixels)
    const unsigned tag = p.slab_tag;
    const mpt_u4 absent = slab_pack(0.0f, 0.0f, 0.0f, tag);     // a frame past the batch's end, a pixel past the film's edge: ready, adds nothing
    const unsigned long long t_begin = wall_clock64();
    int done = 0;
    for (;; done++) {
        int t = 0;
        if (lane == 0) t = (int)atomicAdd(p.fin_counter, 1u);
        t = __builtin_amdgcn_readfirstlane(t);
        if (t >= ntile) break;
        const int tx = t / t8y, ty = t - tx * t8y;
        const int tps_x = p.stripe_w >> tws, st = tx / tps_x;            // stripe of this tile column (as in trace_stream)
        const int ti = p.x0 + st * p.stripe_pitch + ((tx - st * tps_x) << tws), tj = ty << ths;
        for (int q0 = 0; q0 < (1 << tps); q0 += 64) {                    // (wave-uniform trip count)
            const int q = q0 + lane;
            const int i = ti + (q >> ths), j = tj + (q & ((1 << ths) - 1));
            const bool inside = q < (1 << tps) && i < p.x1 && j < p.ny;  // (pixels of the tile past the film's edge get no samples)
            const unsigned off = (unsigned)(((tx << tws) + (q >> ths)) * p.ny + (tj + (q & ((1 << ths) - 1)))) * 16u;
            const size_t pix = (size_t)i * p.ny + j;
            MptVec4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (inside) acc = p.film0[pix];
            for (int f0 = 0; f0 < B; f0 += GROUP) {
                mpt_u4 v[GROUP];
                for (;;) {
                    bool ready = true;
#pragma unroll
                    for (int k = 0; k < GROUP; k++) {
                        v[k] = absent;
                        if (f0 + k < B && inside) v[k] = slab_load_sc1(p.partial + (size_t)(f0 + k) * (size_t)p.partial_stride, frame_bytes, off);
                        ready = ready && slab_ready(v[k], tag);       // each 8-byte half on its own tag (film_ops.h)
                    }
                    if (__ballot(!ready) == 0ull) break;
                    if (wall_clock64() - t_begin > 400000000ull) {       // 4 s at 100 MHz: some sample never came
                        if (lane == 0) __hip_atomic_store(p.watchdog, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        return done;
                    }
                    __builtin_amdgcn_s_sleep(MPT_FIN_SLEEP);
                }
#pragma unroll
                for (int k = 0; k < GROUP; k++)
                    if (f0 + k < B) film_add_sample(acc, slab_r(v[k]), slab_g(v[k]), slab_b(v[k]));
            }
            if (inside) {
                p.film0[pix] = acc;
                if (p.image_out) p.image_out[pix] = film_resolve(acc);
            }
        }
    }
    return done;
}

// GROUP = slab loads in flight per lane: what the calling kernel's register budget allows (see finalise_tiles_impl)
template <int GROUP>
DEV int finalise_tiles(const MptRenderParams &p) {
    // In a workgroup of three or four waves per SIMD only the younger two finalise.  The hardware issues the oldest wave of a
    // SIMD first, so the old waves finish tracing first -- and, finalising, stayed in front of the waves still tracing behind
    // them: with all four at it the launch took 3.15 ms, with the younger two 3.12 (the combine pass after the launch: 3.10 + 0.1;
    // MI355X, same box, profiles/r04_ab_experiments.json).  Every tile is still taken by somebody: the loop runs until none is left.
#ifndef MPT_FIN_YOUNG
#define MPT_FIN_YOUNG 2
#endif
    if ((blockDim.x >> 8) >= 3 && (int)((threadIdx.x >> 8) & 3) < MPT_FIN_YOUNG) return 0;
    if (p.fin_counter)
        return finalise_tiles_impl<GROUP>(p.partial, p.film0, p.image_out, p.fin_counter, p.watchdog, p.tile_w_shift, p.tile_h_shift, p.ny,
                                          p.nitems, p.nchunks, p.nframes, p.partial_stride, p.stripe_w, p.stripe_pitch, p.x0, p.x1, p.slab_tag);
    return 0;
}

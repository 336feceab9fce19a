// render_kernel.hip -- the per-pixel path-trace megakernels (PathEngine._render + do_render +
// path_trace, engine/path.py:18-93) and the AOV preview kernel (engine/preview.py:23-41).
//
// Built twice from this one source: MPT_STRICT=1 -> symbols mpt_launch_*_strict,
// MPT_STRICT=0 -> mpt_launch_*_fast (see pt_device.h).
//
// Fast build (gfx950, wave64) -- see trace_stream:
//   * persistent workgroups pull (8x8 pixel tile, chunk of frames) work items from eight per-XCD queues
//     with stealing; a wave's item is a pool of samples and lanes are NOT tied to pixels: idle lanes are
//     compacted with ballot + mbcnt and handed the next samples the moment their path ends;
//   * the wave runs an in-wave state machine (NODE / LEAF steps in a tight loop, then one SHADE stage
//     per bounce, then NEW) so that each issued stage has as many ready lanes as possible;
//   * every sample's radiance is stored to a [frame][pixel] slab and a combine pass adds the frames
//     to the film in frame order: the reference's summation order, no float atomics, bit-reproducible
//     and identical for any slab split across GPUs.
//   render_kernel_fast (any scene size): 256-lane workgroups, 4 waves per SIMD, scene records gathered
//     from HBM / L2 / Infinity Cache, per-lane int32 traversal stack in LDS, [level][lane].
//   After the loop a wave that has run out of work finalises finished tiles of the film -- sum of the frames, resolve, the image's
//     write-out -- while the others drain (finalise_tiles): a launch that has the GPU to itself needs no combine pass.
//   render_kernel_wide: 4-wide nodes with 8-bit child boxes (the product path for scenes that do not fit LDS).
//   render_kernel_lds (scenes whose node + triangle records fit the CU's 160 KiB LDS): measured on
//     MI355X the gather version spends its time in the vector L1 -- a wave's node fetch touches up to 64
//     different cache lines per load instruction, four instructions per node -- so one persistent
//     1024-lane workgroup per CU copies the records into LDS once and every traversal step becomes four
//     ds_read_b128; int16 stacks.
// Strict build: one lane per pixel, frames summed in a register in order, the reference's traversal;
//   one 16x16 tile per workgroup, blockIdx remapped so an XCD's blocks cover a contiguous run of tiles.

#include "path_common.h"
#include "film_ops.h"
#include <atomic>

template <bool COUNT>
DEV void flush_counters(const MptRenderParams &p, const Cnt &c) {
    if (!COUNT) return;
    unsigned v[20] = { c.samples, c.rays, c.n_box, c.n_tri, c.n_shade, c.n_draws, c.bounces, c.n_node,
                       c.it_node, c.it_leaf, c.it_shade, c.it_new,
                       c.pl_local, c.pl_batches, c.pl_batch_lanes, c.pl_prim, c.pl_tidle, c.pl_sidle, c.pl_trips, c.pl_taken };
#pragma unroll
    for (int k = 0; k < 20; k++) {
        unsigned x = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd(p.counters + k, (unsigned long long)x);
    }
}

// Strict build: a lane owns ONE pixel and walks the batch's frames in order; the film sum is
// kept in a register and grows in exactly the reference's order (filmtable.py:37-39, path.py:93).
template <bool COUNT, class TR>
DEV void trace_pixel(const MptRenderParams &p, const TR &tr, int i, int j, int f, int fend, Cnt &cnt) {
    const int pix = i * p.ny + j;
    MptVec4 acc = p.film0[pix];
    PathState s;
    for (; f < fend; f++) {
        path_begin<COUNT>(p, s, i, j, f, cnt);
        while (!path_step<COUNT>(p, tr, s, cnt)) {}
        acc.x += s.result.x; acc.y += s.result.y; acc.z += s.result.z; acc.w += 1.0f;   // path.py:93
    }
    p.film0[pix] = acc;
}

#if !MPT_STRICT
// the wave state machine of the production build: lane state and traversal steps | SHADE, work queues, trace_stream | tail finalisation
#include "render_lane.h"
#include "render_shade.h"
#include "render_finalise.h"
#include "render_lds_setup.h"     // the LDS copy-in and launch, shared with the test door (walk_eval.hip)
#endif

// ---------------------------------------------------------------- gather kernel: 16x16 tile x chunk per workgroup
#if MPT_STRICT
#define MPT_RENDER_BOUNDS __launch_bounds__(MPT_BLOCK)
#else
// gathers from L2 / Infinity Cache are latency-bound: ask for 4 waves per SIMD (the 32-level kernels then sit at the 128-VGPR
// cap; tools/kernel_resources.py prints registers / scratch of every kernel as built)
#define MPT_RENDER_BOUNDS __launch_bounds__(MPT_BLOCK, 4)
#endif
template <int STACK, bool COUNT>
__global__ MPT_RENDER_BOUNDS void MPT_SUFFIX(render_kernel)(const MptRenderParams p) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    Cnt cnt = {};
#if MPT_STRICT
    // one 16x16 tile per workgroup, every frame of the batch; blockIdx remapped for XCD locality
    int tile = xcd_remap(blockIdx.x, gridDim.x);
    int i, j;
    if (tile_pixel(p, tile, &i, &j)) trace_pixel<COUNT>(p, tr, i, j, 0, p.nframes, cnt);
#else
    // persistent workgroups pulling (8x8 tile, chunk) items; see WorkQueue
    WorkQueue wq; wq.ctr = p.work_counter; wq.nitems = p.nitems; wq.q0 = blockIdx.x & 7; wq.qoff = 0;
    trace_stream<COUNT, MPT_FEAT_GENERIC>(p, tr.w, tr.st, wq, cnt);
    finalise_tiles<MPT_FIN_GROUP_GATHER>(p);
#endif
    flush_counters<COUNT>(p, cnt);
}

#if !MPT_STRICT
// ---------------------------------------------------------------- gather kernel over 4-wide nodes
#ifndef MPT_WIDE_WAVES
#define MPT_WIDE_WAVES 5      // waves per SIMD the 4-wide gather kernel is compiled for (its register budget: 512 / this = 96 VGPRs).
                              // At 96 the allocator parks 27 dwords per lane in scratch, all of them in the shading pass (SHADE's own
                              // temporaries and the prepared primary rays), none in the traversal loop: MI355X C4 1520 -> 1580,
                              // C5 778 -> 825 Msamples/s.  Six waves (80 VGPRs) spill into the steps and lose a third.
#endif
template <bool COUNT, bool QUANT>
__global__ __launch_bounds__(MPT_BLOCK, MPT_WIDE_WAVES) void render_kernel_wide(const MptRenderParams p) {
    typedef GatherWalk4<QUANT> Walk;
    __shared__ int s_stack[Walk::CAP * MPT_BLOCK];
    typename Walk::Lifo stk;
    stk.stack = s_stack + threadIdx.x;
    stk.spill = p.stack_spill;
    stk.lane_off = (blockIdx.x * MPT_BLOCK + threadIdx.x) * (unsigned)Walk::SPILL;   // (grid x 256 x 88 entries: far below 2^32)
    stk.sp = 0;
    Cnt cnt = {};
    WorkQueue wq; wq.ctr = p.work_counter; wq.nitems = p.nitems; wq.q0 = blockIdx.x & 7; wq.qoff = 0;
    Walk w; w.wnode = QUANT ? p.qnode : p.wnode; w.tgeo = p.tfast;
    trace_stream<COUNT, MPT_FEAT_GENERIC>(p, w, stk, wq, cnt);
    finalise_tiles<MPT_FIN_GROUP_GATHER>(p);
    flush_counters<COUNT>(p, cnt);
}

// ---------------------------------------------------------------- LDS-resident persistent kernel
// dynamic LDS: [ (n-1) node records of MPT_LDS_NODE_STRIDE bytes, padded to 16 | n*3 triangle float4 (tfast) | (default_mtl+1)*6 material float4 |
//                n material-record bytes, padded to 16 | lds_stack x 1024 int16 ]     (lds_layout.h mpt_lds_regions: the host sizes the launch by it)
// the wave's record of the launch timeline (option "timeline"; include/miptina.h mpt_get_timeline), or null
DEV unsigned long long *lds_timeline(const MptRenderParams &p) {
    return p.timeline ? p.timeline + MPT_TIMELINE_WORDS * (size_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) : nullptr;
}

template <bool COUNT>
__global__ __launch_bounds__(MPT_LDS_BLOCK) void render_kernel_lds(const MptRenderParams p) {
    extern __shared__ __attribute__((aligned(16))) MptVec4 smem[];
    const MptLdsRegions lay = mpt_lds_regions(p.n, p.default_mtl);
    unsigned long long *tl = lds_timeline(p);
    if (tl && (threadIdx.x & 63) == 0) tl[0] = wall_clock64();
    {   // one copy of the scene per CU: coalesced 16-B loads, ds_write_b128
        lds_copy_nodes(p, smem);
        lds_copy_tris_mats<false>(p, smem, lay, p.default_mtl);
    }
    __syncthreads();
    if (tl && (threadIdx.x & 63) == 0) tl[1] = wall_clock64();

    LdsWalk w;
    LdsWalk::Lifo stk;
    w.fnode = (LdsVec4Ptr)(void *)smem;
    lds_walk_regions(w, stk, smem, lay);
    w.mat_last = p.default_mtl; w.mat_default = p.default_mtl;
    Cnt cnt = {};
    WorkQueue wq; wq.ctr = p.work_counter; wq.nitems = p.nitems; wq.q0 = blockIdx.x & 7; wq.qoff = 0;
    trace_stream<COUNT, MPT_FEAT_GENERIC>(p, w, stk, wq, cnt, tl);
    if (tl && (threadIdx.x & 63) == 0) tl[3] = wall_clock64();
    const int fin_tiles = finalise_tiles<MPT_FIN_GROUP_LDS>(p);
    if (tl && (threadIdx.x & 63) == 0) { tl[4] = wall_clock64(); tl[5] = (unsigned long long)fin_tiles; }   // left the finalisation; tiles it did
    flush_counters<COUNT>(p, cnt);
}

// ---------------------------------------------------------------- LDS-resident persistent kernel over the 4-wide nodes
// dynamic LDS: [ nwide node records of MPT_LDS4_NODE_STRIDE bytes | (n+1)*3 triangle float4 (tfast; record n: the unused slots' NaNs) |
//                (lds_nmats+1)*6 material float4 (the records the model uses, then the default one) | n material-record bytes,
//                padded to 16 | lds_stack x 1024 int16 ]     (lds_layout.h mpt_lds4_regions)
// Two instantiations per COUNT: FEAT = MPT_FEAT_GENERIC (every region of SHADE) and MPT_FEAT_PLAIN, launched for a plain scene
// (untextured materials without clearcoat or transmission, one light, no environment map: the headline scene and BASELINE's
// configs 1, 2, 3, 5): without the texture, environment-map and light-list regions and without the clearcoat and transmission
// lobes (shade_feat.h: what keeps its film the generic one's bit for bit).  A third, LEAN, is the plain one for a scene whose
// materials all have sheen and subsurface exactly zero (shade_feat.h shade_lean_scene: the headline scene, s34, the default
// material, everything a glTF file becomes): without the two terms of the diffuse lobe they multiply, the same film again
template <bool COUNT, int FEAT, bool LEAN = false>
__global__ __launch_bounds__(MPT_LDS_BLOCK) void render_kernel_lds4(const MptRenderParams p) {
    static_assert(!LEAN || FEAT == MPT_FEAT_PLAIN, "the lean variant is instantiated with the plain mask only");
    extern __shared__ __attribute__((aligned(16))) MptVec4 smem[];
    const MptLdsRegions lay = mpt_lds4_regions(p.n, p.nwide, p.lds_nmats);
    unsigned long long *tl = lds_timeline(p);
    if (tl && (threadIdx.x & 63) == 0) tl[0] = wall_clock64();
    {
        lds_copy_nodes4(p, smem);
        lds_copy_tris_mats<true>(p, smem, lay, p.lds_nmats);
    }
    __syncthreads();
    if (tl && (threadIdx.x & 63) == 0) tl[1] = wall_clock64();

    if (!lds_starts_at_zero(smem)) {
        if (threadIdx.x == 0) __hip_atomic_store(p.watchdog, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    LdsWalk4 w;
    LdsWalk4::Lifo stk;
    lds_walk_regions(w, stk, smem, lay);
    w.mat_last = p.lds_nmats; w.mat_default = p.default_mtl;
    stk.ts = p.t_scale;
    Cnt cnt = {};
    WorkQueue wq; wq.ctr = p.work_counter; wq.nitems = p.nitems; wq.q0 = blockIdx.x & 7; wq.qoff = 0;
    trace_stream<COUNT, FEAT, LEAN>(p, w, stk, wq, cnt, tl);
    if (tl && (threadIdx.x & 63) == 0) tl[3] = wall_clock64();
    const int fin_tiles = finalise_tiles<MPT_FIN_GROUP_LDS>(p);
    if (tl && (threadIdx.x & 63) == 0) { tl[4] = wall_clock64(); tl[5] = (unsigned long long)fin_tiles; }
    flush_counters<COUNT>(p, cnt);
}
#endif

// PreviewEngine._render, engine/preview.py:23-41
template <int STACK>
__global__ __launch_bounds__(MPT_BLOCK) void MPT_SUFFIX(preview_kernel)(const MptRenderParams p) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    int tile = xcd_remap(blockIdx.x, gridDim.x);
    int i, j;
    if (!tile_pixel(p, tile, &i, &j)) return;
    const int pix = i * p.ny + j;
    const int h = wanghash2(i, j);
    Cnt cnt = {};
    MptVec4 a1 = p.film1[pix], a2 = p.film2[pix];
    for (int f = 0; f < p.nframes; f++) {
        Rng rng; rng.dim = p.sobol_dim; rng.P = p.P + (size_t)f * p.sobol_dim; rng.i = h;
        V3 albedo = v3s(0.0f), normal = v3s(0.0f);
        float dx = rng_random(rng), dy = rng_random(rng);
        float x = m_div((float)i + dx, (float)p.nx) * 2.0f - 1.0f;
        float y = m_div((float)j + dy, (float)p.ny) * 2.0f - 1.0f;
        V3 ro, rd;
        camera_generate(p, x, y, &ro, &rd);
        Hit hit = tr.template closest<false>(ro, rd, -1, cnt);
        if (hit.hit == 1) {
            V3 hitpos; Disney material;
            get_geometries(p, hit, ro, rd, &hitpos, &normal, material);
            albedo = material.basecolor;
        }
        a1.x += albedo.x; a1.y += albedo.y; a1.z += albedo.z; a1.w += 1.0f;
        a2.x += normal.x; a2.y += normal.y; a2.z += normal.z; a2.w += 1.0f;
    }
    p.film1[pix] = a1;
    p.film2[pix] = a2;
}

// ---------------------------------------------------------------- host-side launchers
template <class K>
static int blocks_per_cu(K kernel) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, MPT_BLOCK, 0) != hipSuccess || nb < 1) nb = 2;
    return nb;
}

typedef void (*RenderKernelFn)(const MptRenderParams);
#if !MPT_STRICT
// occupancy answers are per device (the C ABI allows one context per GPU in a process): asked once per device and kernel variant
static hipError_t cached_blocks_per_cu(std::atomic<int> (*cache)[4], const RenderKernelFn (&variants)[4], int v, int *occ) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MPT_MAX_DEVICES) return hipErrorInvalidDevice;
    *occ = cache[dev][v].load(std::memory_order_relaxed);
    if (!*occ) {
        *occ = blocks_per_cu(variants[v]);
        cache[dev][v].store(*occ, std::memory_order_relaxed);
    }
    return hipSuccess;
}
#endif

// strict build: grid = number of 16x16 tiles.  fast build: persistent workgroups, `grid` = number of CUs
// (scaled here by the blocks each CU can hold); the work items come from p->work_counter.
MPT_KERNEL_API hipError_t MPT_SUFFIX(mpt_launch_render)(const MptRenderParams *p, int grid, int stack, int count,
                                                     hipStream_t stream) {
    // the instantiations, by (stack levels, count)
    static const RenderKernelFn variants[4] = { MPT_SUFFIX(render_kernel)<32, false>, MPT_SUFFIX(render_kernel)<32, true>,
                                                MPT_SUFFIX(render_kernel)<64, false>, MPT_SUFFIX(render_kernel)<64, true> };
    const int v = 2 * stack_instantiation(stack) + (count ? 1 : 0);
#if !MPT_STRICT
    static std::atomic<int> occ_cache[MPT_MAX_DEVICES][4];
    int occ = 0;
    if (hipError_t e = cached_blocks_per_cu(occ_cache, variants, v, &occ)) return e;
    grid *= occ;
#endif
    hipLaunchKernelGGL(variants[v], dim3(grid), dim3(MPT_BLOCK), 0, stream, *p);
    return hipGetLastError();
}

#if !MPT_STRICT
// the same over the 4-wide nodes (p->wnode, p->nwide); feat: the instantiation (shade_feat.h: MPT_FEAT_PLAIN or MPT_FEAT_GENERIC --
// there is no kernel for any other mask, and asking for one is an error, not a fall-back); lean: the lean variant, which only the
// plain mask has
MPT_KERNEL_API hipError_t mpt_launch_render_lds4(const MptRenderParams *p, int grid, int block, size_t lds_bytes, int count, int feat,
                                             int lean, hipStream_t stream) {
    if (lean && feat != MPT_FEAT_PLAIN) return hipErrorInvalidValue;
    if (lean)
        return count ? launch_whole_lds<render_kernel_lds4<true, MPT_FEAT_PLAIN, true>>(grid, block, lds_bytes, stream, *p)
                     : launch_whole_lds<render_kernel_lds4<false, MPT_FEAT_PLAIN, true>>(grid, block, lds_bytes, stream, *p);
    if (feat == MPT_FEAT_PLAIN)
        return count ? launch_whole_lds<render_kernel_lds4<true, MPT_FEAT_PLAIN>>(grid, block, lds_bytes, stream, *p)
                     : launch_whole_lds<render_kernel_lds4<false, MPT_FEAT_PLAIN>>(grid, block, lds_bytes, stream, *p);
    if (feat != MPT_FEAT_GENERIC) return hipErrorInvalidValue;
    return count ? launch_whole_lds<render_kernel_lds4<true, MPT_FEAT_GENERIC>>(grid, block, lds_bytes, stream, *p)
                 : launch_whole_lds<render_kernel_lds4<false, MPT_FEAT_GENERIC>>(grid, block, lds_bytes, stream, *p);
}

MPT_KERNEL_API hipError_t mpt_launch_render_lds(const MptRenderParams *p, int grid, int block, size_t lds_bytes, int count,
                                            hipStream_t stream) {
    return count ? launch_whole_lds<render_kernel_lds<true>>(grid, block, lds_bytes, stream, *p)
                 : launch_whole_lds<render_kernel_lds<false>>(grid, block, lds_bytes, stream, *p);
}
#endif

#if !MPT_STRICT
// Disney.__init__'s derived terms (disney.py:36-50) of every material record, once per upload: the production
// material fetch then reads them instead of re-deriving them at every hit (same device function: same bits)
__global__ void derive_materials_kernel(MptMaterial *mats, int count) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    MptMaterial *mt = mats + i;
    Disney m;
    m.basecolor = v3(mt->p[0], mt->p[1], mt->p[2]);
    m.metallic = mt->p[3]; m.roughness = mt->p[4]; m.specular = mt->p[5]; m.specularTint = mt->p[6];
    m.subsurface = mt->p[7]; m.sheen = mt->p[8]; m.sheenTint = mt->p[9]; m.clearcoat = mt->p[10];
    m.clearcoatGloss = mt->p[11]; m.transmission = mt->p[12]; m.ior = mt->p[13];
    disney_init(m);
    mt->d[0] = m.speccolor.x; mt->d[1] = m.speccolor.y; mt->d[2] = m.speccolor.z;
    mt->d[3] = m.sheencolor.x; mt->d[4] = m.sheencolor.y; mt->d[5] = m.sheencolor.z;
    mt->d[6] = m.alpha; mt->d[7] = m.clearcoatAlpha;
    mt->p[14] = __int_as_float(mt->any_tex);
}

MPT_KERNEL_API hipError_t mpt_launch_derive_materials(MptMaterial *mats, int count, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(derive_materials_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, mats, count);
    return hipGetLastError();
}

// the 4-wide gather kernel's instantiations, by (quant, count)
static const RenderKernelFn wide_variants[4] = { render_kernel_wide<false, false>, render_kernel_wide<true, false>,
                                                 render_kernel_wide<false, true>, render_kernel_wide<true, true> };
static int wide_variant(int count, int quant) { return (quant ? 2 : 0) + (count ? 1 : 0); }

// persistent workgroups over 4-wide nodes; `grid` = number of CUs (scaled here by the blocks each CU can hold);
// *blocks = workgroups launched (the spill strip must hold blocks x 256 lanes x GatherWalk4::SPILL entries)
MPT_KERNEL_API hipError_t mpt_wide_blocks(int grid, int count, int quant, int *blocks) {
    static std::atomic<int> occ_cache[MPT_MAX_DEVICES][4];
    int occ = 0;
    if (hipError_t e = cached_blocks_per_cu(occ_cache, wide_variants, wide_variant(count, quant), &occ)) return e;
    *blocks = grid * occ;
    return hipSuccess;
}

MPT_KERNEL_API hipError_t mpt_launch_render_wide(const MptRenderParams *p, int blocks, int count, int quant, hipStream_t stream) {
    hipLaunchKernelGGL(wide_variants[wide_variant(count, quant)], dim3(blocks), dim3(MPT_BLOCK), 0, stream, *p);
    return hipGetLastError();
}
#endif

MPT_KERNEL_API hipError_t MPT_SUFFIX(mpt_launch_preview)(const MptRenderParams *p, int grid, int stack,
                                                      hipStream_t stream) {
    return launch_by_stack<MPT_SUFFIX(preview_kernel)<32>, MPT_SUFFIX(preview_kernel)<64>>(stack, grid, stream, *p);
}

// walk_eval.hip -- test door through the traversal of the production PathEngine kernels (mpt_walk_trace, tree_query.cpp; DESIGN.md
// section 3.16): any ray a caller likes -- a bounce ray that starts on a surface and avoids it, a shadow ray, a ray along an axis --
// through the in-wave state machine of render_lane.h (lane_start_ray, stage_node / stage_node4, stage_leaf, classify) over each of
// the five walk types of pt_device.h, which the render kernels otherwise run for rays of their own making only.
//
// Production build only, compiled with the render kernels' flags.  Nothing of a walk is restated here: a kernel sets its walk up as
// the render kernel of that walk does (make_block_tracer; render_kernel_wide's LIFO with a spill strip; the LDS copy-in, regions and
// address check of render_lds_setup.h), starts lane i's ray as lane_begin_ray does, and steps it with the render kernels' stages until
// the lane's state is neither NODE nor LEAF.  What comes out is what SHADE would be handed (render_shade.h): hidx >= 0, the
// slot in hidx, tbest (unscaled where the walk scales it), hu, hv -- no second evaluation of the hit.
// With a.dis the rays are shadow rays and a.hit holds "occluded", hidx >= 0, as the shading pass reads it.
//
// Shape: one lane per ray.  The gather walks run MPT_BLOCK lanes per workgroup with the stacks of their render kernels (32 or 64
// levels of int32 in LDS; 4-wide: Walk::CAP levels and the global strip); the LDS walks run 1024 lanes with the whole dynamic LDS:
// every workgroup copies the scene, then serves its 1024 rays.  A lane beyond a.n takes part in the copy-in and the barrier and
// leaves; the stages hold no barrier and their one cross-lane operation (stage_node4's ballot) asks only the lanes that call it.

#include <hip/hip_runtime.h>
#include "path_common.h"
#include "film_ops.h"

#if !MPT_STRICT
#include "render_lane.h"
#include "render_lds_setup.h"

DEV bool walk_finite3(V3 a) { return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z); }

// Lane i's ray through WALK, and its answers.  w / stk: the walk as its render kernel set it up
template <class WALK>
DEV void walk_lane(const MptRenderParams &p, const MptQueryArgs &a, const WALK &w, typename WALK::Lifo &stk, int i) {
    const bool shadow = a.dis != nullptr;
    LaneState L;
    L.st = ST_DONE; L.hidx = -1; L.tbest = MPT_INF; L.hu = 0.0f; L.hv = 0.0f; L.navoid = 0; L.depth = 0; L.shadow = 0;
    const float *o = a.o + (size_t)i * 3, *d = a.d + (size_t)i * 3;
    const V3 ro = v3(o[0], o[1], o[2]), rd = v3(d[0], d[1], d[2]);
    // not a ray (query_kernel.hip query_ray): the lane answers "miss" without a step
    bool ray = walk_finite3(ro) && walk_finite3(rd) && any_ne0(rd);
    const V3 dir = normalized_unfused(rd);                                 // lane_begin_ray
    ray = ray && walk_finite3(dir);
    if (ray) {
        if (a.avoid) {                                                     // the id a node record holds for that triangle (render_shade.h)
            const int f = a.avoid[i];
            if (f >= 0 && f < p.n) { const int slot = a.slot_of[f]; L.navoid = WALK::ODD_IDS ? ((slot << 4) | 1) : ~slot; }
        }
        Cnt cnt = {};
        lane_start_ray<false, WALK>(L, stk, ro, dir, shadow ? fminf(a.dis[i], MPT_INF) : MPT_INF, shadow, cnt);
        if (p.n < 2) L.st = ST_DONE;                                       // lane_begin_ray: no root box to test (a shadow ray included: there is no node record)
        while (L.st == ST_NODE || L.st == ST_LEAF) {
            if (L.st == ST_NODE) {
                if constexpr (WALK::WIDE) stage_node4<false>(w, stk, L, cnt);
                else stage_node<false>(w, stk, L, cnt);
            } else stage_leaf<false>(w, stk, L, cnt);
        }
    }
    const bool was_hit = ray && L.hidx >= 0;
    if (shadow) {
        if (a.hit) a.hit[i] = was_hit ? 1 : 0;
        return;
    }
    const int hslot = WALK::ODD_IDS ? (L.hidx >> 4) : L.hidx;              // render_shade.h
    if (a.hit) a.hit[i] = was_hit ? 1 : 0;
    if (a.index) a.index[i] = was_hit ? a.leaf[hslot] : -1;
    if (a.depth) a.depth[i] = was_hit ? (WALK::T_SCALED ? L.tbest * p.t_unscale : L.tbest) : MPT_INF;
    if (a.u) a.u[i] = was_hit ? L.hu : 0.0f;
    if (a.v) a.v[i] = was_hit ? L.hv : 0.0f;
}

// ---------------------------------------------------------------- the gather walks: render_kernel_fast, render_kernel_wide
template <int STACK>
__global__ __launch_bounds__(MPT_BLOCK) void walk_kernel_gather(const MptRenderParams p, const MptQueryArgs a) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    const int i = (int)blockIdx.x * MPT_BLOCK + (int)threadIdx.x;
    if (i < a.n) walk_lane(p, a, tr.w, tr.st, i);
}

template <bool QUANT>
__global__ __launch_bounds__(MPT_BLOCK) void walk_kernel_wide(const MptRenderParams p, const MptQueryArgs a) {
    typedef GatherWalk4<QUANT> Walk;
    __shared__ int s_stack[Walk::CAP * MPT_BLOCK];
    typename Walk::Lifo stk;
    stk.stack = s_stack + threadIdx.x;
    stk.spill = p.stack_spill;                                             // the door's own strip: grid x 256 x Walk::SPILL entries at least
    stk.lane_off = (blockIdx.x * MPT_BLOCK + threadIdx.x) * (unsigned)Walk::SPILL;
    stk.sp = 0;
    Walk w; w.wnode = QUANT ? p.qnode : p.wnode; w.tgeo = p.tfast;
    const int i = (int)blockIdx.x * MPT_BLOCK + (int)threadIdx.x;
    if (i < a.n) walk_lane(p, a, w, stk, i);
}

// ---------------------------------------------------------------- the LDS walks: render_kernel_lds, render_kernel_lds4
__global__ __launch_bounds__(MPT_LDS_BLOCK) void walk_kernel_lds(const MptRenderParams p, const MptQueryArgs a) {
    extern __shared__ __attribute__((aligned(16))) MptVec4 smem[];
    const MptLdsRegions lay = mpt_lds_regions(p.n, p.default_mtl);
    lds_copy_nodes(p, smem);
    lds_copy_tris_mats<false>(p, smem, lay, p.default_mtl);
    __syncthreads();
    LdsWalk w;
    LdsWalk::Lifo stk;
    w.fnode = (LdsVec4Ptr)(void *)smem;
    lds_walk_regions(w, stk, smem, lay);
    w.mat_last = p.default_mtl; w.mat_default = p.default_mtl;
    const int i = (int)blockIdx.x * MPT_LDS_BLOCK + (int)threadIdx.x;
    if (i < a.n) walk_lane(p, a, w, stk, i);
}

__global__ __launch_bounds__(MPT_LDS_BLOCK) void walk_kernel_lds4(const MptRenderParams p, const MptQueryArgs a) {
    extern __shared__ __attribute__((aligned(16))) MptVec4 smem[];
    const MptLdsRegions lay = mpt_lds4_regions(p.n, p.nwide, p.lds_nmats);
    lds_copy_nodes4(p, smem);
    lds_copy_tris_mats<true>(p, smem, lay, p.lds_nmats);
    __syncthreads();
    if (!lds_starts_at_zero(smem)) {                                       // (render_kernel_lds4: the host turns the flag into an error)
        if (threadIdx.x == 0) __hip_atomic_store(p.watchdog, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    LdsWalk4 w;
    LdsWalk4::Lifo stk;
    lds_walk_regions(w, stk, smem, lay);
    w.mat_last = p.lds_nmats; w.mat_default = p.default_mtl;
    stk.ts = p.t_scale;
    const int i = (int)blockIdx.x * MPT_LDS_BLOCK + (int)threadIdx.x;
    if (i < a.n) walk_lane(p, a, w, stk, i);
}

// a.n rays, one lane each, through walk `walk` (include/miptina.h MPT_WALK_*); stack: the levels the binary gather walk's tree asks
// for; lds_bytes: the launch's dynamic LDS (the LDS walks).  a.n == 0 launches nothing
MPT_KERNEL_API hipError_t mpt_launch_walk_eval(const MptRenderParams *p, const MptQueryArgs *a, int walk, int stack, size_t lds_bytes,
                                               hipStream_t stream) {
    if (a->n <= 0) return hipSuccess;
    const unsigned grid = ((unsigned)a->n + MPT_BLOCK - 1) / MPT_BLOCK, grid_lds = ((unsigned)a->n + MPT_LDS_BLOCK - 1) / MPT_LDS_BLOCK;
    switch (walk) {
    case 0: return launch_by_stack<walk_kernel_gather<32>, walk_kernel_gather<64>>(stack, grid, stream, *p, *a);
    case 1: return launch_whole_lds<walk_kernel_lds>((int)grid_lds, MPT_LDS_BLOCK, lds_bytes, stream, *p, *a);
    case 2: hipLaunchKernelGGL(walk_kernel_wide<false>, dim3(grid), dim3(MPT_BLOCK), 0, stream, *p, *a); return hipGetLastError();
    case 3: hipLaunchKernelGGL(walk_kernel_wide<true>, dim3(grid), dim3(MPT_BLOCK), 0, stream, *p, *a); return hipGetLastError();
    case 4: return launch_whole_lds<walk_kernel_lds4>((int)grid_lds, MPT_LDS_BLOCK, lds_bytes, stream, *p, *a);
    }
    return hipErrorInvalidValue;
}
#endif

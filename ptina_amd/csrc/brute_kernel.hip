// brute_kernel.hip -- the brute-force engine (BruteEngine, engine/brute.py): "should be used for testing only".  The walk of
// path_trace with no light sampling and no MIS: a light is found only when a bounce ray hits it (brute_step, path_common.h).
//
// Built twice from this one source like render_kernel.hip and mlt_kernel.hip: MPT_STRICT=1 (StrictTracer, IEEE, the
// reference's traversal order) and MPT_STRICT=0 (the gather tracer over the production binary tree).
//
// Shape: the preview kernel's.  One workgroup per 16x16 tile of the context's share (tile_pixel: slabs and stripes are
// honoured), one lane per pixel, the lane's traversal stack in LDS.  The lane keeps its film element in registers over
// the frames of the batch and writes it once: no atomics, and the sum is in frame order whatever the split into launches,
// so films repeat bit for bit.  Deliberately NOT here: the persistent workgroups, the in-wave path regeneration and the
// LDS-resident scene of the PathEngine's production kernels -- this is a testing engine.

#include <hip/hip_runtime.h>
#include "path_common.h"

// BruteEngine._render, engine/brute.py:62-74, for the p.nframes frames of a batch
template <int STACK>
__global__ __launch_bounds__(MPT_BLOCK) void MPT_SUFFIX(brute_kernel)(const MptRenderParams p) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    int tile = xcd_remap(blockIdx.x, gridDim.x);
    int i, j;
    if (!tile_pixel(p, tile, &i, &j)) return;
    const int pix = i * p.ny + j;
    Cnt cnt = {};
    MptVec4 acc = p.film0[pix];
    PathState s;
    for (int f = 0; f < p.nframes; f++) {
        path_begin<false>(p, s, i, j, f, cnt);                               // get_rng + jitter + camera ray, brute.py:65-70
        while (!brute_step<false>(p, tr, s, cnt)) {}
        acc.x += s.result.x; acc.y += s.result.y; acc.z += s.result.z; acc.w += 1.0f;   // brute.py:73
    }
    p.film0[pix] = acc;
}

MPT_KERNEL_API hipError_t MPT_SUFFIX(mpt_launch_brute)(const MptRenderParams *p, int grid, int stack, hipStream_t stream) {
    return launch_by_stack<MPT_SUFFIX(brute_kernel)<32>, MPT_SUFFIX(brute_kernel)<64>>(stack, grid, stream, *p);
}

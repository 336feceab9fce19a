// adapt_kernel.hip -- adaptive sampling's list render kernel (PathEngine.render_selected, mpt_render_selected):
// the PathEngine's path (path_begin + path_step, path_common.h) for the pixels of a compacted list only.
//
// Built twice from this one source like render_kernel.hip, mlt_kernel.hip and brute_kernel.hip: MPT_STRICT=1 (StrictTracer, IEEE,
// the reference's traversal order) and MPT_STRICT=0 (the gather tracer over the production binary tree).
//
// Shape: sample lanes.  For a list of `count` pixels and the p.nframes frames of a launch, work item f * count + k traces frame
// f of list entry k and stores its radiance to samples[f * count + k] (16 bytes a lane, a wave's store 1 KiB contiguous): the grid
// is ceil(count * nframes / 256) workgroups, so a short list still fills the device, which one lane per pixel (brute_kernel.hip)
// would not.  Nothing here touches the film: adapt_select.hip's fold adds a pixel's samples in frame order, trace_pixel's order
// (render_kernel.hip), so films repeat bit for bit however a call's frames are split into launches, and in the strict build they
// are what the PathEngine adds to those pixels.  No atomics.  Deliberately NOT here: the persistent workgroups, the in-wave path
// regeneration and the LDS-resident scene of the PathEngine's production kernels -- list items inside trace_stream are a later step.

#include <hip/hip_runtime.h>
#include "path_common.h"

template <int STACK>
__global__ __launch_bounds__(MPT_BLOCK) void MPT_SUFFIX(adapt_render_kernel)(const MptRenderParams p, const int32_t *__restrict__ list, int count,
                                                                             MptVec4 *__restrict__ samples) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    const long long item = (long long)xcd_remap(blockIdx.x, gridDim.x) * MPT_BLOCK + threadIdx.x;
    if (item >= (long long)count * p.nframes) return;
    const int f = (int)(item / count), k = (int)(item - (long long)f * count);
    const int pix = list[k];
    const int i = pix / p.ny, j = pix - i * p.ny;
    Cnt cnt = {};
    PathState s;
    path_begin<false>(p, s, i, j, f, cnt);                                   // get_rng + jitter + camera ray, path.py:82-90
    while (!path_step<false>(p, tr, s, cnt)) {}
    samples[item] = { s.result.x, s.result.y, s.result.z, 1.0f };
}

// list: `count` film indices; samples: room for count * p->nframes records (the caller keeps that product below 2^31)
MPT_KERNEL_API hipError_t MPT_SUFFIX(mpt_launch_adapt_render)(const MptRenderParams *p, const int32_t *list, int count, MptVec4 *samples,
                                                              int stack, hipStream_t stream) {
    const long long items = (long long)count * p->nframes;
    if (items <= 0) return hipSuccess;
    if (items > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const unsigned grid = (unsigned)((items + MPT_BLOCK - 1) / MPT_BLOCK);
    return launch_by_stack<MPT_SUFFIX(adapt_render_kernel)<32>, MPT_SUFFIX(adapt_render_kernel)<64>>(stack, grid, stream, *p, list, count, samples);
}

// history_kernel.hip -- the two kernels of the film's reprojection that trace (mpt_history_keep, mpt_history_reproject;
// film_history.cpp): what each pixel's CENTRE ray sees.
//
//   G-buffer   the view as it is kept: per pixel the face the centre ray hits (-1: none), the object whose range of faces holds it
//              (0 where the model has no object table; -1 on a miss) and the hit's distance along the normalised ray.
//   motion     the same ray in the new view and scene, and where the surface point it hits lay in the kept view: the kept
//              positions of the hit face's corners at the hit's barycentrics, through the kept camera (history_rule.h
//              mpt_history_project), as a 20-byte record per pixel that the resample kernel (history.hip) reads.
//
// Built twice from this one source like brute_kernel.hip: MPT_STRICT=1 (StrictTracer over the reference LBVH, the reference's own
// depth, u and v) and MPT_STRICT=0 (the gather tracer over the binary fnode / tfast records; depth, u and v evaluated once more in
// f64, hit_point.h, as the batch queries do).
// Shape: the preview kernel's.  One workgroup per 16x16 tile of the context's share (tile_pixel: slabs and stripes are the film's),
// one lane per pixel, the lane's traversal stack in LDS through make_block_tracer.  The walks contain no barrier and no cross-lane
// operation, so a lane of the tile padding leaves at once.  No film pass, no sampler state and no counter is read or written.

#include <hip/hip_runtime.h>
#include "path_common.h"
#include "hit_point.h"
#include "history_rule.h"

// the centre ray of pixel (i, j) and its closest hit, with the depth and barycentrics a caller is handed
DEV Hit centre_hit(const MptRenderParams &p, const BlockTracer &tr, int i, int j) {
    const float x = m_div((float)i + 0.5f, (float)p.nx) * 2.0f - 1.0f;
    const float y = m_div((float)j + 0.5f, (float)p.ny) * 2.0f - 1.0f;
    V3 ro, rd;
    camera_generate(p, x, y, &ro, &rd);
    Cnt cnt = {};
    Hit h = tr.template closest<false>(ro, rd, -1, cnt);
#if !MPT_STRICT
    if (h.hit) hit_point_f64(p.tgeo + (size_t)h.index * 4, ro, rd, &h.depth, &h.u, &h.v);
#endif
    return h;
}

// the object of a face: the largest o with first[o] <= face, as query_closest_kernel; 0 where there is no table
DEV int object_of(const MptHistoryArgs &a, int face) {
    if (!a.first || a.nobj <= 0) return 0;
    int lo = 0, hi = a.nobj - 1;
    while (lo < hi) { const int m = (lo + hi + 1) >> 1; if (a.first[m] <= face) lo = m; else hi = m - 1; }
    return lo;
}

template <int STACK>
__global__ __launch_bounds__(MPT_BLOCK) void MPT_SUFFIX(history_gbuffer_kernel)(const MptRenderParams p, const MptHistoryArgs a) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    int i, j;
    if (!tile_pixel(p, tile, &i, &j)) return;
    const Hit h = centre_hit(p, tr, i, j);
    const size_t pix = (size_t)i * p.ny + j;
    const int face = h.hit ? a.leaf[h.index] : -1;
    a.face[pix] = face;
    a.id[pix] = h.hit ? object_of(a, face) : -1;
    a.depth[pix] = h.hit ? h.depth : MPT_INF;
}

template <int STACK>
__global__ __launch_bounds__(MPT_BLOCK) void MPT_SUFFIX(history_motion_kernel)(const MptRenderParams p, const MptHistoryArgs a) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    int i, j;
    if (!tile_pixel(p, tile, &i, &j)) return;
    const Hit h = centre_hit(p, tr, i, j);
    const float nan = __builtin_nanf("");
    MptMotion m = { -1, nan, nan, nan, MPT_MOTION_NONE };
    if (!h.hit) {
        if (a.same_camera) { m.fx = (float)i; m.fy = (float)j; m.d_exp = 0.0f; m.flags = MPT_MOTION_BACKGROUND; }
    } else {
        const int face = a.leaf[h.index];
        m.cur_id = object_of(a, face);
        const float *kept = a.kept_verts + (size_t)face * 9, *cur = a.cur_verts + (size_t)face * 24;
        float k[9];
        bool same = a.same_camera != 0;
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int d = 0; d < 3; d++) {
                k[c * 3 + d] = kept[c * 3 + d];
                same = same && __float_as_uint(k[c * 3 + d]) == __float_as_uint(cur[c * 8 + d]);
            }
        if (same) {
            m.fx = (float)i; m.fy = (float)j; m.d_exp = h.depth; m.flags = MPT_MOTION_STATIC;
        } else {
            float fx, fy, d_exp;
            if (mpt_history_project(k, k + 3, k + 6, h.u, h.v, a.kept_w2v, a.kept_v2w, p.nx, p.ny, &fx, &fy, &d_exp)) { m.fx = fx; m.fy = fy; m.d_exp = d_exp; }
        }
    }
    a.motion[(size_t)i * p.ny + j] = m;
}

// p->ntiles workgroups; a share without pixels launches nothing
MPT_KERNEL_API hipError_t MPT_SUFFIX(mpt_launch_history_gbuffer)(const MptRenderParams *p, const MptHistoryArgs *a, int stack, hipStream_t stream) {
    if (p->ntiles <= 0) return hipSuccess;
    return launch_by_stack<MPT_SUFFIX(history_gbuffer_kernel)<32>, MPT_SUFFIX(history_gbuffer_kernel)<64>>(stack, (unsigned)p->ntiles, stream, *p, *a);
}

MPT_KERNEL_API hipError_t MPT_SUFFIX(mpt_launch_history_motion)(const MptRenderParams *p, const MptHistoryArgs *a, int stack, hipStream_t stream) {
    if (p->ntiles <= 0) return hipSuccess;
    return launch_by_stack<MPT_SUFFIX(history_motion_kernel)<32>, MPT_SUFFIX(history_motion_kernel)<64>>(stack, (unsigned)p->ntiles, stream, *p, *a);
}

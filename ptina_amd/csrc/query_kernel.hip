// query_kernel.hip -- batch ray queries against the built tree (BVHTree.intersect / occluded, tree/lbvh.py; the reference's
// LinearBVH.intersect, lbvh.py:314-347, asked for many rays at once): the closest hit of each of n rays, or whether anything lies
// within a distance along it.  DESIGN.md section 3.15.
//
// Built twice from this one source like brute_kernel.hip: MPT_STRICT=1 (StrictTracer: snode, the reference LBVH in the reference's
// order, IEEE) and MPT_STRICT=0 (the gather tracer over the binary fnode / tfast records).  No tree, record format or option of its own.
//
// Shape: mlt_trace_kernel's.  One lane per ray, MPT_BLOCK lanes per workgroup, the lane's traversal stack in LDS at
// s_stack[level * MPT_BLOCK + threadIdx.x] like every kernel that walks through make_block_tracer.  The walks contain no barrier and no
// cross-lane operation (bvh_closest, bvh_walk, GatherWalk: pt_device.h), so lanes may leave before them: a lane beyond n, and a lane
// whose ray is no ray -- an origin or direction with a non-finite component, a direction that is exactly zero, or one whose
// normalisation is not finite (a squared length that overflows or underflows f32) -- which answers "miss" without a traversal step.
// The direction is normalised as path_step does (normalized()), so depths are world distances.
// The tracers name triangles by leaf slot; the caller's avoid and the answer's index are faces of the model (a.slot_of, a.leaf).
// In the production build depth, u and v of the winning triangle are evaluated once more, in f64 for the ray as given (hit_point_f64).
// Answers go out as plain per-lane stores to structure-of-arrays outputs; an output that is null is not written.

#include <hip/hip_runtime.h>
#include "path_common.h"
#include "hit_point.h"          // hit_point_f64: the production build's second evaluation of the winning triangle

DEV bool finite3(V3 a) { return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z); }

// ray i of the batch, normalised (and its direction as given); false: not a ray (the lane answers "miss").  The face to avoid
// comes back as a leaf slot
DEV bool query_ray(const MptRenderParams &p, const MptQueryArgs &a, int i, V3 *ro, V3 *rd, int *avoid, V3 *rd_given = nullptr) {
    const float *o = a.o + (size_t)i * 3, *d = a.d + (size_t)i * 3;
    const V3 ro_ = v3(o[0], o[1], o[2]), rd_ = v3(d[0], d[1], d[2]);
    *avoid = -1;
    if (!finite3(ro_) || !finite3(rd_) || !any_ne0(rd_)) return false;
    const V3 dir = normalized(rd_);
    if (!finite3(dir)) return false;
    if (a.avoid) {
        const int f = a.avoid[i];
        if (f >= 0 && f < p.n) *avoid = a.slot_of[f];
    }
    *ro = ro_; *rd = dir;
    if (rd_given) *rd_given = rd_;
    return true;
}

template <int STACK>
__global__ __launch_bounds__(MPT_BLOCK) void MPT_SUFFIX(query_closest_kernel)(const MptRenderParams p, const MptQueryArgs a) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    const int i = (int)blockIdx.x * MPT_BLOCK + (int)threadIdx.x;
    if (i >= a.n) return;
    Hit h; h.hit = 0; h.depth = MPT_INF; h.index = -1; h.u = 0.0f; h.v = 0.0f;
    V3 ro, rd, rd_given; int avoid;
    if (query_ray(p, a, i, &ro, &rd, &avoid, &rd_given)) {
        Cnt cnt = {};
        h = tr.template closest<false>(ro, rd, avoid, cnt);
#if !MPT_STRICT
        if (h.hit) hit_point_f64(p.tgeo + (size_t)h.index * 4, ro, rd_given, &h.depth, &h.u, &h.v);
#endif
    }
    int face = -1, object = -1;
    if (h.hit) {
        face = a.leaf[h.index];
        if (a.object && a.nobj > 0) {                                          // largest o with first[o] <= face, as compose_kernel
            int lo = 0, hi = a.nobj - 1;
            while (lo < hi) { const int m = (lo + hi + 1) >> 1; if (a.first[m] <= face) lo = m; else hi = m - 1; }
            object = lo;
        }
    } else {
        h.depth = MPT_INF; h.u = 0.0f; h.v = 0.0f;
    }
    if (a.hit) a.hit[i] = h.hit ? 1 : 0;
    if (a.depth) a.depth[i] = h.depth;
    if (a.index) a.index[i] = face;
    if (a.u) a.u[i] = h.u;
    if (a.v) a.v[i] = h.v;
    if (a.object) a.object[i] = object;
}

// the reference's shadow test, path.py:50-51: occluded iff there is a hit and it is not beyond dis
template <int STACK>
__global__ __launch_bounds__(MPT_BLOCK) void MPT_SUFFIX(query_occluded_kernel)(const MptRenderParams p, const MptQueryArgs a) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    const int i = (int)blockIdx.x * MPT_BLOCK + (int)threadIdx.x;
    if (i >= a.n) return;
    int occ = 0;
    V3 ro, rd; int avoid;
    if (query_ray(p, a, i, &ro, &rd, &avoid)) {
        // (no hit is farther than MPT_INF in either build: a larger dis, or one that is no number, asks the same question)
        const float dis = a.dis ? fminf(a.dis[i], MPT_INF) : MPT_INF;
        Cnt cnt = {};
        occ = tr.template occluded<false>(ro, rd, avoid, dis, cnt) ? 1 : 0;
    }
    a.occ[i] = occ;
}

// a.n rays, one lane each; a.n == 0 launches nothing
MPT_KERNEL_API hipError_t MPT_SUFFIX(mpt_launch_query_closest)(const MptRenderParams *p, const MptQueryArgs *a, int stack, hipStream_t stream) {
    if (a->n <= 0) return hipSuccess;
    const unsigned grid = ((unsigned)a->n + MPT_BLOCK - 1) / MPT_BLOCK;
    return launch_by_stack<MPT_SUFFIX(query_closest_kernel)<32>, MPT_SUFFIX(query_closest_kernel)<64>>(stack, grid, stream, *p, *a);
}

MPT_KERNEL_API hipError_t MPT_SUFFIX(mpt_launch_query_occluded)(const MptRenderParams *p, const MptQueryArgs *a, int stack, hipStream_t stream) {
    if (a->n <= 0) return hipSuccess;
    if (!a->occ) return hipErrorInvalidValue;
    const unsigned grid = ((unsigned)a->n + MPT_BLOCK - 1) / MPT_BLOCK;
    return launch_by_stack<MPT_SUFFIX(query_occluded_kernel)<32>, MPT_SUFFIX(query_occluded_kernel)<64>>(stack, grid, stream, *p, *a);
}

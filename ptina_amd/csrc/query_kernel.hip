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

#if !MPT_STRICT
// Which triangle is hit, the walk decides; how far and where on it, the production build's answer evaluates once more for that one
// triangle: Moller-Trumbore in f64 over the vertex and edges of its reference-order record and the caller's ray AS GIVEN, its
// direction not normalised (u and v do not depend on its length; depth = t |d|).  The f32 normalisation alone turns a ray by up to
// 6e-8 rad, which at a grazing angle onto a sliver moves the hit's u and v in the fourth digit whatever arithmetic follows
// (measured on the 300-triangle test scene: 5.6e-4 by the walk's own f32 values, 4.5e-4 by f64 behind the f32 normalisation, 1e-4
// by the reference's Face.intersect, which on a model far from the origin is itself 1.2e-3 off: DESIGN.md 3.15) -- harmless to a
// path, not to a caller who asked for the point.  One 64-byte read and some seventy f64 operations per ray that hits.  The strict
// build reports the reference's own f32 numbers.  (det = -n . d, which the walk's test found to be at least MPT_EPS |d| in size.)
DEV void hit_point_f64(const MptVec4 *g, V3 ro, V3 rd_given, float *depth, float *u, float *v) {
    const MptVec4 g0 = g[0], g1 = g[1], g2 = g[2];
    const double e1[3] = { g1.x, g1.y, g1.z }, e2[3] = { g2.x, g2.y, g2.z }, d[3] = { rd_given.x, rd_given.y, rd_given.z };
    const double s[3] = { (double)ro.x - g0.x, (double)ro.y - g0.y, (double)ro.z - g0.z };
    const double px = d[1] * e2[2] - d[2] * e2[1], py = d[2] * e2[0] - d[0] * e2[2], pz = d[0] * e2[1] - d[1] * e2[0];
    const double qx = s[1] * e1[2] - s[2] * e1[1], qy = s[2] * e1[0] - s[0] * e1[2], qz = s[0] * e1[1] - s[1] * e1[0];
    const double inv = 1.0 / (e1[0] * px + e1[1] * py + e1[2] * pz);
    *u = (float)((s[0] * px + s[1] * py + s[2] * pz) * inv);
    *v = (float)((d[0] * qx + d[1] * qy + d[2] * qz) * inv);
    *depth = (float)((e2[0] * qx + e2[1] * qy + e2[2] * qz) * inv * sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
}
#endif

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

// anim.hip -- keyframe animation on the device: the poses of the objects bound to a clip, evaluated at the
// scene's time by the rule of anim_rule.h and written where deform_kernel reads them (MptDeformObj::pose_at: ntargets morph weights,
// then njoints 3x4 matrices, f64).  Nothing but the time crosses to the device: skeletons (parents, depths, rest poses, inverse
// binds), tracks, key times and values lie in arenas (scene_anim.cpp).
//
// anim_kernel: ONE launch per mpt_compose covers every bound object whose pose must be evaluated, a workgroup of 256 lanes each:
//   1. the joints' rest T R S go to LDS (80 bytes a joint), the morph weights start at 0;
//   2. a lane per track samples it at the object's local time (mpt_anim_sample: a binary search over the key times, then STEP /
//      LINEAR / slerp / CUBICSPLINE) and overwrites its joint's T, R or S, or the weights.  At most one track per (target, path), so
//      no two lanes write the same words;
//   3. a lane per joint builds its local matrix in LDS (96 bytes a joint);
//   4. the hierarchy runs level by level over the depths the host computed when the skeleton was set: at level d the joints of depth
//      d become global[parent] . local, one barrier per level (a chain of 256 joints takes 255 of them; the kernel is latency-bound
//      and a launch of many objects hides them behind one another);
//   5. a lane per joint multiplies by its inverse bind and stores the palette; lanes store the weights.
// At 256 joints 44.5 KB of LDS.  Evaluated in f64, every sum in the rule's order without contraction (-ffp-contract=off, the
// Makefile's rule for this file).  Vector stores only, no atomics, no scratch.
// An object with a SECOND BINDING (MptAnimObj::blend, uniform in its workgroup) has clip B sampled beside
// clip A in step 2, at B's own local time, into the LDS of the matrices, which is idle until step 3 (20 KB of T R S and the weights
// fit its 24 KB); behind a barrier a lane per joint blends B into A's T R S and a lane per target the weights (anim_rule.h: the
// weight from the scene's time, lerp, nlerp over the shorter arc; weight 0 keeps A and weight 1 copies B, bit for bit), and behind
// another the kernel goes on with step 3.  An object without one runs the arithmetic it ran before there was a blend.
// motion_kernel moves whole objects by object clips; its comment stands in front of it.
// The f64 acos and sin of the slerp are the device library's: their error against the host's is what tests/anim_ref.py's bound
// allows for (ULP_TRIG_DEVICE there, measured through mpt_anim_trig below).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "mpt_types.h"
#include "anim_rule.h"

enum { AN_BLOCK = 256 };
static_assert(MPT_DEFORM_MAX_JOINTS <= AN_BLOCK, "a lane per joint");

__global__ __launch_bounds__(AN_BLOCK) void anim_kernel(const MptAnimObj *__restrict__ objs, double t, const int32_t *__restrict__ parents,
                                                        const int32_t *__restrict__ depths, const double *__restrict__ rest,
                                                        const double *__restrict__ inverse_bind, const MptAnimTrack *__restrict__ tracks,
                                                        const float *__restrict__ times, const float *__restrict__ values, double *pose) {
    __shared__ double s_trs[MPT_DEFORM_MAX_JOINTS * MPT_ANIM_REST];
    __shared__ double s_mat[MPT_DEFORM_MAX_JOINTS * 12];
    __shared__ double s_w[MPT_DEFORM_MAX_TARGETS];
    static_assert(MPT_DEFORM_MAX_JOINTS * MPT_ANIM_REST + MPT_DEFORM_MAX_TARGETS <= MPT_DEFORM_MAX_JOINTS * 12, "clip B's T R S and weights lie in s_mat");
    double *const b_trs = s_mat, *const b_w = s_mat + MPT_DEFORM_MAX_JOINTS * MPT_ANIM_REST;   // of a blended object, until its locals are built
    const MptAnimObj o = objs[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const double tau = mpt_anim_local_time(t, o.offset, o.speed, o.loop, o.t0, o.t1);
    for (int k = lane; k < o.njoints * MPT_ANIM_REST; k += AN_BLOCK) s_trs[k] = rest[(size_t)o.joint_at * MPT_ANIM_REST + k];
    if (lane < o.ntargets) s_w[lane] = 0.0;
    if (o.blend) {                                                   // (uniform in the workgroup, as every branch on o below)
        for (int k = lane; k < o.njoints * MPT_ANIM_REST; k += AN_BLOCK) b_trs[k] = rest[(size_t)o.joint_at * MPT_ANIM_REST + k];
        if (lane < o.ntargets) b_w[lane] = 0.0;
    }
    __syncthreads();
    for (int r = lane; r < o.ntracks; r += AN_BLOCK) {
        const MptAnimTrack tr = tracks[o.track_at + r];
        double *out = tr.path == MPT_ANIM_W ? s_w : s_trs + tr.target * MPT_ANIM_REST + (tr.path == MPT_ANIM_T ? 0 : tr.path == MPT_ANIM_R ? 3 : 7);
        mpt_anim_sample(tr, times, values, o.ntargets, tau, out);
    }
    if (o.blend) {
        const double tau_b = mpt_anim_local_time(t, o.offset_b, o.speed_b, o.loop_b, o.t0_b, o.t1_b);
        for (int r = lane; r < o.ntracks_b; r += AN_BLOCK) {
            const MptAnimTrack tr = tracks[o.track_b_at + r];
            double *out = tr.path == MPT_ANIM_W ? b_w : b_trs + tr.target * MPT_ANIM_REST + (tr.path == MPT_ANIM_T ? 0 : tr.path == MPT_ANIM_R ? 3 : 7);
            mpt_anim_sample(tr, times, values, o.ntargets, tau_b, out);
        }
        __syncthreads();
        const double w = mpt_anim_blend_weight(t, o.w0, o.w1, o.fade_start, o.fade_duration);
        if (w == 1.0) {                                              // b itself; at w == 0 a stays
            if (lane < o.njoints)
                for (int k = 0; k < MPT_ANIM_REST; k++) s_trs[lane * MPT_ANIM_REST + k] = b_trs[lane * MPT_ANIM_REST + k];
            if (lane < o.ntargets) s_w[lane] = b_w[lane];
        } else if (!(w == 0.0)) {
            if (lane < o.njoints) mpt_anim_blend_joint(s_trs + lane * MPT_ANIM_REST, b_trs + lane * MPT_ANIM_REST, w);
            if (lane < o.ntargets) mpt_anim_blend_values(s_w + lane, b_w + lane, w, 1);
        }
    }
    __syncthreads();
    int parent = -1, depth = 0;
    if (lane < o.njoints) {
        parent = parents[o.joint_at + lane]; depth = depths[o.joint_at + lane];
        mpt_anim_local(s_trs + lane * MPT_ANIM_REST, s_mat + lane * 12);
    }
    for (int d = 1; d <= o.levels; d++) {                            // (uniform: every lane meets every barrier)
        __syncthreads();
        if (lane < o.njoints && depth == d) mpt_anim_mul(s_mat + parent * 12, s_mat + lane * 12, s_mat + lane * 12);
    }
    double *out = pose + o.pose_at;
    if (lane < o.njoints) {                                          // (a joint's own matrix: written by this lane alone)
        double P[12];
        mpt_anim_mul(s_mat + lane * 12, inverse_bind + ((size_t)o.joint_at + (size_t)lane) * 12, P);
#pragma unroll
        for (int k = 0; k < 12; k++) out[o.ntargets + lane * 12 + k] = P[k];
    }
    if (lane < o.ntargets) out[lane] = s_w[lane];
}

// motion_kernel: a lane per object that an object clip moves.  The lane samples its clip's (at most three)
// tracks over the binding's rest T R S, which it keeps in LDS (80 bytes a lane: a track's values are written by index), builds the
// local matrix and world = base . local, and stores the sixteen doubles as eight 16-byte words and the epoch into the object's row of
// the object table, as scatter_place_kernel does for an instance.  Vector stores only, no atomics
__global__ __launch_bounds__(AN_BLOCK) void motion_kernel(const MptMotionObj *__restrict__ objs, int n, double t, const MptAnimTrack *__restrict__ tracks,
                                                          const float *__restrict__ times, const float *__restrict__ values, MptComposeObj *rows, int nrows,
                                                          unsigned epoch) {
    __shared__ double s_trs[AN_BLOCK * MPT_ANIM_REST];
    const int i = (int)(blockIdx.x * AN_BLOCK + threadIdx.x);
    if (i >= n) return;
    const MptMotionObj &o = objs[i];
    if ((unsigned)o.obj >= (unsigned)nrows) return;                  // (a guard of the stores below: the table is the host's own)
    double *trs = s_trs + (int)threadIdx.x * MPT_ANIM_REST;
#pragma unroll
    for (int k = 0; k < MPT_ANIM_REST; k++) trs[k] = o.rest[k];
    const double tau = mpt_anim_local_time(t, o.offset, o.speed, o.loop, o.t0, o.t1);
    double base[16], world[16];
#pragma unroll
    for (int k = 0; k < 16; k++) base[k] = o.base[k];
    mpt_anim_motion(o.ntracks < 3 ? o.ntracks : 3, tracks + o.track_at, times, values, tau, trs, base, world);
    MptComposeObj *row = rows + o.obj;
    double2 *dst = (double2 *)row->world;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = make_double2(world[2 * k], world[2 * k + 1]);
    row->epoch = epoch;
}

// the measurement door of the slerp's library functions: acos and sin of x [n] as the device evaluates them (mpt_anim_trig)
__global__ void anim_trig_kernel(const double *__restrict__ x, int n, double *__restrict__ acos_out, double *__restrict__ sin_out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    acos_out[i] = acos(x[i]);
    sin_out[i] = sin(x[i]);
}

// ---------------------------------------------------------------- launchers
// objs [nobj]: the bound objects to evaluate at scene time t, a workgroup each; the other pointers are the arenas
MPT_KERNEL_API hipError_t mpt_launch_anim(const MptAnimObj *objs, int nobj, double t, const int32_t *parents, const int32_t *depths, const double *rest,
                                          const double *inverse_bind, const MptAnimTrack *tracks, const float *times, const float *values, double *pose,
                                          hipStream_t stream) {
    if (nobj < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(anim_kernel, dim3((unsigned)nobj), dim3(AN_BLOCK), 0, stream, objs, t, parents, depths, rest, inverse_bind, tracks, times, values, pose);
    return hipGetLastError();
}

// objs [n]: the moved objects to evaluate at scene time t, a lane each; rows [nrows]: the object table
MPT_KERNEL_API hipError_t mpt_launch_motion(const MptMotionObj *objs, int n, double t, const MptAnimTrack *tracks, const float *times, const float *values,
                                            MptComposeObj *rows, int nrows, unsigned epoch, hipStream_t stream) {
    if (n < 1 || nrows < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_kernel, dim3((unsigned)((n + AN_BLOCK - 1) / AN_BLOCK)), dim3(AN_BLOCK), 0, stream, objs, n, t, tracks, times, values, rows, nrows, epoch);
    return hipGetLastError();
}

MPT_KERNEL_API hipError_t mpt_launch_anim_trig(const double *x, int n, double *acos_out, double *sin_out, hipStream_t stream) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(anim_trig_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, n, acos_out, sin_out);
    return hipGetLastError();
}

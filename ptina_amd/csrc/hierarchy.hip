// hierarchy.hip -- objects parented to objects and to joints on the device: the world matrices of the bound
// children that a compose evaluates, by the rule at the end of anim_rule.h, written into the object table behind motion_kernel and the
// table's upload and in front of the scatters and the composition.
//
// hierarchy_kernel: an ITEM is one bound child and takes one lane.  The lane
//   1. takes its local matrix from its record, or -- a child with a motion binding -- evaluates base . T R S with mpt_anim_motion, the
//      function motion_kernel calls, over the binding's rest T R S in LDS (80 bytes a lane: a track's values are written by index);
//   2. reads its parent's row of the object table;
//   3. if it follows a joint, reads the twelve doubles of the palette entry from the pose buffer, where anim_kernel or the host's
//      upload left them earlier in the stream;
//   4. forms world(parent) . local, or world(parent) . ([M; 0 0 0 1] . local);
//   5. stores the sixteen doubles as eight 16-byte words and the epoch into its own row, as motion_kernel does.
// The items of a launch are ordered by depth, and level l is the range [at[l], at[l + 1]) of them: a parent that this compose
// evaluates stands in an earlier level than its child, every other parent's row is already as it will be.  Two roads run this one
// kernel.  Up to MPT_HIER_ONE_GROUP items, ONE workgroup walks all the levels, lanes striding over a level's items, with a device-scope
// fence and a barrier between two levels: one launch.  Above, one launch per level, a lane per item, the stream ordering the levels.
// The table is read and written through one pointer that is neither const nor restrict, so that no load of a parent's row moves above
// the fence.  f64, every product in the rule's order without contraction (-ffp-contract=off, the Makefile's rule for this file).
// Vector stores only, no atomics, no scratch: 20 KB of LDS; the compiler's resource usage stands in DESIGN.md section 3.17.3.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "mpt_types.h"
#include "anim_rule.h"

enum { HI_BLOCK = 256 };

// one item: `trs` is the lane's ten doubles of LDS
static __device__ __forceinline__ void hier_item(const MptHierObj &o, double t, const MptAnimTrack *__restrict__ tracks, const float *__restrict__ times,
                                                 const float *__restrict__ values, const double *__restrict__ pose, int64_t npose, MptComposeObj *rows,
                                                 int nrows, unsigned epoch, double *trs) {
    // (a guard of the loads and stores below: the table and the pose buffer are the host's own; an item that fails it is skipped whole)
    if ((unsigned)o.obj >= (unsigned)nrows || (unsigned)o.parent >= (unsigned)nrows || (o.joint_at >= 0 && o.joint_at + 12 > npose)) return;
    double L[16], P[16], world[16];
    if (o.ntracks >= 0) {
#pragma unroll
        for (int k = 0; k < MPT_ANIM_REST; k++) trs[k] = o.rest[k];
        double base[16];
#pragma unroll
        for (int k = 0; k < 16; k++) base[k] = o.local[k];
        const double tau = mpt_anim_local_time(t, o.offset, o.speed, o.loop, o.t0, o.t1);
        mpt_anim_motion(o.ntracks < 3 ? o.ntracks : 3, tracks + o.track_at, times, values, tau, trs, base, L);
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) L[k] = o.local[k];
    }
    const double2 *src = (const double2 *)rows[o.parent].world;
#pragma unroll
    for (int k = 0; k < 8; k++) { const double2 v = src[k]; P[2 * k] = v.x; P[2 * k + 1] = v.y; }
    if (o.joint_at >= 0) {
        double M[12];
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] = pose[o.joint_at + k];
        mpt_hier_world(P, M, L, world);
    } else
        mpt_hier_world(P, nullptr, L, world);
    MptComposeObj *row = rows + o.obj;
    double2 *dst = (double2 *)row->world;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = make_double2(world[2 * k], world[2 * k + 1]);
    row->epoch = epoch;
}

__global__ __launch_bounds__(HI_BLOCK) void hierarchy_kernel(const MptHierObj *__restrict__ items, MptHierLevels lv, int nlevels, double t,
                                                             const MptAnimTrack *__restrict__ tracks, const float *__restrict__ times,
                                                             const float *__restrict__ values, const double *__restrict__ pose, int64_t npose,
                                                             MptComposeObj *rows, int nrows, unsigned epoch) {
    __shared__ double s_trs[HI_BLOCK * MPT_ANIM_REST];
    double *trs = s_trs + (int)threadIdx.x * MPT_ANIM_REST;
    const int stride = (int)gridDim.x * HI_BLOCK;
    for (int l = 0; l < nlevels; l++) {                              // (uniform: every lane meets every barrier; more than one level: one workgroup)
        if (l > 0) {
            __threadfence();
            __syncthreads();
        }
        const int end = lv.at[l + 1];
        for (int i = lv.at[l] + (int)(blockIdx.x * HI_BLOCK + threadIdx.x); i < end; i += stride)
            hier_item(items[i], t, tracks, times, values, pose, npose, rows, nrows, epoch, trs);
    }
}

// ---------------------------------------------------------------- launchers
// items [lv.at[nlevels]]: the bound children to evaluate at scene time t, ordered by depth; one workgroup walks the nlevels levels
MPT_KERNEL_API hipError_t mpt_launch_hierarchy_walk(const MptHierObj *items, const MptHierLevels *lv, int nlevels, double t, const MptAnimTrack *tracks,
                                                    const float *times, const float *values, const double *pose, int64_t npose, MptComposeObj *rows,
                                                    int nrows, unsigned epoch, hipStream_t stream) {
    if (nlevels < 1 || nlevels > MPT_HIER_MAX_DEPTH || nrows < 1 || lv->at[nlevels] - lv->at[0] > MPT_HIER_ONE_GROUP) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hierarchy_kernel, dim3(1), dim3(HI_BLOCK), 0, stream, items, *lv, nlevels, t, tracks, times, values, pose, npose, rows, nrows, epoch);
    return hipGetLastError();
}

// ... and one level alone, the items [begin, end), a lane each
MPT_KERNEL_API hipError_t mpt_launch_hierarchy_level(const MptHierObj *items, int begin, int end, double t, const MptAnimTrack *tracks, const float *times,
                                                     const float *values, const double *pose, int64_t npose, MptComposeObj *rows, int nrows, unsigned epoch,
                                                     hipStream_t stream) {
    if (begin < 0 || end <= begin || nrows < 1) return hipErrorInvalidValue;
    MptHierLevels lv{};
    lv.at[0] = begin; lv.at[1] = end;
    hipLaunchKernelGGL(hierarchy_kernel, dim3((unsigned)((end - begin + HI_BLOCK - 1) / HI_BLOCK)), dim3(HI_BLOCK), 0, stream, items, lv, 1, t, tracks, times,
                       values, pose, npose, rows, nrows, epoch);
    return hipGetLastError();
}

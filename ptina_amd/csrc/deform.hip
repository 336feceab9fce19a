// deform.hip -- mesh deformation on the device: glTF 2.0's morph targets and linear-blend skinning on the
// pool's face-corner records ([3k][8] f32: pos3 nrm3 uv2).  An object of a mesh that carries targets or a skin gets a DEFORMED
// COPY of the mesh in the pool, an ordinary object-space mesh record that compose_kernel then reads as it reads any mesh.
//
// Per corner, with the object's morph weights w_t (f64) and joint matrices J (3x4 f64, glTF's globalJoint . inverseBind):
//     q = p + w_0 dp_0 + w_1 dp_1 + ...          targets in index order; a target whose weight is exactly 0 is skipped
//     m = n + w_0 dn_0 + ...                     the same rule
//     with a skin (indices j0..j3, f32 weights a0..a3 as given, not renormalised; all four terms always taken):
//         M[r][c] = ((a0 J[j0][r][c] + a1 J[j1][r][c]) + a2 J[j2][r][c]) + a3 J[j3][r][c]
//         q'[r]   = ((M[r][0] q0 + M[r][1] q1) + M[r][2] q2) + M[r][3]
//         m'[r]   =  (M[r][0] m0 + M[r][1] m1) + M[r][2] m2
//     len = sqrt((m'0^2 + m'1^2) + m'2^2),  nrm = m' / len      (always, also without a skin)
//     uv copied
// The normal goes through M itself, not its inverse transpose: the rule compose_kernel applies to `world`, following the reference
// (multimesh.py:58-65); a zero normal gives NaN, as there.  Evaluated in f64, each sum left to right without contraction
// (-ffp-contract=off, the Makefile's rule for this file), rounded to f32 once, at the store.
//
// deform_kernel: ONE launch per mpt_compose covers every object whose pose changed.  A workgroup of 256 lanes takes one chunk of
// MPT_DEFORM_CHUNK = 1024 corners of one object, four per lane; the run table maps blocks to (object, chunk) -- run_table.h
// -- and since every object's runs start at a block of its own, a workgroup lies in exactly one object.  It stages that
// object's joint palette into LDS (96 bytes per joint: at 64 joints 6 bytes per corner, against 88 streamed): each lane gathers
// four joints per corner, which from global memory would be several times the stream on the divergent-gather path.  The morph
// weights are read through the scalar cache (their address depends on the block alone) and the skip of a zero weight is a uniform
// branch.  Base records travel as two 16-byte loads and two 16-byte stores, a target's deltas (24-byte records) as three 8-byte
// loads, the skin as one 8-byte and one 16-byte load.  Vector stores only, no atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "mpt_types.h"
#include "run_table.h"

enum { DF_BLOCK = 256, DF_PER_LANE = MPT_DEFORM_CHUNK / DF_BLOCK };
static_assert(DF_PER_LANE * DF_BLOCK == MPT_DEFORM_CHUNK, "a chunk is a whole number of corners per lane");

__global__ __launch_bounds__(DF_BLOCK) void deform_kernel(const float4 *pool_in, float4 *pool_out, const MptDeformObj *__restrict__ objs,
                                                          const MptRun *__restrict__ runs, int nruns, const float *__restrict__ deltas,
                                                          const uint16_t *__restrict__ joints, const float *__restrict__ weights,
                                                          const double *__restrict__ pose) {
    __shared__ double s_pal[MPT_DEFORM_MAX_JOINTS * 12];
    const int r = mpt_run_of(runs, nruns);
    const MptDeformObj o = objs[runs[r].item];
    const int chunk = (int)blockIdx.x - runs[r].block;
    const double *__restrict__ w = pose + o.pose_at;                          // [ntargets], then the palette [njoints][12]
    for (int k = (int)threadIdx.x; k < o.njoints * 12; k += DF_BLOCK) s_pal[k] = w[o.ntargets + k];
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < DF_PER_LANE; c++) {
        const int v = chunk * MPT_DEFORM_CHUNK + c * DF_BLOCK + (int)threadIdx.x;
        if (v >= o.nverts) break;
        const size_t src = ((size_t)o.src_vert + (size_t)v) * 2;
        const float4 q0 = pool_in[src], q1 = pool_in[src + 1];                // pos3 nrm.x | nrm.yz uv2
        double q[3] = { q0.x, q0.y, q0.z }, m[3] = { q0.w, q1.x, q1.y };
        for (int t = 0; t < o.ntargets; t++) {
            const double wt = w[t];
            if (wt == 0.0) continue;                                          // (uniform)
            const float2 *d = (const float2 *)(deltas + ((size_t)o.delta_at + ((size_t)t * (size_t)o.nverts + (size_t)v) * 6));
            const float2 d0 = d[0], d1 = d[1], d2 = d[2];                     // dp.xy | dp.z dn.x | dn.yz
            q[0] = q[0] + wt * d0.x; q[1] = q[1] + wt * d0.y; q[2] = q[2] + wt * d1.x;
            m[0] = m[0] + wt * d1.y; m[1] = m[1] + wt * d2.x; m[2] = m[2] + wt * d2.y;
        }
        if (o.njoints > 0) {
            const size_t s = (size_t)o.skin_at + (size_t)v;
            const ushort4 j = ((const ushort4 *)joints)[s];
            const float4 af = ((const float4 *)weights)[s];
            const double a0 = af.x, a1 = af.y, a2 = af.z, a3 = af.w;
            const double *J0 = s_pal + 12 * (int)j.x, *J1 = s_pal + 12 * (int)j.y, *J2 = s_pal + 12 * (int)j.z, *J3 = s_pal + 12 * (int)j.w;
            double qs[3], ms[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                double M[4];
#pragma unroll
                for (int k = 0; k < 4; k++) M[k] = ((a0 * J0[4 * r + k] + a1 * J1[4 * r + k]) + a2 * J2[4 * r + k]) + a3 * J3[4 * r + k];
                qs[r] = ((M[0] * q[0] + M[1] * q[1]) + M[2] * q[2]) + M[3];
                ms[r] = (M[0] * m[0] + M[1] * m[1]) + M[2] * m[2];
            }
#pragma unroll
            for (int r = 0; r < 3; r++) { q[r] = qs[r]; m[r] = ms[r]; }
        }
        const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
        const size_t dst = ((size_t)o.dst_vert + (size_t)v) * 2;
        pool_out[dst] = make_float4((float)q[0], (float)q[1], (float)q[2], (float)(m[0] / len));
        pool_out[dst + 1] = make_float4((float)(m[1] / len), (float)(m[2] / len), q1.z, q1.w);
    }
}

// ---------------------------------------------------------------- launcher
// pool: the mesh pool, read at the objects' src_vert and written at their dst_vert (ranges that never overlap); runs[nruns] and
// blocks: mpt_deform_plan's table over objs and the sum of its blocks
MPT_KERNEL_API hipError_t mpt_launch_deform(float *pool, const MptDeformObj *objs, const MptRun *runs, int nruns, int blocks,
                                            const float *deltas, const uint16_t *joints, const float *weights, const double *pose,
                                            hipStream_t stream) {
    if (nruns < 1 || blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(deform_kernel, dim3((unsigned)blocks), dim3(DF_BLOCK), 0, stream, (const float4 *)pool, (float4 *)pool, objs, runs, nruns,
                       deltas, joints, weights, pose);
    return hipGetLastError();
}

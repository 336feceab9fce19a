// compose.hip -- scene composition on the device: object-space meshes of a pool, placed by the world
// matrices of an object table, written as the world-space model the tree builders read ([3n][8] f32 records pos3 nrm3 uv2 and
// [n] material ids) -- the reference's compose_multiple_meshes (multimesh.py:58-65) without the trip through the host.
//
// compose_kernel, one lane per OUTPUT vertex v, 256 per workgroup: face v / 3 names the object o by a binary search over the
// objects' first faces (largest o with first[o] <= face: an object without faces is never found), the lane reads record
// v - 3 first_face of the object's mesh as two 16-byte loads, and writes
//     ph = (p, 1) . W^T,  pos = ph.xyz / ph.w          (a real divide: W need not be affine)
//     nh = (n, 0) . W^T,  nrm = nh.xyz / sqrt(nh.xyz . nh.xyz)    (W itself, not its inverse transpose; a zero normal gives NaN:
//                                                                  both as the reference)
//     uv copied
// evaluated in f64, each sum left to right without contraction (-ffp-contract=off, the Makefile's rule for this file), rounded to f32
// once, at the store: two 16-byte stores.  The lane of a face's first vertex writes the face's material id.
// A partial launch (all = 0) covers the runs of workgroups that overlap the changed objects' output; a lane whose object does not
// carry the launch's epoch writes nothing and reads the position that is there.
// Bounds: every workgroup leaves the min / max of its 256 positions (fminf / fmaxf: exact and order-free, NaN ignored) in
// part[wg][6]; compose_fold_kernel, ONE workgroup of 1024 lanes, folds all partials -- also those of workgroups this launch did not run, whose
// output has not changed -- into the host's mapped record.  No atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "mpt_types.h"
#include "run_table.h"
#include "compose_rule.h"

enum { CP_BLOCK = 256, CP_WAVE = 64, CP_WAVES = CP_BLOCK / CP_WAVE, CP_FOLD = 1024, CP_FOLD_WAVES = CP_FOLD / CP_WAVE };

// lanes' values -> the workgroup's, in lane 0 of wave 0: s_part[waves][6]
__device__ static void block_minmax(float lo[3], float hi[3], float (*s_part)[6], int waves) {
#pragma unroll
    for (int d = CP_WAVE / 2; d > 0; d >>= 1)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], d, CP_WAVE));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d, CP_WAVE));
        }
    const int wave = (int)threadIdx.x / CP_WAVE;
    if (((int)threadIdx.x & (CP_WAVE - 1)) == 0)
        for (int k = 0; k < 3; k++) { s_part[wave][k] = lo[k]; s_part[wave][3 + k] = hi[k]; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < waves; w++)
            for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], s_part[w][k]); hi[k] = fmaxf(hi[k], s_part[w][3 + k]); }
}

// one output vertex of object o: written when the object carries the launch's epoch (or all), else read back; returns pos3 nrm.x
__device__ static inline float4 compose_vertex(const float4 *__restrict__ pool, const MptComposeObj *__restrict__ o, int v, int face, int all,
                                               unsigned epoch, float4 *__restrict__ out, int *__restrict__ mtlids) {
    if (!all && o->epoch != epoch) return out[(size_t)v * 2];
    const size_t src = ((size_t)o->mesh_vert + (size_t)(v - 3 * o->first_face)) * 2;
    const float4 q0 = pool[src], q1 = pool[src + 1];                          // pos3 nrm.x | nrm.yz uv2
    const double p[3] = { q0.x, q0.y, q0.z }, n[3] = { q0.w, q1.x, q1.y };
    double ph[4], nh[3];
#pragma unroll
    for (int j = 0; j < 4; j++) ph[j] = mpt_place_row(p, o->world, j);        // (compose_rule.h: scatter.hip places the corners of a surface by it too)
#pragma unroll
    for (int j = 0; j < 3; j++) nh[j] = (n[0] * o->world[4 * j] + n[1] * o->world[4 * j + 1]) + n[2] * o->world[4 * j + 2];
    const double len = sqrt((nh[0] * nh[0] + nh[1] * nh[1]) + nh[2] * nh[2]);
    const float4 r0 = make_float4((float)(ph[0] / ph[3]), (float)(ph[1] / ph[3]), (float)(ph[2] / ph[3]), (float)(nh[0] / len));
    out[(size_t)v * 2] = r0;
    out[(size_t)v * 2 + 1] = make_float4((float)(nh[1] / len), (float)(nh[2] / len), q1.z, q1.w);
    if (v == 3 * face) mtlids[face] = o->mtlid;
    return r0;
}

__global__ __launch_bounds__(CP_BLOCK) void compose_kernel(const float4 *__restrict__ pool, const MptComposeObj *__restrict__ objs,
                                                           const int *__restrict__ first, int nobj, int nverts,
                                                           const MptRun *__restrict__ runs, int nruns, int all, unsigned epoch,
                                                           float4 *__restrict__ out, int *__restrict__ mtlids, float *__restrict__ part) {
    __shared__ float s_part[CP_WAVES][6];
    int wg = (int)blockIdx.x;
    if (!all) {
        const int r = mpt_run_of(runs, nruns);
        wg = runs[r].item + ((int)blockIdx.x - runs[r].block);
    }
    const int v = wg * CP_BLOCK + (int)threadIdx.x;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    if (v < nverts) {
        const int face = v / 3;
        int a = 0, b = nobj - 1;
        while (a < b) { const int m = (a + b + 1) >> 1; if (first[m] <= face) a = m; else b = m - 1; }
        // most waves lie inside one object: its record is then read once for the wave, through the scalar cache, instead of by
        // every lane (the same operations on the same numbers either way)
        const int a0 = __builtin_amdgcn_readfirstlane(a);
        const float4 r0 = __all(a == a0) ? compose_vertex(pool, objs + a0, v, face, all, epoch, out, mtlids)
                                         : compose_vertex(pool, objs + a, v, face, all, epoch, out, mtlids);
        lo[0] = hi[0] = r0.x; lo[1] = hi[1] = r0.y; lo[2] = hi[2] = r0.z;     // (a NaN is dropped by the first fminf / fmaxf it meets)
    }
    block_minmax(lo, hi, s_part, CP_WAVES);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; k++) { part[(size_t)wg * 6 + k] = lo[k]; part[(size_t)wg * 6 + 3 + k] = hi[k]; }
}

__global__ __launch_bounds__(CP_FOLD) void compose_fold_kernel(const float *__restrict__ part, int nwg, float *__restrict__ bounds_host) {
    __shared__ float s_part[CP_FOLD_WAVES][6];
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int w = (int)threadIdx.x; w < nwg; w += CP_FOLD) {
        const float2 *q = (const float2 *)(part + (size_t)w * 6);             // (24-byte records: 8-byte words)
        const float2 a = q[0], b = q[1], c = q[2];
        lo[0] = fminf(lo[0], a.x); lo[1] = fminf(lo[1], a.y); lo[2] = fminf(lo[2], b.x);
        hi[0] = fmaxf(hi[0], b.y); hi[1] = fmaxf(hi[1], c.x); hi[2] = fmaxf(hi[2], c.y);
    }
    block_minmax(lo, hi, s_part, CP_FOLD_WAVES);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; k++) { bounds_host[k] = lo[k]; bounds_host[3 + k] = hi[k]; }
}

// ---------------------------------------------------------------- launchers
MPT_KERNEL_API size_t mpt_compose_groups(size_t nverts) { return (nverts + CP_BLOCK - 1) / CP_BLOCK; }

// blocks: workgroups to launch -- with all = 1 every one of the output, mpt_compose_groups(nverts), else the sum of the runs (runs[nruns]
// holds their first output workgroup and first block); part: 6 floats per output workgroup; bounds_host: the device alias of the
// host's mapped {min3, max3}
MPT_KERNEL_API hipError_t mpt_launch_compose(const float *pool, const MptComposeObj *objs, const int *first, int nobj, int nverts,
                                             const MptRun *runs, int nruns, int blocks, int all, unsigned epoch, float *out,
                                             int *mtlids, float *part, float *bounds_host, hipStream_t stream) {
    if (nobj < 1 || nverts < 1 || (!all && blocks > 0 && nruns < 1)) return hipErrorInvalidValue;
    if (blocks > 0)
        hipLaunchKernelGGL(compose_kernel, dim3((unsigned)blocks), dim3(CP_BLOCK), 0, stream, (const float4 *)pool, objs, first, nobj, nverts, runs,
                           nruns, all, epoch, (float4 *)out, mtlids, part);
    hipLaunchKernelGGL(compose_fold_kernel, dim3(1), dim3(CP_FOLD), 0, stream, (const float *)part, (int)mpt_compose_groups((size_t)nverts), bounds_host);
    return hipGetLastError();
}

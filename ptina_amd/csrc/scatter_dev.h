// scatter_dev.h -- what the kernels of scatter.hip and scatter_space.hip share on the device: the shape of their workgroups, the
// world corners of a face of the surface, the blocks of a run and the workgroup's exclusive scan.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mpt_types.h"
#include "run_table.h"
#include "scatter_rule.h"

enum { SC_BLOCK = MPT_SCATTER_CHUNK, SC_WAVE = 64, SC_WAVES = SC_BLOCK / SC_WAVE };

// the world corners of face g of the surface `S`: records 3 g .. 3 g + 2 of its copy in the pool; uv (may be null): their texcoords
static __device__ __forceinline__ void sc_corners(const float4 *__restrict__ pool, const MptComposeObj &S, int g, double P[3][3], float uv[3][2]) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const size_t src = ((size_t)S.mesh_vert + (size_t)g * 3 + (size_t)c) * 2;
        const float4 q0 = pool[src];
        const float rec[3] = { q0.x, q0.y, q0.z };
        mpt_scatter_corner(rec, S.world, P[c]);
        if (uv) { const float4 q1 = pool[src + 1]; uv[c][0] = q1.z; uv[c][1] = q1.w; }
    }
}

// the blocks [b0, b1) of run r of a launch of `blocks` blocks
static __device__ __forceinline__ void sc_run_blocks(const MptRun *__restrict__ runs, int nruns, int blocks, int r, int *b0, int *b1) {
    *b0 = runs[r].block;
    *b1 = r + 1 < nruns ? runs[r + 1].block : blocks;
}

// the exclusive scan of the workgroup's values; *total (every lane): their sum
static __device__ __forceinline__ uint64_t sc_block_scan(uint64_t x, uint64_t *s_sum, uint64_t *total) {
    const int lane = (int)threadIdx.x & (SC_WAVE - 1), wave = (int)threadIdx.x / SC_WAVE;
    uint64_t inc = x;
#pragma unroll
    for (int d = 1; d < SC_WAVE; d <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)inc, d, SC_WAVE);
        if (lane >= d) inc += up;
    }
    if (lane == SC_WAVE - 1) s_sum[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < SC_WAVES; k++) { if (k < wave) before += s_sum[k]; all += s_sum[k]; }
    __syncthreads();                           // (s_sum is written again by the caller's next round)
    *total = all;
    return before + inc - x;
}

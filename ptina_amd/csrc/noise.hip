// noise.hip -- how noisy film pass 0 still is, estimated on the device from the film F and the mark M, a copy of F taken earlier
// (mpt_film_mark / mpt_get_noise; the definition is in include/miptina.h; the numpy restatement
// tests/noise_ref.py).  The samples of a pixel fall into two groups -- the nA = M.w the mark holds and the nB = F.w - M.w added
// since -- and the distance between the groups' means, scaled to the standard error of the mean of all of them and taken relative
// to the brightness, is the estimate e.  With equal halves (k = 1) this is Cycles' adaptive-sampling criterion as written (its
// error is (|I.r-A.r| + |I.g-A.g| + |I.b-A.b|) / (3 n) over 1e-4 + sqrt((I.r+I.g+I.b) / (3 n)), I the sum of all n samples and A
// twice the sum of one half of them: |I - A| / n = |a - b| / 2 = |m - a|), so the thresholds are the "noise threshold" a Blender
// user knows.  The reference has nothing of the kind: its scripts pick a sample count by hand.
//
//   one pass    noise_estimate_kernel: workgroup b takes the film elements [1024 b, 1024 (b + 1)), lane t the elements
//               1024 b + t + 256 k, k = 0 .. 3 ascending: two 16-byte loads (F, M) per element, a wave's loads 1 KiB contiguous;
//               it writes e to the map (4 bytes a lane, 256 contiguous bytes a wave; optional) and, in re-mark mode, F over M
//               (16 bytes a lane) -- 32 B read and 0, 4, 16 or 20 B written per pixel, nothing read twice.  The lanes'
//               statistics fold to the workgroup's partial.
//   the fold    ONE workgroup of noise_fold_kernel folds the partials, and lane 0 writes the statistics to the host's mapped record.
// Both stages are film_fold.h's, which says why count, max and sum repeat bit for bit.
//
// Arithmetic: f32 without contraction (-ffp-contract=off, the Makefile's rule for this file), with IEEE-rounded division and
// square root and denormals kept -- hipcc's defaults for HIP code, which this file relies on and does not override: every
// operation of e is one correctly rounded f32 operation, so the map and the maximum equal the numpy restatement bit for bit.  The
// sum of the f32 values e is taken in f64.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/miptina.h"
#include "mpt_types.h"
#include "film_ops.h"
#include "film_fold.h"
#include "noise_pixel.h"            // nz_pixel: e of one pixel, shared with adapt_select.hip

enum { NZ_BLOCK = 256, NZ_PER_LANE = 4, NZ_RUN = NZ_BLOCK * NZ_PER_LANE };   // 1024 consecutive film elements per workgroup
static_assert(NZ_BLOCK == FILM_FOLD_BLOCK, "the fold is written for this block");

// the statistics as they are summed; a partial (mpt_launch_noise's `part`) is one of these in the room of an mpt_noise_stats
struct NzAcc {
    double sum; long long valid, above; float max;
    static __device__ __forceinline__ NzAcc zero() { return { 0.0, 0, 0, 0.0f }; }
    __device__ __forceinline__ void add(const NzAcc &o) { sum += o.sum; valid += o.valid; above += o.above; max = fmaxf(max, o.max); }
    __device__ __forceinline__ NzAcc across(int h) const {
        return { film_lane_xor(sum, h), film_lane_xor(valid, h), film_lane_xor(above, h), film_lane_xor(max, h) };
    }
};
static_assert(sizeof(NzAcc) == sizeof(mpt_noise_stats), "a partial is one 32-byte record");

// map: [npix] or NULL; remark: mark := film in the same pass; part: one record per workgroup
__global__ __launch_bounds__(NZ_BLOCK) void noise_estimate_kernel(const float4 *__restrict__ film, float4 *__restrict__ mark, size_t npix,
                                                                  float threshold, int remark, float *__restrict__ map,
                                                                  NzAcc *__restrict__ part) {
    __shared__ NzAcc s_wave[FILM_FOLD_WAVES];
    const size_t base = (size_t)blockIdx.x * NZ_RUN + threadIdx.x;
    float4 F[NZ_PER_LANE], M[NZ_PER_LANE];
#pragma unroll
    for (int k = 0; k < NZ_PER_LANE; k++) {          // every load of the lane in flight before the first is used
        const size_t p = base + (size_t)k * NZ_BLOCK;
        F[k] = M[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (p < npix) { F[k] = film[p]; M[k] = mark[p]; }
    }
    NzAcc acc = NzAcc::zero();
#pragma unroll
    for (int k = 0; k < NZ_PER_LANE; k++) {
        const size_t p = base + (size_t)k * NZ_BLOCK;
        if (p < npix) {
            float e;
            if (nz_pixel(F[k], M[k], &e)) {
                acc.sum += (double)e;
                acc.valid += 1;
                acc.above += e > threshold ? 1 : 0;
                acc.max = fmaxf(acc.max, e);
            }
            if (map) map[p] = e;
            if (remark) mark[p] = F[k];
        }
    }
    const NzAcc tot = film_block_fold(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(NZ_BLOCK) void noise_fold_kernel(const NzAcc *__restrict__ part, int nparts, float threshold,
                                                              mpt_noise_stats *__restrict__ stats_host) {
    __shared__ NzAcc s_wave[FILM_FOLD_WAVES];
    const NzAcc tot = film_fold_parts(part, nparts, s_wave);
    if (threadIdx.x == 0) {
        stats_host->valid = tot.valid; stats_host->above = tot.above; stats_host->sum = tot.sum; stats_host->max = tot.max;
        stats_host->threshold = threshold;
    }
}

// ---------------------------------------------------------------- launchers
// (film_fold_count(npix, NZ_RUN), spelled out: tests/test_noise_cpu.py holds the restatement's sizing to this line)
MPT_KERNEL_API size_t mpt_noise_parts(size_t npix) { return (npix + NZ_RUN - 1) / NZ_RUN; }

// part: mpt_noise_parts(npix) records (at least one); stats_host: the device alias of the host's mapped record
MPT_KERNEL_API hipError_t mpt_launch_noise(const MptVec4 *film, MptVec4 *mark, size_t npix, float threshold, int remark, float *map,
                                           mpt_noise_stats *part, mpt_noise_stats *stats_host, hipStream_t stream) {
    unsigned nparts;
    if (const hipError_t e = film_fold_grid(npix, NZ_RUN, &nparts)) return e;
    if (nparts) hipLaunchKernelGGL(noise_estimate_kernel, dim3(nparts), dim3(NZ_BLOCK), 0, stream, (const float4 *)film, (float4 *)mark,
                                   npix, threshold, remark, map, (NzAcc *)part);
    hipLaunchKernelGGL(noise_fold_kernel, dim3(1), dim3(NZ_BLOCK), 0, stream, (const NzAcc *)part, (int)nparts, threshold, stats_host);
    return hipGetLastError();
}

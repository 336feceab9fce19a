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
//               statistics fold in the wave by a fixed butterfly (lane l takes lane l ^ h, h = 32, 16, ..., 1), the four waves'
//               in LDS in ascending order, and the workgroup leaves one mpt_noise_stats.
//   the fold    ONE workgroup of noise_fold_kernel: lane t takes the partials t, t + 256, ... ascending, the same butterfly, the
//               same four-wave fold, and lane 0 writes the statistics to the host's mapped record.
// The shape of the sum is a function of the number of pixels alone -- not of how many CUs the launch got -- and there is no atomic:
// count, max and sum repeat bit for bit.
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

static_assert(sizeof(MptVec4) == sizeof(float4), "the film's records are read as float4");
static_assert(sizeof(mpt_noise_stats) == 32, "a partial is one 32-byte record");

enum { NZ_BLOCK = 256, NZ_PER_LANE = 4, NZ_RUN = NZ_BLOCK * NZ_PER_LANE };   // 1024 consecutive film elements per workgroup
enum { NZ_WAVE = 64, NZ_WAVES = NZ_BLOCK / NZ_WAVE };

// display.hip's rule: fminf(fmaxf(c, 0), 3e38): NaN -> 0 (fmaxf returns its other argument), negative -> 0, +inf -> 3e38
__device__ __forceinline__ float nz_clamp0(float c) { return fminf(fmaxf(c, 0.0f), 3.0e38f); }

// e of one pixel; false (and e = 0) where the pixel is not valid
__device__ __forceinline__ bool nz_pixel(const float4 F, const float4 M, float *e) {
    const float nA = M.w, n = F.w, nB = n - nA;
    *e = 0.0f;
    if (!(nA > 0.0f && nB > 0.0f)) return false;
    const float a[3] = { nz_clamp0(M.x / nA), nz_clamp0(M.y / nA), nz_clamp0(M.z / nA) };
    const float m[3] = { nz_clamp0(F.x / n), nz_clamp0(F.y / n), nz_clamp0(F.z / n) };
    const float k = sqrtf(nA / nB);
    const float d[3] = { fabsf(m[0] - a[0]) * k, fabsf(m[1] - a[1]) * k, fabsf(m[2] - a[2]) * k };
    const float num = ((d[0] + d[1]) + d[2]) / 3.0f;
    const float den = 1e-4f + sqrtf(((m[0] + m[1]) + m[2]) / 3.0f);
    *e = nz_clamp0(num / den);          // (the clamp moves only a value that is not finite: saturated channels overflow the sums)
    return true;
}

struct NzAcc { double sum; long long valid, above; float max; };

__device__ __forceinline__ NzAcc nz_add(NzAcc a, const NzAcc b) {
    a.sum += b.sum; a.valid += b.valid; a.above += b.above; a.max = fmaxf(a.max, b.max);
    return a;
}

// the 256 lanes' accumulators: a butterfly within each wave (every lane ends with the wave's total; a + b is b + a bit for bit),
// then the waves' totals through LDS, added in ascending order by every lane
__device__ __forceinline__ NzAcc nz_fold(NzAcc v, NzAcc *s_wave) {
#pragma unroll
    for (int h = NZ_WAVE / 2; h > 0; h >>= 1) {
        NzAcc o;
        o.sum = __shfl_xor(v.sum, h, NZ_WAVE);
        o.valid = __shfl_xor(v.valid, h, NZ_WAVE);
        o.above = __shfl_xor(v.above, h, NZ_WAVE);
        o.max = __shfl_xor(v.max, h, NZ_WAVE);
        v = nz_add(v, o);
    }
    if ((threadIdx.x & (NZ_WAVE - 1)) == 0) s_wave[threadIdx.x / NZ_WAVE] = v;
    __syncthreads();
    NzAcc tot = s_wave[0];
#pragma unroll
    for (int w = 1; w < NZ_WAVES; w++) tot = nz_add(tot, s_wave[w]);
    return tot;
}

__device__ __forceinline__ void nz_store(mpt_noise_stats *out, const NzAcc tot, float threshold) {
    out->valid = tot.valid; out->above = tot.above; out->sum = tot.sum; out->max = tot.max; out->threshold = threshold;
}

// map: [npix] or NULL; remark: mark := film in the same pass; part: one record per workgroup
__global__ __launch_bounds__(NZ_BLOCK) void noise_estimate_kernel(const float4 *__restrict__ film, float4 *__restrict__ mark, size_t npix,
                                                                  float threshold, int remark, float *__restrict__ map,
                                                                  mpt_noise_stats *__restrict__ part) {
    __shared__ NzAcc s_wave[NZ_WAVES];
    const size_t base = (size_t)blockIdx.x * NZ_RUN + threadIdx.x;
    float4 F[NZ_PER_LANE], M[NZ_PER_LANE];
#pragma unroll
    for (int k = 0; k < NZ_PER_LANE; k++) {          // every load of the lane in flight before the first is used
        const size_t p = base + (size_t)k * NZ_BLOCK;
        F[k] = M[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (p < npix) { F[k] = film[p]; M[k] = mark[p]; }
    }
    NzAcc acc = { 0.0, 0, 0, 0.0f };
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
    const NzAcc tot = nz_fold(acc, s_wave);
    if (threadIdx.x == 0) nz_store(&part[blockIdx.x], tot, threshold);
}

__global__ __launch_bounds__(NZ_BLOCK) void noise_fold_kernel(const mpt_noise_stats *__restrict__ part, int nparts, float threshold,
                                                              mpt_noise_stats *__restrict__ stats_host) {
    __shared__ NzAcc s_wave[NZ_WAVES];
    NzAcc acc = { 0.0, 0, 0, 0.0f };
    for (int q = (int)threadIdx.x; q < nparts; q += NZ_BLOCK) {
        const mpt_noise_stats s = part[q];
        acc = nz_add(acc, NzAcc{ s.sum, (long long)s.valid, (long long)s.above, s.max });
    }
    const NzAcc tot = nz_fold(acc, s_wave);
    if (threadIdx.x == 0) nz_store(stats_host, tot, threshold);
}

// ---------------------------------------------------------------- launchers
MPT_KERNEL_API size_t mpt_noise_parts(size_t npix) { return (npix + NZ_RUN - 1) / NZ_RUN; }

// part: mpt_noise_parts(npix) records (at least one); stats_host: the device alias of the host's mapped record
MPT_KERNEL_API hipError_t mpt_launch_noise(const MptVec4 *film, MptVec4 *mark, size_t npix, float threshold, int remark, float *map,
                                           mpt_noise_stats *part, mpt_noise_stats *stats_host, hipStream_t stream) {
    const size_t nparts = mpt_noise_parts(npix);
    if (nparts > 0x7fffffffULL) return hipErrorInvalidConfiguration;
    if (nparts) hipLaunchKernelGGL(noise_estimate_kernel, dim3((unsigned)nparts), dim3(NZ_BLOCK), 0, stream, (const float4 *)film,
                                   (float4 *)mark, npix, threshold, remark, map, part);
    hipLaunchKernelGGL(noise_fold_kernel, dim3(1), dim3(NZ_BLOCK), 0, stream, (const mpt_noise_stats *)part, (int)nparts, threshold, stats_host);
    return hipGetLastError();
}

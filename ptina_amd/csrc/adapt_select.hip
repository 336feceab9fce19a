// adapt_select.hip -- adaptive sampling's two build-independent halves (the numpy restatement
// tests/adaptive_ref.py): which pixels of film pass 0 still need samples, as a compacted list, and the fold of the samples the
// list render kernel (adapt_kernel.hip) left for them into the film.
//
// Selection.  With e and `valid` of noise_pixel.h (the estimate mpt_get_noise reports), a pixel is ABOVE when it is valid and
// e > threshold, and ACTIVE when it is valid and either above or, with dilate = 1, one of its up to eight neighbours inside the
// film is above (Cycles' filter does the same: a converged pixel beside a noisy one keeps sampling).  A pixel that is not valid --
// no samples on one side of the mark, which covers every column a slab or stripe split did not render -- is never active.
//   1 flags    adapt_select_kernel: ONE workgroup per 16x16 tile of the whole film, tile b = ti * tiles_y + tj (ti along x), lane
//              t the pixel (16 ti + (t >> 4), 16 tj + (t & 15)): a wave's 64 lanes are four runs of 16 consecutive film elements.
//              The 18x18 states of the tile and its one-pixel halo (not valid or outside | valid | valid and above) are computed
//              from film and mark into LDS (without dilate the halo is not read); each wave's ballot of its active lanes goes
//              to ballot[4 b + wave] and the tile's count to count[b].
//   2 scan     adapt_scan_kernel, ONE workgroup: count[] becomes its exclusive prefix sum, in place, and the total goes to the
//              host's mapped record (beside the statistics: no copy).
//   3 scatter  adapt_scatter_kernel, the grid of 1: a set lane writes its film index i * ny + j to
//              list[offset of its tile + bits set in the earlier waves' ballots + bits set below its own in its wave's].
// No atomics; the list's order -- tile-major, lane order within the tile -- is a function of the film alone, and neighbouring
// entries are neighbouring pixels.  The statistics of a selection are mpt_launch_noise's own (noise.hip), launched beside these on
// the same film and mark: a sum in f64 is not associative, so only noise.hip's shape of the sum gives noise.hip's bits.
//
// Fold.  adapt_fold_kernel, lane k: acc = film[list[k]]; with remark, mark[list[k]] = acc; then acc += (samples[f * count + k], 1)
// for f ascending -- trace_pixel's order of additions (render_kernel.hip), so the film does not depend on how a call's frames were
// split into launches.  Every listed pixel has one lane (the list is strictly ascending or a selection's: no duplicates).
//
// Arithmetic: f32 without contraction (-ffp-contract=off, the Makefile's rule for this file), as noise.hip.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mpt_types.h"
#include "film_ops.h"
#include "noise_pixel.h"

enum { AD_BLOCK = 256, AD_WAVE = 64, AD_WAVES = AD_BLOCK / AD_WAVE, AD_HALO = MPT_TILE + 2, AD_CELLS = AD_HALO * AD_HALO };
enum { AD_VALID = 1, AD_ABOVE = 2 };
static_assert(AD_BLOCK == MPT_TILE * MPT_TILE, "one lane per pixel of a tile");

__global__ __launch_bounds__(AD_BLOCK) void adapt_select_kernel(const float4 *__restrict__ film, const float4 *__restrict__ mark, int nx, int ny,
                                                                int tiles_y, float threshold, int dilate,
                                                                unsigned long long *__restrict__ ballot, int *__restrict__ count) {
    __shared__ unsigned char s_state[AD_CELLS];
    __shared__ int s_count[AD_WAVES];
    const int ti = (int)blockIdx.x / tiles_y, tj = (int)blockIdx.x - ti * tiles_y;
    const int i0 = ti * MPT_TILE - 1, j0 = tj * MPT_TILE - 1;                  // the halo's corner
    for (int c = (int)threadIdx.x; c < AD_CELLS; c += AD_BLOCK) {
        const int ci = c / AD_HALO, cj = c - ci * AD_HALO;
        const int i = i0 + ci, j = j0 + cj;
        const bool rim = ci == 0 || ci == AD_HALO - 1 || cj == 0 || cj == AD_HALO - 1;
        unsigned char st = 0;
        if (i >= 0 && i < nx && j >= 0 && j < ny && (dilate || !rim)) {
            const size_t p = (size_t)i * ny + j;
            float e;
            if (nz_pixel(film[p], mark[p], &e)) st = e > threshold ? (AD_VALID | AD_ABOVE) : AD_VALID;
        }
        s_state[c] = st;
    }
    __syncthreads();
    const int c = (((int)threadIdx.x >> 4) + 1) * AD_HALO + ((int)threadIdx.x & 15) + 1;
    unsigned any = s_state[c];
    bool active = false;
    if (any & AD_VALID) {                                                     // (a lane past the film's edge holds 0)
        if (dilate) {
#pragma unroll
            for (int di = -1; di <= 1; di++)
#pragma unroll
                for (int dj = -1; dj <= 1; dj++) any |= s_state[c + di * AD_HALO + dj];
        }
        active = (any & AD_ABOVE) != 0;
    }
    const unsigned long long b = __ballot(active);
    const int wave = (int)threadIdx.x / AD_WAVE;
    if (((int)threadIdx.x & (AD_WAVE - 1)) == 0) {
        ballot[(size_t)blockIdx.x * AD_WAVES + wave] = b;
        s_count[wave] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) count[blockIdx.x] = (s_count[0] + s_count[1]) + (s_count[2] + s_count[3]);
}

// count[0 .. ntiles) := its exclusive prefix sum; *total_host = the sum.  Lane t takes the run [t per, (t + 1) per) of tiles
__global__ __launch_bounds__(AD_BLOCK) void adapt_scan_kernel(int *__restrict__ count, int ntiles, long long *__restrict__ total_host) {
    __shared__ int s_sum[AD_BLOCK];
    const int t = (int)threadIdx.x;
    const int per = (ntiles + AD_BLOCK - 1) / AD_BLOCK;
    const int lo = min(t * per, ntiles), hi = min(lo + per, ntiles);
    int own = 0;
    for (int q = lo; q < hi; q++) own += count[q];
    s_sum[t] = own;
    __syncthreads();
    for (int d = 1; d < AD_BLOCK; d <<= 1) {                                   // inclusive scan of the 256 lanes' sums
        const int v = t >= d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    int run = s_sum[t] - own;
    for (int q = lo; q < hi; q++) { const int n = count[q]; count[q] = run; run += n; }
    if (t == AD_BLOCK - 1) *total_host = (long long)s_sum[t];
}

__global__ __launch_bounds__(AD_BLOCK) void adapt_scatter_kernel(const unsigned long long *__restrict__ ballot, const int *__restrict__ offset,
                                                                 int ny, int tiles_y, int32_t *__restrict__ list) {
    const int ti = (int)blockIdx.x / tiles_y, tj = (int)blockIdx.x - ti * tiles_y;
    const int wave = (int)threadIdx.x / AD_WAVE, lane = (int)threadIdx.x & (AD_WAVE - 1);
    int at = offset[blockIdx.x];
    for (int w = 0; w < wave; w++) at += __popcll(ballot[(size_t)blockIdx.x * AD_WAVES + w]);
    const unsigned long long mine = ballot[(size_t)blockIdx.x * AD_WAVES + wave];
    if ((mine >> lane) & 1ull) {                                              // (only pixels inside the film are ever set)
        const int i = ti * MPT_TILE + ((int)threadIdx.x >> 4), j = tj * MPT_TILE + ((int)threadIdx.x & 15);
        list[at + __popcll(mine & ((1ull << lane) - 1ull))] = i * ny + j;
    }
}

__global__ __launch_bounds__(AD_BLOCK) void adapt_fold_kernel(float4 *__restrict__ film, float4 *__restrict__ mark, const int32_t *__restrict__ list,
                                                              int count, const float4 *__restrict__ samples, int nframes, int remark) {
    const int k = (int)blockIdx.x * AD_BLOCK + (int)threadIdx.x;
    if (k >= count) return;
    const int pix = list[k];
    const float4 f0 = film[pix];
    if (remark) mark[pix] = f0;
    MptVec4 acc = { f0.x, f0.y, f0.z, f0.w };
    for (int f = 0; f < nframes; f++) {
        const float4 s = samples[(size_t)f * count + k];
        film_add_sample(acc, s.x, s.y, s.z);
    }
    film[pix] = make_float4(acc.x, acc.y, acc.z, acc.w);
}

// ---------------------------------------------------------------- launchers
// tiles of an nx x ny film; a film of npix pixels has at most mpt_adapt_tile_bound(npix) whatever its shape
MPT_KERNEL_API size_t mpt_adapt_tiles(int nx, int ny) {
    return (size_t)((nx + MPT_TILE - 1) / MPT_TILE) * (size_t)((ny + MPT_TILE - 1) / MPT_TILE);
}
MPT_KERNEL_API size_t mpt_adapt_tile_bound(size_t npix) { return npix / MPT_TILE + 2; }   // (reached by a film one pixel wide)

// ballot: 4 words per tile; count: one int per tile (left holding the tiles' offsets); list: room for nx * ny indices;
// total_host: the device alias of the host's mapped count
MPT_KERNEL_API hipError_t mpt_launch_adapt_select(const MptVec4 *film, const MptVec4 *mark, int nx, int ny, float threshold, int dilate,
                                                  unsigned long long *ballot, int *count, int32_t *list, long long *total_host,
                                                  hipStream_t stream) {
    const size_t ntiles = mpt_adapt_tiles(nx, ny);
    if (nx < 1 || ny < 1 || ntiles > 0x7fffffffULL || (size_t)nx * ny > 0x7fffffffULL) return hipErrorInvalidConfiguration;
    const int tiles_y = (ny + MPT_TILE - 1) / MPT_TILE;
    hipLaunchKernelGGL(adapt_select_kernel, dim3((unsigned)ntiles), dim3(AD_BLOCK), 0, stream, (const float4 *)film, (const float4 *)mark, nx, ny,
                       tiles_y, threshold, dilate, ballot, count);
    hipLaunchKernelGGL(adapt_scan_kernel, dim3(1), dim3(AD_BLOCK), 0, stream, count, (int)ntiles, total_host);
    hipLaunchKernelGGL(adapt_scatter_kernel, dim3((unsigned)ntiles), dim3(AD_BLOCK), 0, stream, (const unsigned long long *)ballot,
                       (const int *)count, ny, tiles_y, list);
    return hipGetLastError();
}

// samples: [nframes][count]; mark may be null when remark is 0
MPT_KERNEL_API hipError_t mpt_launch_adapt_fold(MptVec4 *film, MptVec4 *mark, const int32_t *list, int count, const MptVec4 *samples,
                                                int nframes, int remark, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(adapt_fold_kernel, dim3((unsigned)((count + AD_BLOCK - 1) / AD_BLOCK)), dim3(AD_BLOCK), 0, stream, (float4 *)film,
                       (float4 *)mark, list, count, (const float4 *)samples, nframes, remark);
    return hipGetLastError();
}

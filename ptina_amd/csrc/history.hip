// history.hip -- the kernels of the film's reprojection that do not trace (mpt_history_keep, mpt_history_reproject,
// mpt_history_eval; film_history.cpp; the numpy restatement tests/reproject_ref.py).
//
//   keep verts   the positions of the model as the kept view sees it: 36 of a face's 96 bytes, [face][corner][xyz], one lane per face.
//   resample     one lane per pixel of the WHOLE film, workgroup b the elements [256 b, 256 (b + 1)): F_new of the pixel from the old
//                accumulators, the kept G-buffer and the pixel's motion record (history_rule.h mpt_history_pixel, which is the
//                definition), zeros outside the context's slab or stripes.  A divergent gather: 20 bytes of motion record, then per
//                tap that lies in the film 4 + 4 bytes of G-buffer and, where they agree, ONE 16-byte load of the old accumulators;
//                one 16-byte store.  It reads one buffer and writes another (the host swaps them), so no pixel sees a value of this
//                launch, there is no atomic, and the film repeats bit for bit.  No LDS but the fold's four records.
//   the fold     what became of the pixels, counted per workgroup and folded by ONE workgroup into the host's mapped record: both
//                stages are film_fold.h's, whose integer sums are exact and independent of the order.
//
// Arithmetic: f32 without contraction (history_rule.h states it per function; the Makefile's rule for this file says the same),
// IEEE division, denormals kept -- hipcc's defaults for HIP code.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/miptina.h"
#include "mpt_types.h"
#include "film_fold.h"
#include "history_rule.h"

enum { HS_BLOCK = 256 };
static_assert(HS_BLOCK == FILM_FOLD_BLOCK, "the fold is written for this block");

// the counts as they are summed; a partial is one of these in the room of an mpt_history_stats
struct HsAcc {
    long long n[MPT_OUTCOMES];
    static __device__ __forceinline__ HsAcc zero() { return {}; }
    __device__ __forceinline__ void add(const HsAcc &o) {
#pragma unroll
        for (int k = 0; k < MPT_OUTCOMES; k++) n[k] += o.n[k];
    }
    __device__ __forceinline__ HsAcc across(int h) const {
        HsAcc r;
#pragma unroll
        for (int k = 0; k < MPT_OUTCOMES; k++) r.n[k] = film_lane_xor(n[k], h);
        return r;
    }
};
static_assert(sizeof(HsAcc) == sizeof(mpt_history_stats), "a partial is one 48-byte record");

__global__ __launch_bounds__(256) void history_verts_kernel(const float *__restrict__ verts, float *__restrict__ kept, int n) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int d = 0; d < 3; d++) kept[(size_t)f * 9 + c * 3 + d] = verts[(size_t)f * 24 + c * 8 + d];
}

// is column x of the film one this context renders?  (film_read.cpp own_column)
__device__ __forceinline__ bool own_column(const MptResampleArgs &a, int x) {
    if (x < a.x0 || x >= a.x1) return false;
    return a.stripe_w == 0 || (x / a.stripe_w) % a.stripe_mod == a.stripe_idx;
}

__global__ __launch_bounds__(HS_BLOCK) void history_resample_kernel(const MptResampleArgs a, HsAcc *__restrict__ part) {
    __shared__ HsAcc s_wave[FILM_FOLD_WAVES];
    const size_t npix = (size_t)a.nx * a.ny;
    const size_t t = (size_t)blockIdx.x * HS_BLOCK + threadIdx.x;
    HsAcc acc = HsAcc::zero();
    if (t < npix) {
        const int i = (int)(t / (size_t)a.ny), j = (int)(t - (size_t)i * a.ny);
        MptVec4 out = { 0.0f, 0.0f, 0.0f, 0.0f };
        if (own_column(a, i)) {
            const MptMotion m = a.motion[t];
            const MptHistoryOutcome o = mpt_history_pixel(a.f_old, a.face, a.id, a.depth, a.nx, a.ny, i, j, m, a.max_history, a.depth_tol, &out);
            acc.n[o == MPT_OUTCOME_STATIC ? MPT_OUTCOME_KEPT : o] = 1;          // (a static pixel is a kept one ...
            if (o == MPT_OUTCOME_STATIC) acc.n[MPT_OUTCOME_STATIC] = 1;          //  ... and counts as both)
        }
        a.f_new[t] = out;
    }
    const HsAcc tot = film_block_fold(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(HS_BLOCK) void history_fold_kernel(const HsAcc *__restrict__ part, int nparts, mpt_history_stats *__restrict__ stats_host) {
    __shared__ HsAcc s_wave[FILM_FOLD_WAVES];
    const HsAcc tot = film_fold_parts(part, nparts, s_wave);
    if (threadIdx.x == 0) {
        stats_host->kept = tot.n[MPT_OUTCOME_KEPT]; stats_host->statics = tot.n[MPT_OUTCOME_STATIC];
        stats_host->background_kept = tot.n[MPT_OUTCOME_BACKGROUND_KEPT]; stats_host->disoccluded = tot.n[MPT_OUTCOME_DISOCCLUDED];
        stats_host->offscreen = tot.n[MPT_OUTCOME_OFFSCREEN]; stats_host->background_reset = tot.n[MPT_OUTCOME_BACKGROUND_RESET];
    }
}

// ---------------------------------------------------------------- launchers
MPT_KERNEL_API size_t mpt_history_parts(size_t npix) { return film_fold_count(npix, HS_BLOCK); }

// kept: [n][9] floats from the model's [3 n][8] records; n == 0 launches nothing
MPT_KERNEL_API hipError_t mpt_launch_history_verts(const float *verts, float *kept, int n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(history_verts_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, verts, kept, n);
    return hipGetLastError();
}

// part: mpt_history_parts(nx * ny) records (at least one); stats_host: the device alias of the host's mapped record
MPT_KERNEL_API hipError_t mpt_launch_history_resample(const MptResampleArgs *a, mpt_history_stats *part, mpt_history_stats *stats_host, hipStream_t stream) {
    unsigned nparts;
    if (const hipError_t e = film_fold_grid((size_t)a->nx * a->ny, HS_BLOCK, &nparts)) return e;
    if (nparts) hipLaunchKernelGGL(history_resample_kernel, dim3(nparts), dim3(HS_BLOCK), 0, stream, *a, (HsAcc *)part);
    hipLaunchKernelGGL(history_fold_kernel, dim3(1), dim3(HS_BLOCK), 0, stream, (const HsAcc *)part, (int)nparts, stats_host);
    return hipGetLastError();
}

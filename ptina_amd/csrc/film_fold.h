// film_fold.h -- the film's deterministic two-stage sum, stated once for every quantity a read-back meters over the film (the
// display's exposure, display.hip; the noise statistics, noise.hip).
//
//   first stage   workgroup b of 256 lanes takes the film elements [run b, run (b + 1)), lane t the elements run b + t + 256 k,
//                 k ascending (the feature's own loop; its run length is its own), folds the lanes' accumulators with
//                 film_block_fold and leaves one accumulator, part[b].
//   second stage  ONE workgroup: film_fold_parts -- lane t takes the partials t, t + 256, ... ascending, then the same block fold --
//                 and lane 0 writes the result to a host-mapped word.
// The shape of the sum is a function of the number of elements and the run length alone -- not of how many CUs a launch got --
// and there is no atomic: every sum, count and maximum repeats bit for bit.
//
// An accumulator type A is an aggregate that supplies
//     static A zero();              the empty sum
//     void add(const A &o);         this += o, field by field (a + b must be b + a bit for bit: the butterfly relies on it)
//     A across(int h) const;        the accumulator of lane l ^ h of the wave: film_lane_xor on each field
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

enum { FILM_FOLD_BLOCK = 256, FILM_FOLD_WAVE = 64, FILM_FOLD_WAVES = FILM_FOLD_BLOCK / FILM_FOLD_WAVE };

// the value lane l ^ h of the wave holds (f32, f64, i64: a 64-bit value crosses as its two words)
template <class T>
__device__ __forceinline__ T film_lane_xor(T v, int h) { return __shfl_xor(v, h, FILM_FOLD_WAVE); }

// The 256 lanes' accumulators: a butterfly within each wave (lane l takes lane l ^ h, h = 32, 16, ..., 1: every lane ends with the
// wave's total), then the four waves' totals through LDS (s_wave[FILM_FOLD_WAVES]), added in ascending order by every lane
template <class A>
__device__ __forceinline__ A film_block_fold(A v, A *s_wave) {
#pragma unroll
    for (int h = FILM_FOLD_WAVE / 2; h > 0; h >>= 1) v.add(v.across(h));
    if ((threadIdx.x & (FILM_FOLD_WAVE - 1)) == 0) s_wave[threadIdx.x / FILM_FOLD_WAVE] = v;
    __syncthreads();
    A tot = s_wave[0];
#pragma unroll
    for (int w = 1; w < FILM_FOLD_WAVES; w++) tot.add(s_wave[w]);
    return tot;
}

// the second stage, by one workgroup of FILM_FOLD_BLOCK lanes
template <class A>
__device__ __forceinline__ A film_fold_parts(const A *__restrict__ part, int nparts, A *s_wave) {
    A acc = A::zero();
    for (int q = (int)threadIdx.x; q < nparts; q += FILM_FOLD_BLOCK) acc.add(part[q]);
    return film_block_fold(acc, s_wave);
}

// launch side: the first stage's workgroups (= partials) for npix elements in runs of `run`, and the refusal of a count that no
// grid, and no int, holds
static inline size_t film_fold_count(size_t npix, size_t run) { return (npix + run - 1) / run; }
static inline hipError_t film_fold_grid(size_t npix, size_t run, unsigned *nparts) {
    const size_t n = film_fold_count(npix, run);
    if (n > 0x7fffffffULL) return hipErrorInvalidConfiguration;
    *nparts = (unsigned)n;
    return hipSuccess;
}

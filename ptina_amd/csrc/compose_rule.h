// compose_rule.h -- how a world matrix places a point of a mesh, stated once for compose.hip's
// compose_vertex, which rounds the result to f32 at its store, and for scatter.hip (scatter_rule.h), which keeps it in f64.
// Plain C++17 that a host compiler takes as it is; under hipcc the same function is the kernels' arithmetic.  f64, every sum left
// to right, never contracted (the pragma for a host compiler, -ffp-contract=off for the .hip files: the Makefile's rule).
#pragma once

#if defined(__HIPCC__)
#define MPT_HD __host__ __device__ inline
#else
#define MPT_HD inline
#endif
#if defined(__clang__)
#define MPT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MPT_NO_CONTRACT
#endif

// Component j of ph = (p, 1) . W^T for the row-major 4x4 matrix W: the point is ph.xyz / ph.w, a real divide (W need not be affine)
MPT_HD double mpt_place_row(const double p[3], const double *W, int j) {
    MPT_NO_CONTRACT
    return ((p[0] * W[4 * j] + p[1] * W[4 * j + 1]) + p[2] * W[4 * j + 2]) + W[4 * j + 3];
}

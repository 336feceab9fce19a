// noise_pixel.h -- the noise estimate e of ONE pixel, from its film accumulator F and its mark M: the one definition behind the
// noise map and statistics (noise.hip) and the selection of the pixels that still need samples (adapt_select.hip).  The
// definition is in include/miptina.h (mpt_get_noise), the numpy restatement in tests/noise_ref.py.
//
// Arithmetic: f32 without contraction -- both files are built with -ffp-contract=off -- with hipcc's IEEE-rounded division and
// square root and denormals kept: every operation of e is one correctly rounded f32 operation.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "film_ops.h"

// e of one pixel; false (and e = 0) where the pixel is not valid
__device__ __forceinline__ bool nz_pixel(const float4 F, const float4 M, float *e) {
    const float nA = M.w, n = F.w, nB = n - nA;
    *e = 0.0f;
    if (!(nA > 0.0f && nB > 0.0f)) return false;
    const float a[3] = { film_sanitise(M.x / nA), film_sanitise(M.y / nA), film_sanitise(M.z / nA) };
    const float m[3] = { film_sanitise(F.x / n), film_sanitise(F.y / n), film_sanitise(F.z / n) };
    const float k = sqrtf(nA / nB);
    const float d[3] = { fabsf(m[0] - a[0]) * k, fabsf(m[1] - a[1]) * k, fabsf(m[2] - a[2]) * k };
    const float num = ((d[0] + d[1]) + d[2]) / 3.0f;
    const float den = 1e-4f + sqrtf(((m[0] + m[1]) + m[2]) / 3.0f);
    *e = film_sanitise(num / den);          // (the clamp moves only a value that is not finite: saturated channels overflow the sums)
    return true;
}

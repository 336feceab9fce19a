// wide_quant.h -- what the 4-wide collapse (wide_build.hip) and the refit (refit.hip) both say about a record: how the binary
// record is taken apart, the surface-area figure in fixed point, and the quantisation of a wide node's child boxes to 8 bits.
// Stated once, so the collapse and the refit write the same bytes; both files are compiled with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>
#include <cmath>
#include "mpt_types.h"

struct WbChild { int id; float lo[3], hi[3]; };

__device__ __forceinline__ int wb_asi(float f) { return __float_as_int(f); }
__device__ __forceinline__ float wb_asf(int v) { return __int_as_float(v); }

__device__ __forceinline__ void wb_children_of(const MptVec4 *__restrict__ fnode, int b, WbChild out[2]) {
    const MptVec4 r0 = fnode[(size_t)b * 4 + 0], r1 = fnode[(size_t)b * 4 + 1], r2 = fnode[(size_t)b * 4 + 2], r3 = fnode[(size_t)b * 4 + 3];
    out[0].id = wb_asi(r3.x); out[1].id = wb_asi(r3.y);
    out[0].lo[0] = r0.x; out[1].lo[0] = r0.y; out[0].hi[0] = r0.z; out[1].hi[0] = r0.w;
    out[0].lo[1] = r1.x; out[1].lo[1] = r1.y; out[0].hi[1] = r1.z; out[1].hi[1] = r1.w;
    out[0].lo[2] = r2.x; out[1].lo[2] = r2.y; out[0].hi[2] = r2.z; out[1].hi[2] = r2.w;
}

__device__ __forceinline__ float wb_area(const WbChild &c) {
    const float dx = fmaxf(c.hi[0] - c.lo[0], 0.f), dy = fmaxf(c.hi[1] - c.lo[1], 0.f), dz = fmaxf(c.hi[2] - c.lo[2], 0.f);
    return dx * dy + dy * dz + dz * dx;
}

// the surface area of the root's box (the union of the two children of record 0), and an area in units of 2^-40 of it
__device__ __forceinline__ double wb_root_area(const MptVec4 *__restrict__ fnode) {
    WbChild ch[2];
    wb_children_of(fnode, 0, ch);
    WbChild root = ch[0];
    for (int k = 0; k < 3; k++) { root.lo[k] = fminf(ch[0].lo[k], ch[1].lo[k]); root.hi[k] = fmaxf(ch[0].hi[k], ch[1].hi[k]); }
    return (double)wb_area(root);
}

__device__ __forceinline__ unsigned long long wb_fixed_share(float a, double ra) {
    if (!(ra > 0.0)) return 0ull;
    const double r = fmin(fmax((double)a / ra, 0.0), 1.0);
    return (unsigned long long)(r * 1099511627776.0);
}

// surface areas are summed as integers in units of 2^-40 of the root's (the sum of <= 2^22 of them stays below 2^63): the
// figure is the same bits run to run, whatever order the lanes arrive in (round-3 ADVICE: it was a double atomicAdd per lane)
__device__ __forceinline__ unsigned long long wb_area_fixed(const MptVec4 *__restrict__ fnode, float a) {
    return wb_fixed_share(a, wb_root_area(fnode));
}

// The quantised record of a wide node whose used children are ch[0 .. cnt) and whose id row is ids: child planes as bytes over
// the node's own box, rounded outwards by a quarter of a step more than needed (the kernel's decode
// q * (scale * inv) + (origin * inv - o * inv) is off by far less).  qo: the node's four float4
__device__ __forceinline__ void wb_quantise(const WbChild *ch, int cnt, const int ids[4], MptVec4 *qo) {
    float plo[3] = { INFINITY, INFINITY, INFINITY }, phi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int k = 0; k < cnt; k++)
        for (int a = 0; a < 3; a++) { plo[a] = fminf(plo[a], ch[k].lo[a]); phi[a] = fmaxf(phi[a], ch[k].hi[a]); }
    float scale[3];
    unsigned qlo[3] = { 0, 0, 0 }, qhi[3] = { 0, 0, 0 };
    for (int a = 0; a < 3; a++) {
        const float e = phi[a] - plo[a];
        float sc = e > 0.f ? e / 255.f : 0.f;
        // 255 steps must reach the far side in f32, and a flat node still needs a positive step
        while (e > 0.f && plo[a] + 255.f * sc < phi[a]) sc = nextafterf(sc, INFINITY);
        if (!(sc > 0.f)) sc = fmaxf(fabsf(plo[a]) * 1e-6f, 1e-30f);
        scale[a] = sc;
        for (int k = 0; k < 4; k++) {
            unsigned l = 255, h = 0;                  // unused child: an inverted box
            if (k < cnt) {
                const float fl = floorf((ch[k].lo[a] - plo[a]) / sc - 0.25f), fh = ceilf((ch[k].hi[a] - plo[a]) / sc + 0.25f);
                l = (unsigned)fminf(255.f, fmaxf(0.f, fl));
                h = (unsigned)fminf(255.f, fmaxf(0.f, fh));
            }
            qlo[a] |= l << (8 * k); qhi[a] |= h << (8 * k);
        }
    }
    qo[0] = { plo[0], plo[1], plo[2], scale[0] };
    qo[1] = { scale[1], scale[2], wb_asf((int)qlo[0]), wb_asf((int)qhi[0]) };
    qo[2] = { wb_asf((int)qlo[1]), wb_asf((int)qhi[1]), wb_asf((int)qlo[2]), wb_asf((int)qhi[2]) };
    qo[3] = { wb_asf(ids[0]), wb_asf(ids[1]), wb_asf(ids[2]), wb_asf(ids[3]) };
}

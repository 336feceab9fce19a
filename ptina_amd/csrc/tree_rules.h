// tree_rules.h -- the rules of the tree builders, each stated once: what a triangle's box, centre and Morton key are, which
// two children an LBVH node has, how the binary record (fnode) and the 4-wide records (wnode, qnode) are laid out, how a wide
// node grows from a binary one, the quantisation of its child boxes to 8 bits and the surface-area figures.
//
// One definition for every pass that builds or fits a tree: the host passes (tree_host.h, behind tree_build.cpp and the
// stand-alone tools/tree_rules_check.cpp) and the device passes (lbvh_build.hip, sah_build.hip, wide_build.hip, refit.hip),
// in IEEE arithmetic without contraction whatever the flags of the including file, so that they write the same bytes.  Plain
// C++17; nothing of HIP unless the HIP compiler reads it.  What stays with the kernels is how words cross between lanes
// (atomics, tickets, reductions): these functions only compute.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstring>
#include "mpt_types.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MPT_HD __host__ __device__ inline
#else
#define MPT_HD inline
#endif

// ------------------------------------------------------------------ words
MPT_HD float asf(int v) { float f; memcpy(&f, &v, 4); return f; }
MPT_HD int asi(float f) { int v; memcpy(&v, &f, 4); return v; }

// order-preserving float <-> int (the bounds that are reduced with integer atomics)
MPT_HD int f2ord(float f) { const int i = asi(f); return i >= 0 ? i : i ^ 0x7fffffff; }
MPT_HD float ord2f(int i) { return asf(i >= 0 ? i : i ^ 0x7fffffff); }

// ------------------------------------------------------------------ a triangle of the model (verts: [3n][8] = pos3 nrm3 uv2)
MPT_HD const float *vpos(const float *verts, int f, int k) { return verts + ((size_t)f * 3 + k) * 8; }

MPT_HD void leaf_box(const float *verts, int f, float *lo, float *hi) {         // lbvh.py:155-158
#pragma clang fp contract(off)
    for (int a = 0; a < 3; a++) {
        lo[a] = fminf(fminf(vpos(verts, f, 0)[a], vpos(verts, f, 1)[a]), vpos(verts, f, 2)[a]);
        hi[a] = fmaxf(fmaxf(vpos(verts, f, 0)[a], vpos(verts, f, 1)[a]), vpos(verts, f, 2)[a]);
    }
}

MPT_HD float centroid(const float *verts, int f, int a) {                       // lbvh.py:161-165
#pragma clang fp contract(off)
    return ((vpos(verts, f, 0)[a] + vpos(verts, f, 1)[a]) + vpos(verts, f, 2)[a]) / 3.0f;
}

// ------------------------------------------------------------------ the LBVH's keys and hierarchy
MPT_HD unsigned expand_bits(unsigned v) {                                       // lbvh.py:13-17
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

MPT_HD int quant1024(float x) {                                                 // clamp(ifloor(v * 1024), 0, 1023), lbvh.py:29
#pragma clang fp contract(off)
    float f = floorf(x * 1024.0f);
    if (!(f == f) || f < 0.f) return 0;
    if (f > 1023.f) return 1023;
    return (int)f;
}

// The sort key of face f: the 30-bit Morton code of its centre within the centres' bounds, then the face -- unique, so equal
// codes cannot corrupt the hierarchy.  bmin / bmax: the bounds over all centres, starting from +-1e6 (lbvh.py:173,179-183)
MPT_HD unsigned long long morton_key(const float *cen, const float *bmin, const float *bmax, int f) {
#pragma clang fp contract(off)
    unsigned w[3];
    for (int a = 0; a < 3; a++) w[a] = expand_bits((unsigned)quant1024((cen[a] - bmin[a]) / (bmax[a] - bmin[a])));
    const unsigned code = w[0] * 4 + w[1] * 2 + w[2];
    return ((unsigned long long)code << 32) | (unsigned)f;
}

MPT_HD int delta(const unsigned long long *key, int n, int i, int j) {          // (the keys differ: never clz(0))
    if (j < 0 || j >= n) return -1;
    return __builtin_clzll(key[i] ^ key[j]);
}

// The two children of internal node i over the n sorted keys: a leaf slot (< n) or an internal node + n.
// lbvh.py:212-231 (determineRange :93-146, findSplit :62-89)
MPT_HD void lbvh_children(const unsigned long long *key, int n, int i, int *c0, int *c1) {
    int l, r;
    if (i == 0) { l = 0; r = n - 1; }
    else {
        int d = delta(key, n, i, i + 1) > delta(key, n, i, i - 1) ? 1 : -1;
        int dmin = delta(key, n, i, i - d);
        int lmax = 2;
        while (delta(key, n, i, i + lmax * d) > dmin) lmax <<= 1;
        int s = 0;
        for (int t = lmax >> 1; t > 0; t >>= 1)
            if (delta(key, n, i, i + (s + t) * d) > dmin) s += t;
        l = i; r = i + s * d;
        if (d < 0) { int tmp = l; l = r; r = tmp; }
    }
    int cp = delta(key, n, l, r);
    int m = l, s = r - l;
    for (;;) {
        s = (s + 1) >> 1;
        int q = m + s;
        if (q < r && delta(key, n, l, q) > cp) m = q;
        if (s <= 1) break;
    }
    *c0 = (m == l) ? m : m + n;
    *c1 = (m + 1 == r) ? m + 1 : m + 1 + n;
}

// such a child as the fast build's records name it: an internal node >= 0, leaf slot s as ~s
MPT_HD int lbvh_fast_id(int ch, int n) { return ch < n ? ~ch : ch - n; }

// ------------------------------------------------------------------ boxes
MPT_HD float half_area(const float *l, const float *h) {                        // half the surface area; an inverted box has none
#pragma clang fp contract(off)
    const float dx = fmaxf(h[0] - l[0], 0.f), dy = fmaxf(h[1] - l[1], 0.f), dz = fmaxf(h[2] - l[2], 0.f);
    return dx * dy + dy * dz + dz * dx;
}

struct WbChild { int id; float lo[3], hi[3]; };

MPT_HD float wb_area(const WbChild &c) { return half_area(c.lo, c.hi); }

// the area of the node whose two children these are: of their union
MPT_HD float wb_own_area(const WbChild two[2]) {
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = fminf(two[0].lo[a], two[1].lo[a]); hi[a] = fmaxf(two[0].hi[a], two[1].hi[a]); }
    return half_area(lo, hi);
}

// ------------------------------------------------------------------ the binary record (fnode, mpt_types.h)
// 16 words: {c0.lo.x, c1.lo.x, c0.hi.x, c1.hi.x} {y} {z} {id0, id1, 0, 0}; an id >= 0 is an internal node, an id < 0 leaf slot ~id
MPT_HD constexpr int fnode_lo(int k, int a) { return a * 4 + k; }
MPT_HD constexpr int fnode_hi(int k, int a) { return a * 4 + 2 + k; }
MPT_HD constexpr int fnode_id(int k) { return 12 + k; }
#define FNODE_ID_ROW 3          // the float4 of an fnode record that holds the ids

MPT_HD void wb_children_of(const MptVec4 *__restrict__ fnode, int b, WbChild out[2]) {
    MptVec4 r[4];
    for (int q = 0; q < 4; q++) r[q] = fnode[(size_t)b * 4 + q];
    const float *w = &r[0].x;
    for (int k = 0; k < 2; k++) {
        out[k].id = asi(w[fnode_id(k)]);
        for (int a = 0; a < 3; a++) { out[k].lo[a] = w[fnode_lo(k, a)]; out[k].hi[a] = w[fnode_hi(k, a)]; }
    }
}

// child k (0 / 1) of node i, with par2 = 2 * i + k, has this box and id
MPT_HD void fnode_write_child(MptVec4 *__restrict__ fnode, int par2, const float *l, const float *h, int id) {
    float *r = &fnode[(size_t)(par2 >> 1) * 4].x;
    const int k = par2 & 1;
    for (int a = 0; a < 3; a++) { r[fnode_lo(k, a)] = l[a]; r[fnode_hi(k, a)] = h[a]; }
    r[fnode_id(k)] = asf(id);
}

// ------------------------------------------------------------------ the 4-wide records (wnode, qnode)
// wnode, 32 words: {lo.x[4]} {hi.x[4]} {lo.y[4]} {hi.y[4]} {lo.z[4]} {hi.z[4]} {id[4]} {-}; the used slots come first
MPT_HD constexpr int wnode_lo(int k, int a) { return (2 * a) * 4 + k; }
MPT_HD constexpr int wnode_hi(int k, int a) { return (2 * a + 1) * 4 + k; }
MPT_HD constexpr int wnode_id(int k) { return 24 + k; }
#define WNODE_ID_ROW 6          // the float4 of a wnode record that holds the ids (of a qnode record: the last, 3)

MPT_HD MptVec4 wb_id_row(const int ids[4]) { return { asf(ids[0]), asf(ids[1]), asf(ids[2]), asf(ids[3]) }; }

// The collapse's grow step.  ch[0], ch[1]: the two children of a binary node; the internal child with the largest surface area
// is replaced by its own two children until four are held or only leaves are left.  -> how many are held
MPT_HD int wb_grow(const MptVec4 *__restrict__ fnode, WbChild ch[4]) {
    int cnt = 2;
    while (cnt < 4) {
        int best = -1; float ba = -1.f;
        for (int k = 0; k < cnt; k++)
            if (ch[k].id >= 0) { const float a = wb_area(ch[k]); if (a > ba) { ba = a; best = k; } }
        if (best < 0) break;
        WbChild two[2];
        wb_children_of(fnode, ch[best].id, two);
        ch[best] = two[0];
        ch[cnt++] = two[1];
    }
    return cnt;
}

// The exact record of a wide node that holds ch[0 .. cnt): rec, and its id row once more in ids -- an internal child by the
// BINARY node it grows from (the caller numbers it).  An unused slot holds empty_id = ~n, leaf slot n: one extra triangle record
// of NaNs that no ray can hit, and a point box at 1e30, out of every ray's reach
MPT_HD void wb_exact_record(const WbChild *ch, int cnt, int empty_id, int ids[4], MptVec4 rec[8]) {
    float *f = &rec[0].x;
    for (int k = 0; k < 32; k++) f[k] = 0.f;
    for (int k = 0; k < 4; k++) {
        ids[k] = k < cnt ? ch[k].id : empty_id;
        for (int a = 0; a < 3; a++) { f[wnode_lo(k, a)] = k < cnt ? ch[k].lo[a] : 1e30f; f[wnode_hi(k, a)] = k < cnt ? ch[k].hi[a] : 1e30f; }
        f[wnode_id(k)] = asf(ids[k]);
    }
}

// The quantised record of a wide node whose used children are ch[0 .. cnt) and whose id row is ids: child planes as bytes over
// the node's own box, rounded outwards by a quarter of a step more than needed (the kernel's decode
// q * (scale * inv) + (origin * inv - o * inv) is off by far less).  qo: the node's four float4
MPT_HD void wb_quantise(const WbChild *ch, int cnt, const int ids[4], MptVec4 *qo) {
#pragma clang fp contract(off)
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
    qo[1] = { scale[1], scale[2], asf((int)qlo[0]), asf((int)qhi[0]) };
    qo[2] = { asf((int)qlo[1]), asf((int)qhi[1]), asf((int)qlo[2]), asf((int)qhi[2]) };
    qo[3] = wb_id_row(ids);
}

// ------------------------------------------------------------------ the area share in fixed point
// the surface area of the root's box (the union of the two children of record 0), and an area in units of 2^-40 of it
MPT_HD double wb_root_area(const MptVec4 *__restrict__ fnode) {
    WbChild ch[2];
    wb_children_of(fnode, 0, ch);
    return (double)wb_own_area(ch);
}

MPT_HD unsigned long long wb_fixed_share(float a, double ra) {
#pragma clang fp contract(off)
    if (!(ra > 0.0)) return 0ull;
    const double r = fmin(fmax((double)a / ra, 0.0), 1.0);
    return (unsigned long long)(r * 1099511627776.0);
}

// surface areas are summed as integers in units of 2^-40 of the root's (the sum of <= 2^22 of them stays below 2^63): the
// figure is the same bits run to run, whatever order the lanes arrive in
MPT_HD unsigned long long wb_area_fixed(const MptVec4 *__restrict__ fnode, float a) {
    return wb_fixed_share(a, wb_root_area(fnode));
}

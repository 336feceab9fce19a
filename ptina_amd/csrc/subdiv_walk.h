// subdiv_walk.h -- the two walks of the last level that subdiv.hip and displace.hip both do (DESIGN.md sections 3.19, 3.20), each
// stated once: a vertex's ring walk for its normal sum, and a face's walk down the base-4 digits of its index for its corners'
// face-varying uvs -- for a Catmull-Clark copy (section 3.19.2) a quad's walk, from its polygon's fan.  Device code only; f64, every
// sum in the order written (the files that include it are built with -ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mpt_types.h"

struct SdVec { double x, y, z; };
static __device__ __forceinline__ SdVec sd_add(SdVec a, SdVec b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
static __device__ __forceinline__ SdVec sd_sub(SdVec a, SdVec b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
static __device__ __forceinline__ SdVec sd_mul(double s, SdVec a) { return { s * a.x, s * a.y, s * a.z }; }
static __device__ __forceinline__ SdVec sd_at(const double *P, int32_t v) { return { P[(size_t)v * 3], P[(size_t)v * 3 + 1], P[(size_t)v * 3 + 2] }; }

// The normal sum of vertex i of the last level, whose position is v, over the positions P [V_L][3]: N = 0, then
// N += cross(r_k - v, r_k+1 - v) for its faces in ring order (an interior ring closes, a boundary ring does not).  T is the mesh's
// topology block, nrule_at the last level's rules in it
static __device__ __forceinline__ SdVec sd_ring_normal(const int32_t *__restrict__ T, int32_t nrule_at, const double *P, int i, SdVec v) {
    const int32_t head = T[nrule_at + 2 * i], at = T[nrule_at + 2 * i + 1];
    const int kind = head & 3, n = head >> 2;
    const int32_t *__restrict__ ring = T + at;
    const int nfaces = kind == MPT_SUBDIV_VERT_BND ? n - 1 : n;
    SdVec N = { 0.0, 0.0, 0.0 };
    const SdVec A0 = sd_sub(sd_at(P, ring[0]), v);
    SdVec A = A0;
    for (int k = 0; k < nfaces; k++) {
        SdVec B = A0;
        if (k + 1 < n) B = sd_sub(sd_at(P, ring[k + 1]), v);
        const SdVec X = { A.y * B.z - A.z * B.y, A.z * B.x - A.x * B.z, A.x * B.y - A.y * B.x };
        N = sd_add(N, X);
        A = B;
    }
    return N;
}

// The uvs of the three corners of face g of level `levels`: from the control records' (pool, first vertex src_vert) cage face
// g >> 2 levels down the digits of g in base 4, the most significant first, midpoints 0.5 * (u_i + u_j), unrounded
struct SdFaceUv { double u0, v0, u1, v1, u2, v2; };
static __device__ __forceinline__ SdFaceUv sd_face_uv(const float4 *pool, int32_t src_vert, int levels, int g) {
    const size_t parent = ((size_t)src_vert + (size_t)(g >> (2 * levels)) * 3) * 2;
    const float4 p0 = pool[parent + 1], p1 = pool[parent + 3], p2 = pool[parent + 5];
    double u0 = p0.z, v0 = p0.w, u1 = p1.z, v1 = p1.w, u2 = p2.z, v2 = p2.w;
    for (int s = levels - 1; s >= 0; s--) {
        const int d = (g >> (2 * s)) & 3;
        const double m01u = 0.5 * (u0 + u1), m01v = 0.5 * (v0 + v1), m12u = 0.5 * (u1 + u2), m12v = 0.5 * (v1 + v2);
        const double m20u = 0.5 * (u2 + u0), m20v = 0.5 * (v2 + v0);
        const double n0u = d == 0 ? u0 : d == 1 ? u1 : d == 2 ? u2 : m01u, n0v = d == 0 ? v0 : d == 1 ? v1 : d == 2 ? v2 : m01v;
        const double n1u = d == 0 ? m01u : d == 1 ? m12u : d == 2 ? m20u : m12u, n1v = d == 0 ? m01v : d == 1 ? m12v : d == 2 ? m20v : m12v;
        const double n2u = d == 0 ? m20u : d == 1 ? m01u : d == 2 ? m12u : m20u, n2v = d == 0 ? m20v : d == 1 ? m01v : d == 2 ? m12v : m20v;
        u0 = n0u; v0 = n0v; u1 = n1u; v1 = n1v; u2 = n2u; v2 = n2v;
    }
    return { u0, v0, u1, v1, u2, v2 };
}

// Catmull-Clark.  The uvs of the three corners of emitted face g of level `levels`: g is half of quad
// q = g >> 1 of the last level, which descends from quad q >> 2 (levels - 1) of level 1, and that one is quad i of a polygon of n
// corners whose fan starts at triangle `first` of the control records (Q, the mesh's table of level-1 quads: first, n | i << 8).
// Corner j of the polygon has its uv at corner j of the first triangle for j < 2, else at corner 2 of triangle j - 2.  A face
// point's uv is ((u_0 + u_1) + ...) / n in the face's own order, an edge's 0.5 * (u_i + u_j); quad (c_0 .. c_3) has child d
// (c_d, e(c_d, c_d+1), f, e(c_d-1, c_d)), down the base-4 digits of q; the halves of a quad are (0, 1, 2) and (0, 2, 3)
struct SdUv { double u, v; };
static __device__ __forceinline__ SdUv sd_poly_uv(const float4 *pool, int32_t src_vert, int32_t first, int j) {
    const size_t corner = j < 2 ? (size_t)first * 3 + (size_t)j : ((size_t)first + (size_t)(j - 2)) * 3 + 2;
    const float4 p = pool[((size_t)src_vert + corner) * 2 + 1];
    return { (double)p.z, (double)p.w };
}
static __device__ __forceinline__ SdUv sd_uv_mid(SdUv a, SdUv b) { return { 0.5 * (a.u + b.u), 0.5 * (a.v + b.v) }; }
static __device__ __forceinline__ SdFaceUv sd_quad_uv(const float4 *pool, int32_t src_vert, const int32_t *__restrict__ Q, int levels, int g) {
    const int q = g >> 1, q1 = q >> (2 * (levels - 1));
    const int32_t first = Q[2 * q1], ni = Q[2 * q1 + 1];
    const int n = ni & 255, i = ni >> 8;
    const SdUv c0 = sd_poly_uv(pool, src_vert, first, 0), c1 = sd_poly_uv(pool, src_vert, first, 1);
    SdUv s = { c0.u + c1.u, c0.v + c1.v };
    for (int j = 2; j < n; j++) {
        const SdUv c = sd_poly_uv(pool, src_vert, first, j);
        s = { s.u + c.u, s.v + c.v };
    }
    const SdUv ci = sd_poly_uv(pool, src_vert, first, i), cn = sd_poly_uv(pool, src_vert, first, i + 1 < n ? i + 1 : 0);
    const SdUv cp = sd_poly_uv(pool, src_vert, first, i > 0 ? i - 1 : n - 1);
    SdUv a0 = ci, a1 = sd_uv_mid(ci, cn), a2 = { s.u / (double)n, s.v / (double)n }, a3 = sd_uv_mid(cp, ci);
    for (int t = levels - 2; t >= 0; t--) {
        const int d = (q >> (2 * t)) & 3;
        const SdUv f = { (((a0.u + a1.u) + a2.u) + a3.u) / 4.0, (((a0.v + a1.v) + a2.v) + a3.v) / 4.0 };
        const SdUv c = d == 0 ? a0 : d == 1 ? a1 : d == 2 ? a2 : a3, nx = d == 0 ? a1 : d == 1 ? a2 : d == 2 ? a3 : a0;
        const SdUv pv = d == 0 ? a3 : d == 1 ? a0 : d == 2 ? a1 : a2;
        a0 = c; a1 = sd_uv_mid(c, nx); a2 = f; a3 = sd_uv_mid(pv, c);
    }
    if (g & 1) return { a0.u, a0.v, a2.u, a2.v, a3.u, a3.v };
    return { a0.u, a0.v, a1.u, a1.v, a2.u, a2.v };
}

// The uvs of face g of a copy's last level by its mesh's scheme (uniform in a job, so in a workgroup)
static __device__ __forceinline__ SdFaceUv sd_copy_face_uv(const float4 *pool, const MptSubdivJob &o, const int32_t *__restrict__ topo, int g) {
    if (o.rule_at[0]) return sd_quad_uv(pool, o.src_vert, topo + o.topo_at + o.rule_at[0], o.levels, g);
    return sd_face_uv(pool, o.src_vert, o.levels, g);
}

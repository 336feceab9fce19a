// subdiv_walk.h -- the two walks of the last level that subdiv.hip and displace.hip both do (DESIGN.md sections 3.19, 3.20), each
// stated once: a vertex's ring walk for its normal sum, and a face's walk down the base-4 digits of its index for its corners'
// face-varying uvs.  Device code only; f64, every sum in the order written (the files that include it are built with
// -ffp-contract=off).
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

// scatter_rule.h -- the rule of a scatter (the definition stands in include/miptina.h and at the top of
// scatter.hip): the draws, the weight of a face, its integer share, the choice of a face and a point on it, and the world matrix of
// an instance on the surface as it is now.  Plain C++17 with nothing of HIP and no context (as history_rule.h), so that a
// stand-alone program can run all of it under a sanitizer (tools/scatter_rule_check.cpp); under hipcc the same functions are the
// kernels' arithmetic.  The C ABI has selection and placement as mpt_scatter_rule, and the elimination of a spaced scatter -- a
// minimum distance, the last section but one -- as mpt_scatter_space_rule.
//
// Arithmetic: f64, one correctly rounded operation per operator in the order written, never contracted (the pragma below in every
// function that computes, for a host compiler; -ffp-contract=off for scatter.hip, the Makefile's rule), so that
// tests/scatter_ref.py restates every record and every matrix bit for bit.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include "mpt_types.h"         // MptScatterPoint (plain structures and constants)
#include "compose_rule.h"      // MPT_HD, MPT_NO_CONTRACT, mpt_place_row

// ------------------------------------------------------------------ draws
// SplitMix64's finaliser; draw k of instance i is mix(key + 16 i + k) with key = mix(seed).  (k runs to 19 -- the eighth yaw pair
// -- so the last pairs of instance i are the first draws of instance i + 1: they are reached once in 10^4 instances.)
MPT_HD uint64_t mpt_scatter_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
MPT_HD uint64_t mpt_scatter_draw(uint64_t key, uint64_t i, uint32_t k) { return mpt_scatter_mix(key + 16 * i + k); }
// ((d >> 11) + 0.5) * 2^-53: in (0, 1]; the sum is exact below 2^52 and rounds once (to even) from there on, alike everywhere
MPT_HD double mpt_scatter_unit(uint64_t d) {
    MPT_NO_CONTRACT
    return ((double)(d >> 11) + 0.5) * 0x1p-53;
}

// ------------------------------------------------------------------ the surface's world points
// corner `rec` (pos3 ... f32, as the pool holds it) of the surface placed by its world matrix: compose_vertex's position, unrounded
MPT_HD void mpt_scatter_corner(const float *rec, const double *W, double P[3]) {
    MPT_NO_CONTRACT
    const double p[3] = { rec[0], rec[1], rec[2] };
    const double pw = mpt_place_row(p, W, 3);
    for (int k = 0; k < 3; k++) P[k] = mpt_place_row(p, W, k) / pw;
}

MPT_HD void mpt_scatter_cross(const double P0[3], const double P1[3], const double P2[3], double c[3]) {
    MPT_NO_CONTRACT
    const double a[3] = { P1[0] - P0[0], P1[1] - P0[1], P1[2] - P0[2] }, b[3] = { P2[0] - P0[0], P2[1] - P0[1], P2[2] - P0[2] };
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
MPT_HD double mpt_scatter_length(const double c[3]) {
    MPT_NO_CONTRACT
    return std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
}

// ------------------------------------------------------------------ weights
// The density of a face: channel `channel` (0 to 3: r, g, b, a; 4: ((r + g) + b) / 3.0) of the image [nx][ny] of rgba f32 texels
// at the mean ((u0 + u1) + u2) / 3.0 of its corner uvs, by displace.hip's bilinear rule (texels wrapped by Python's modulo),
// clamped to [0, 1]; NaN counts as 0
MPT_HD int64_t mpt_scatter_pymod(int64_t a, int64_t b) { const int64_t r = a % b; return r < 0 ? r + b : r; }
MPT_HD double mpt_scatter_density(const float *texels, int nx, int ny, int channel, const float uv[3][2]) {
    MPT_NO_CONTRACT
    const double u = (((double)uv[0][0] + (double)uv[1][0]) + (double)uv[2][0]) / 3.0, v = (((double)uv[0][1] + (double)uv[1][1]) + (double)uv[2][1]) / 3.0;
    const double px = u * (double)(nx - 1), py = v * (double)(ny - 1);
    const double fx = std::floor(px), fy = std::floor(py);
    if (!(std::fabs(fx) < 0x1p62) || !(std::fabs(fy) < 0x1p62)) return 0.0;      // (never for admitted uvs: they stay below 2^20)
    const int64_t ix = (int64_t)fx, iy = (int64_t)fy;
    const double x0 = px - fx, x1 = py - fy, y0 = 1.0 - x0, y1 = 1.0 - x1;
    const int64_t xa = mpt_scatter_pymod(ix, nx) * ny, xb = mpt_scatter_pymod(ix + 1, nx) * ny, ya = mpt_scatter_pymod(iy, ny), yb = mpt_scatter_pymod(iy + 1, ny);
    const float *t11 = texels + (xb + yb) * 4, *t10 = texels + (xb + ya) * 4, *t00 = texels + (xa + ya) * 4, *t01 = texels + (xa + yb) * 4;
#define MPT_SCATTER_MIX(k) ((((double)t11[k] * x0) * x1 + ((double)t10[k] * x0) * y1) + ((double)t00[k] * y0) * y1) + ((double)t01[k] * y0) * x1
    double d;
    if (channel == 4) { const double hr = MPT_SCATTER_MIX(0), hg = MPT_SCATTER_MIX(1), hb = MPT_SCATTER_MIX(2); d = ((hr + hg) + hb) / 3.0; }
    else d = MPT_SCATTER_MIX(channel);
#undef MPT_SCATTER_MIX
    if (!(d == d)) return 0.0;
    return d < 0.0 ? 0.0 : d > 1.0 ? 1.0 : d;
}

// w = area * dens of the face with world corners P0 P1 P2; a weight that is not finite counts as 0
MPT_HD double mpt_scatter_weight(const double P0[3], const double P1[3], const double P2[3], double dens) {
    MPT_NO_CONTRACT
    double c[3];
    mpt_scatter_cross(P0, P1, P2, c);
    const double w = (0.5 * mpt_scatter_length(c)) * dens;
    return std::isfinite(w) ? w : 0.0;
}

// q = floor(w / wmax * 2^24), at most 2^24: a face below 2^-24 of the largest gets no share.  (wmax > 0: a surface without one is refused)
MPT_HD uint32_t mpt_scatter_quantise(double w, double wmax) {
    MPT_NO_CONTRACT
    if (!(wmax > 0.0) || !(w > 0.0)) return 0;
    return (uint32_t)std::floor(w / wmax * 16777216.0);
}

// ------------------------------------------------------------------ selection
// The sticky record of instance i: cdf [F + 1] is the exclusive scan of q with the total T = cdf[F] > 0 behind it.  The face is the
// largest g with cdf[g] <= t, t = draw 0 mod T: a face with q = 0 shares its cdf with the face behind it and is never the largest
MPT_HD void mpt_scatter_select(const uint64_t *cdf, int64_t F, uint64_t key, uint64_t i, double smin, double smax, int random_yaw, MptScatterPoint *out) {
    MPT_NO_CONTRACT
    const uint64_t t = mpt_scatter_draw(key, i, 0) % cdf[F];
    int64_t a = 0, b = F - 1;
    while (a < b) { const int64_t m = (a + b + 1) >> 1; if (cdf[m] <= t) a = m; else b = m - 1; }
    const double su = std::sqrt(mpt_scatter_unit(mpt_scatter_draw(key, i, 1))), v = mpt_scatter_unit(mpt_scatter_draw(key, i, 2));
    out->face = (int32_t)a; out->pad = 0;
    out->b1 = su * (1.0 - v);
    out->b2 = su * v;
    out->scale = smin + (smax - smin) * mpt_scatter_unit(mpt_scatter_draw(key, i, 3));
    out->cy = 1.0; out->sy = 0.0;
    if (!random_yaw) return;
    for (uint32_t j = 0; j < 8; j++) {       // a unit vector without trigonometry: the first pair inside the unit disc and off its centre
        const double x = 2.0 * mpt_scatter_unit(mpt_scatter_draw(key, i, 4 + 2 * j)) - 1.0, y = 2.0 * mpt_scatter_unit(mpt_scatter_draw(key, i, 5 + 2 * j)) - 1.0;
        const double r2 = x * x + y * y;
        if (!(r2 > 0x1p-20 && r2 <= 1.0)) continue;
        const double len = std::sqrt(r2);
        out->cy = x / len; out->sy = y / len;
        return;
    }
}

// ------------------------------------------------------------------ placement
// a vector at unit length, as the host normalises `up` once
MPT_HD void mpt_scatter_normalise(const double c[3], double n[3]) {
    MPT_NO_CONTRACT
    const double len = mpt_scatter_length(c);
    for (int k = 0; k < 3; k++) n[k] = c[k] / len;
}

// Tangent T0 and bitangent B0 of the unit vector N, with T0 x N = B0 (columns T0, N, B0 are a right-handed frame): the
// construction of Duff et al., "Building an Orthonormal Basis, Revisited" (JCGT 6(1), 2017) -- its second vector is T0, its first
// B0.  s = copysign(1, N.z), a = -1 / (s + N.z), b = (N.x N.y) a; N = (0, 0, -1) takes s = -1 and a = 0.5, no special case
MPT_HD void mpt_scatter_basis(const double N[3], double T0[3], double B0[3]) {
    MPT_NO_CONTRACT
    const double s = std::copysign(1.0, N[2]);
    const double a = -1.0 / (s + N[2]);
    const double b = (N[0] * N[1]) * a;
    B0[0] = 1.0 + (s * (N[0] * N[0])) * a; B0[1] = s * b; B0[2] = -(s * N[0]);
    T0[0] = b; T0[1] = s + (N[1] * N[1]) * a; T0[2] = -N[1];
}

// The world matrix (row-major) of an instance with record r on the face with world corners P0 P1 P2 as they are now: columns
// scale Tn, scale N, scale Bn, P; bottom row 0 0 0 1.  align 0: N is the face's geometric normal (a collapsed face gives NaN);
// else N is `up`, of unit length
// the point of record r on the face with world corners P0 P1 P2: P = (b0 P0 + b1 P1) + b2 P2, b0 = (1 - b1) - b2.  The fourth column
// of the matrix below, and the position a spaced scatter's candidates are held apart by
MPT_HD void mpt_scatter_point_of(const double P0[3], const double P1[3], const double P2[3], const MptScatterPoint &r, double P[3]) {
    MPT_NO_CONTRACT
    const double b0 = (1.0 - r.b1) - r.b2;
    for (int k = 0; k < 3; k++) P[k] = (b0 * P0[k] + r.b1 * P1[k]) + r.b2 * P2[k];
}

MPT_HD void mpt_scatter_place(const double P0[3], const double P1[3], const double P2[3], const MptScatterPoint &r, int align, const double up[3],
                              double world[16]) {
    MPT_NO_CONTRACT
    double N[3], T0[3], B0[3], P[3];
    mpt_scatter_point_of(P0, P1, P2, r, P);
    if (align == 0) {
        double c[3];
        mpt_scatter_cross(P0, P1, P2, c);
        mpt_scatter_normalise(c, N);
    } else {
        N[0] = up[0]; N[1] = up[1]; N[2] = up[2];
    }
    mpt_scatter_basis(N, T0, B0);
    for (int k = 0; k < 3; k++) {
        const double Tn = r.cy * T0[k] + r.sy * B0[k], Bn = r.cy * B0[k] - r.sy * T0[k];
        world[4 * k] = r.scale * Tn;
        world[4 * k + 1] = r.scale * N[k];
        world[4 * k + 2] = r.scale * Bn;
        world[4 * k + 3] = P[k];
    }
    world[12] = 0.0; world[13] = 0.0; world[14] = 0.0; world[15] = 1.0;
}

// ------------------------------------------------------------------ spacing
// A SPACED scatter has a minimum distance r > 0 and M >= count candidates.  Candidate j is, bit for bit, instance j of the
// selection above; its position P_j is mpt_scatter_point_of on the surface as it stands.  j and k CONFLICT iff
// d2 = ((dx dx) + (dy dy)) + (dz dz) < r2 = r r: a distance of exactly r is allowed, and a coordinate that is not finite makes the
// comparison false, so such a point conflicts with nothing.  In candidate order, j is KEPT iff no kept k < j conflicts with it
// (the greedy pass, the lexicographically first maximal independent set); the instances are the first `count` kept candidates.
enum { MPT_SPACE_UNDECIDED = 0, MPT_SPACE_KEPT = 1, MPT_SPACE_REJECTED = 2 };
enum : int64_t { MPT_SPACE_MAX_CANDIDATES = (int64_t)1 << 24 };

MPT_HD bool mpt_scatter_conflict(const double a[3], const double b[3], double r2) {
    MPT_NO_CONTRACT
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
    return d2 < r2;
}

// What an undecided candidate makes of one look at its conflicting lower neighbours' states (a round of the device): any kept ->
// rejected; else none undecided -> kept; else it waits.  States only move from undecided to their final value, and the lowest
// undecided candidate always decides, so rounds in any interleaving end in the greedy set
MPT_HD int mpt_scatter_space_decide(bool any_kept, bool any_undecided) {
    return any_kept ? MPT_SPACE_REJECTED : any_undecided ? MPT_SPACE_UNDECIDED : MPT_SPACE_KEPT;
}

// The elimination over pos [n][3] on the host: kept [n] (1 or 0) by the greedy pass, and the number of rounds the SYNCHRONOUS form
// of the rounds takes (every candidate reads the states the round before left): candidate j decides in round t(j) -- a rejected one
// in the round after the first of its conflicting kept lower neighbours was kept, a kept one in the round after the last of its
// conflicting lower neighbours decided (round 1 without any) -- and the count is the largest t.  All pairs are looked at: n^2 / 2
// tests, for tests and tools.  t [n] is the caller's scratch.
inline int32_t mpt_scatter_space_of(const double *pos, int64_t n, double r, uint8_t *kept, int32_t *t) {
    MPT_NO_CONTRACT
    const double r2 = r * r;
    int32_t rounds = 0;
    for (int64_t j = 0; j < n; j++) {
        int32_t first_kept = 0, last = 0;
        for (int64_t k = 0; k < j; k++) {
            if (!mpt_scatter_conflict(pos + 3 * j, pos + 3 * k, r2)) continue;
            if (kept[k] && (first_kept == 0 || t[k] < first_kept)) first_kept = t[k];
            if (t[k] > last) last = t[k];
        }
        kept[j] = first_kept == 0;
        t[j] = (first_kept ? first_kept : last) + 1;
        if (t[j] > rounds) rounds = t[j];
    }
    return rounds;
}

// ------------------------------------------------------------------ the device's search structure (no part of the rule)
// A uniform grid over the box [lo, hi] of the finite positions, so that a candidate looks at the 27 cells around its own instead of
// at everybody.  (scatter_space.hip's header has the argument that no conflicting pair is missed.)
//   edge: h = max(r (1 + 2^-20), 2^-20 times the largest extent, 2^-1000) -- a hair above r, at most 2^20 cells along an axis so that
//     cell coordinates are small exact integers whatever the extent, and well inside the normal numbers.  A box whose extent is not
//     finite has h = +inf and the one cell 0: every pair is tested
//   cell: c(x) = (int) floor((x - lo) / h), each operation rounded once: a monotone function of x, 0 at lo
MPT_HD double mpt_space_edge(double r, const double lo[3], const double hi[3]) {
    MPT_NO_CONTRACT
    double ext = 0.0;
    for (int k = 0; k < 3; k++) { const double e = hi[k] - lo[k]; if (!(e <= ext)) ext = e; }      // (NaN or +inf takes it)
    double h = r * (1.0 + 0x1p-20);
    const double he = ext * 0x1p-20;
    if (!(he <= h)) h = he;
    if (!(h >= 0x1p-1000)) h = 0x1p-1000;
    return std::isfinite(h) ? h : INFINITY;
}
MPT_HD int32_t mpt_space_cell(double x, double lo, double h) {
    MPT_NO_CONTRACT
    if (!(h < INFINITY)) return 0;
    const double u = std::floor((x - lo) / h);
    return u >= 0.0 ? (u <= 0x1p21 ? (int32_t)u : (int32_t)0x1p21) : 0;                           // (finite x in [lo, hi]: 0 <= u <= 2^20 + 1)
}
// the bucket of cell (cx, cy, cz), each below 2^21 + 1: SplitMix64's finaliser over the packed coordinates
MPT_HD uint32_t mpt_space_bucket(int32_t cx, int32_t cy, int32_t cz, uint32_t mask) {
    return (uint32_t)mpt_scatter_mix((uint64_t)cx | (uint64_t)cy << 22 | (uint64_t)cz << 44) & mask;
}

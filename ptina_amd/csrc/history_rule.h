// history_rule.h -- the pure pieces of the film's reprojection (film_history.cpp, history_kernel.hip, history.hip; DESIGN.md
// section 3.18): when mpt_history_reproject is allowed, where a surface point of the new view lay in the kept view, and what one
// pixel of the new film takes from the old one.  Plain C++17 that a host compiler takes as it is (as refit_rule.h), so that a
// stand-alone program can run all of it under a sanitizer (tools/history_rule_check.cpp); under hipcc the same functions are the
// kernels' arithmetic.  The C ABI has the rule as mpt_history_allowed.
//
// Arithmetic: f32, one correctly rounded operation per operator, never contracted, so that tests/reproject_ref.py restates the
// resampling bit for bit.  What keeps it so: the pragma below in every function that computes (a host compiler's own contraction),
// -ffp-contract=off for history.hip, where mpt_history_pixel runs (the Makefile's rule, as for noise_pixel.h), and -- because
// history_kernel.hip's production build is compiled with -ffp-contract=fast, under which the backend fuses a product into a sum
// whatever a pragma says (measured: 11 v_pk_fma_f32 in mpt_history_project with the pragma alone, none with the helper) --
// mpt_rn_mul for every product of mpt_history_project that feeds a sum.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

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

// a * b rounded to f32 before anything else sees it: on the device the product passes through an empty asm statement, which costs
// no instruction and leaves the backend no multiply to fuse into the sum that follows
MPT_HD float mpt_rn_mul(float a, float b) {
    float r = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(r));
#endif
    return r;
}

// ------------------------------------------------------------------ the refusal rule
enum MptHistoryVerdict { MPT_HISTORY_OK = 0, MPT_HISTORY_NONE, MPT_HISTORY_SIZE, MPT_HISTORY_FACES, MPT_HISTORY_STALE_TREE,
                         MPT_HISTORY_MAX_HISTORY, MPT_HISTORY_DEPTH_TOL };

// May the film of nx x ny pixels, over a model of `nfaces` faces whose tree is valid or not, take over the history kept at
// kept_nx x kept_ny over kept_faces faces (have: there is one)?  A refusal writes its words to `why` (always terminated).
inline MptHistoryVerdict mpt_history_rule(int have, int kept_nx, int kept_ny, int nx, int ny, int kept_faces, int nfaces, int tree_valid,
                                          float max_history, float depth_tol, char *why, size_t why_size) {
    if (why && why_size) why[0] = 0;
    if (!have) {
        if (why && why_size) snprintf(why, why_size, "reproject: no history: call keep_history() first (a reproject spends it, drop_history() drops it)");
        return MPT_HISTORY_NONE;
    }
    if (nx != kept_nx || ny != kept_ny) {
        if (why && why_size) snprintf(why, why_size, "reproject: the film is %dx%d, the history was kept at %dx%d: call keep_history() again", nx, ny, kept_nx, kept_ny);
        return MPT_HISTORY_SIZE;
    }
    if (nfaces != kept_faces) {
        if (why && why_size) snprintf(why, why_size, "reproject: the model has %d faces, the history was kept for %d: call keep_history() again", nfaces, kept_faces);
        return MPT_HISTORY_FACES;
    }
    if (!tree_valid) {
        if (why && why_size) snprintf(why, why_size, "reproject: BVH not built for the model as it stands: call build_tree() or update_tree() first");
        return MPT_HISTORY_STALE_TREE;
    }
    if (!(max_history > 0.0f)) {                                   // (+inf passes; a NaN does not)
        if (why && why_size) snprintf(why, why_size, "reproject: max_history must be positive or +inf, got %g", (double)max_history);
        return MPT_HISTORY_MAX_HISTORY;
    }
    if (!(depth_tol > 0.0f) || !std::isfinite(depth_tol)) {
        if (why && why_size) snprintf(why, why_size, "reproject: depth_tol must be finite and positive, got %g", (double)depth_tol);
        return MPT_HISTORY_DEPTH_TOL;
    }
    return MPT_HISTORY_OK;
}

// ------------------------------------------------------------------ the motion record
// What the motion kernel leaves per pixel of the NEW view (mpt_history_motion of include/miptina.h, 20 bytes): the object its
// centre ray hits (-1: none), where that surface point lay in the kept view in pixel units (pixel q's centre is q), how far from
// the kept camera's ray origin it lay, and the flags.  Without a place in the kept view fx, fy and d_exp are NaN.
struct MptMotion { int32_t cur_id; float fx, fy, d_exp; int32_t flags; };
#ifndef MPT_MOTION_NONE                     // (include/miptina.h states the same three; this file stands without it)
#define MPT_MOTION_NONE       0
#define MPT_MOTION_STATIC     1
#define MPT_MOTION_BACKGROUND 2
#endif
static_assert(sizeof(MptMotion) == 20, "a motion record is five words");

// The point of barycentrics (u, v) on the KEPT triangle a, b, c, seen by the kept camera (w2v, v2w row-major as uploaded) on a film
// of nx x ny pixels.  false: behind that camera (clip.w <= 0, or no number).
MPT_HD bool mpt_history_project(const float a[3], const float b[3], const float c[3], float u, float v, const float *w2v, const float *v2w,
                                int nx, int ny, float *fx, float *fy, float *d_exp) {
    MPT_NO_CONTRACT
    const float w0 = (1.0f - u) - v;
    float P[3], clip[4];
    for (int k = 0; k < 3; k++) P[k] = (mpt_rn_mul(w0, a[k]) + mpt_rn_mul(u, b[k])) + mpt_rn_mul(v, c[k]);
    for (int k = 0; k < 4; k++)
        clip[k] = ((mpt_rn_mul(w2v[4 * k], P[0]) + mpt_rn_mul(w2v[4 * k + 1], P[1])) + mpt_rn_mul(w2v[4 * k + 2], P[2])) + w2v[4 * k + 3];
    if (!(clip[3] > 0.0f)) return false;
    const float x = clip[0] / clip[3], y = clip[1] / clip[3];
    *fx = mpt_rn_mul((x + 1.0f) * 0.5f, (float)nx) - 0.5f;
    *fy = mpt_rn_mul((y + 1.0f) * 0.5f, (float)ny) - 0.5f;
    // the kept camera's ray origin at (x, y): camera_generate's near-plane point (pt_device.h), with the kept matrix
    float o[4];
    for (int k = 0; k < 4; k++) o[k] = ((mpt_rn_mul(v2w[4 * k], x) + mpt_rn_mul(v2w[4 * k + 1], y)) - v2w[4 * k + 2]) + v2w[4 * k + 3];
    const float dx = P[0] - o[0] / o[3], dy = P[1] - o[1] / o[3], dz = P[2] - o[2] / o[3];
    *d_exp = sqrtf((mpt_rn_mul(dx, dx) + mpt_rn_mul(dy, dy)) + mpt_rn_mul(dz, dz));
    return true;
}

// ------------------------------------------------------------------ one pixel of the new film
// what became of a pixel, in the order of mpt_history_stats' counts (a static pixel that kept its history counts as kept as well)
enum MptHistoryOutcome { MPT_OUTCOME_KEPT = 0, MPT_OUTCOME_STATIC, MPT_OUTCOME_BACKGROUND_KEPT, MPT_OUTCOME_DISOCCLUDED, MPT_OUTCOME_OFFSCREEN,
                         MPT_OUTCOME_BACKGROUND_RESET, MPT_OUTCOMES };

// does a point at (fx, fy) have a tap of positive weight inside the film?  (false for NaNs; inside, floorf(f) fits an int)
MPT_HD bool mpt_history_onscreen(float fx, float fy, int nx, int ny) { return fx > -1.0f && fx < (float)nx && fy > -1.0f && fy < (float)ny; }

// F_new(i, j) from the old accumulators f_old [nx * ny] (element x * ny + y; V4: four floats x, y, z, w), the kept G-buffer and
// the pixel's motion record: the four bilinear taps about (fx, fy), a outer and b inner, each used iff its weight is positive,
// it lies inside the film, it holds samples, the kept view saw the same object there and at the expected distance; the used taps
// renormalised; the sample count capped.  One 16-byte load per tap that passes the tests before it, no other access to f_old.
// The sums start from -0, the identity of IEEE addition, so that a single tap of weight 1 comes back word for word.
template <class V4>
MPT_HD MptHistoryOutcome mpt_history_pixel(const V4 *f_old, const int32_t *face_kept, const int32_t *id_kept, const float *depth_kept, int nx, int ny,
                                           int i, int j, const MptMotion &m, float max_history, float depth_tol, V4 *out) {
    MPT_NO_CONTRACT
    out->x = out->y = out->z = out->w = 0.0f;
    if (m.cur_id < 0) {                                             // the centre ray hits nothing
        if (m.flags == MPT_MOTION_BACKGROUND && face_kept[(size_t)i * ny + j] == -1) {
            const V4 f = f_old[(size_t)i * ny + j];
            if (f.w > 0.0f) {                                       // its own accumulators, capped like any other history
                *out = f;
                if (f.w > max_history) {
                    const float s = max_history / f.w;
                    out->x = f.x * s; out->y = f.y * s; out->z = f.z * s; out->w = f.w * s;
                }
                return MPT_OUTCOME_BACKGROUND_KEPT;
            }
        }
        return MPT_OUTCOME_BACKGROUND_RESET;
    }
    if (!mpt_history_onscreen(m.fx, m.fy, nx, ny)) return MPT_OUTCOME_OFFSCREEN;
    const float x0f = floorf(m.fx), y0f = floorf(m.fy);
    const float tx = m.fx - x0f, ty = m.fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float tol = depth_tol * m.d_exp;
    float ax = -0.0f, ay = -0.0f, az = -0.0f, aw = -0.0f, bsum = -0.0f;
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            const float bw = (a ? tx : 1.0f - tx) * (b ? ty : 1.0f - ty);
            const int qx = x0 + a, qy = y0 + b;
            if (!(bw > 0.0f) || qx < 0 || qx >= nx || qy < 0 || qy >= ny) continue;
            const size_t q = (size_t)qx * ny + qy;
            if (id_kept[q] != m.cur_id) continue;
            if (!(fabsf(depth_kept[q] - m.d_exp) <= tol)) continue;
            const V4 f = f_old[q];
            if (!(f.w > 0.0f)) continue;
            ax = ax + bw * f.x; ay = ay + bw * f.y; az = az + bw * f.z; aw = aw + bw * f.w;
            bsum = bsum + bw;
        }
    if (!(bsum > 0.0f)) return MPT_OUTCOME_DISOCCLUDED;
    float rx = ax / bsum, ry = ay / bsum, rz = az / bsum, rw = aw / bsum;
    if (rw > max_history) {
        const float s = max_history / rw;
        rx = rx * s; ry = ry * s; rz = rz * s; rw = rw * s;
    }
    out->x = rx; out->y = ry; out->z = rz; out->w = rw;
    return m.flags == MPT_MOTION_STATIC ? MPT_OUTCOME_STATIC : MPT_OUTCOME_KEPT;
}

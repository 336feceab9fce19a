// anim_rule.h -- the rule of keyframe animation (summarised in include/miptina.h): the validation of a
// skeleton's and a clip's arrays, a binding's local time, a track at that time, a joint's local matrix, the hierarchy and the palette;
// and, at the end of the file, two clips blended on one object and an object moved as a whole by an object clip (section 3.17.2), and
// objects parented to objects and to joints (section 3.17.3).
// Plain C++17 with nothing of HIP and no context (as deform_rule.h and scatter_rule.h), so that a stand-alone program can run all of
// it under a sanitizer (tools/anim_rule_check.cpp); under hipcc the MPT_HD functions are anim.hip's arithmetic.  The C ABI has the
// whole evaluation of one object's pose as mpt_anim_rule and the validation of a clip as mpt_clip_check.
//
// Arithmetic: f64, one correctly rounded operation per operator in the order written, never contracted (the pragma below in every
// function that computes, for a host compiler; -ffp-contract=off for anim.hip, the Makefile's rule), so that tests/anim_ref.py
// restates every pose bit for bit -- except through the one branch of the slerp that calls acos and sin, the only library functions
// here: there host, device and numpy each have their own, and the tests hold them to a bound (tests/anim_ref.py, error_bound).
// Key times and values are f32 and widen exactly.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "mpt_types.h"         // MptAnimTrack, MPT_ANIM_*, MPT_DEFORM_MAX_* (plain structures and constants)
#include "compose_rule.h"      // MPT_HD, MPT_NO_CONTRACT

// ------------------------------------------------------------------ what may be a skeleton, what may be a clip
enum MptSkeletonVerdict { MPT_SKELETON_OK = 0, MPT_SKELETON_ARGS, MPT_SKELETON_NJOINTS, MPT_SKELETON_PARENT, MPT_SKELETON_NOT_FINITE, MPT_SKELETON_ZERO_ROTATION };
enum MptClipVerdict { MPT_CLIP_OK = 0, MPT_CLIP_ARGS, MPT_CLIP_KIND, MPT_CLIP_TARGET, MPT_CLIP_NO_TARGETS, MPT_CLIP_NKEYS, MPT_CLIP_TIME_NOT_FINITE,
                      MPT_CLIP_TIME_ORDER, MPT_CLIP_DUPLICATE, MPT_CLIP_ZERO_ROTATION, MPT_CLIP_VALUE_NOT_FINITE };

// the values of one key of a track: 3, 4, 3 or ntargets
MPT_HD int mpt_anim_components(int path, int ntargets) { return path == MPT_ANIM_R ? 4 : path == MPT_ANIM_W ? ntargets : 3; }
// ... and the floats a key holds of them: CUBICSPLINE keeps in-tangent, value, out-tangent
MPT_HD int mpt_anim_key_floats(int path, int interp, int ntargets) { return (interp == MPT_ANIM_CUBICSPLINE ? 3 : 1) * mpt_anim_components(path, ntargets); }

// May parents [njoints], rest [njoints][10] (translation3 rotation4 xyzw scale3) and inverse_bind [njoints][12] be a skeleton?  A
// refusal writes its words, which name the argument, to `why` (always terminated).
inline MptSkeletonVerdict mpt_skeleton_rule(int njoints, const int32_t *parents, const double *rest, const double *inverse_bind, char *why, size_t why_size) {
    auto say = [&](MptSkeletonVerdict v, const char *fmt, long long a, long long b) {
        if (why && why_size) snprintf(why, why_size, fmt, a, b);
        return v;
    };
    if (why && why_size) why[0] = 0;
    if (njoints < 1 || njoints > MPT_DEFORM_MAX_JOINTS) return say(MPT_SKELETON_NJOINTS, "skeleton: njoints %lld outside [1, %lld]", njoints, MPT_DEFORM_MAX_JOINTS);
    if (!parents || !rest || !inverse_bind) return say(MPT_SKELETON_ARGS, "skeleton: parents, rest and inverse_bind must hold %lld joints", njoints, 0);
    for (int j = 0; j < njoints; j++) {
        if (parents[j] < -1 || parents[j] >= j)
            return say(MPT_SKELETON_PARENT, "skeleton: parents[%lld] is %lld: parents come before their children (-1: a root)", j, parents[j]);
        for (int k = 0; k < MPT_ANIM_REST; k++)
            if (!std::isfinite(rest[(size_t)j * MPT_ANIM_REST + k])) return say(MPT_SKELETON_NOT_FINITE, "skeleton: rest[%lld][%lld] is not finite", j, k);
        for (int k = 0; k < 12; k++)
            if (!std::isfinite(inverse_bind[(size_t)j * 12 + k])) return say(MPT_SKELETON_NOT_FINITE, "skeleton: inverse_bind[%lld][%lld] is not finite", j, k);
        const double *q = rest + (size_t)j * MPT_ANIM_REST + 3;
        if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0) return say(MPT_SKELETON_ZERO_ROTATION, "skeleton: the rest rotation rest[%lld][3..6] is zero", j, 0);
    }
    return MPT_SKELETON_OK;
}

// depth[j] of every joint (a root: 0); returns the greatest.  The skeleton has passed mpt_skeleton_rule
inline int mpt_anim_depths(int njoints, const int32_t *parents, int32_t *depth) {
    int levels = 0;
    for (int j = 0; j < njoints; j++) {
        depth[j] = parents[j] < 0 ? 0 : depth[parents[j]] + 1;
        if (depth[j] > levels) levels = depth[j];
    }
    return levels;
}

// May spec [ntracks][4] (target, path, interpolation, nkeys per track), times [ntimes] (the tracks' key times, back to back) and
// values [nvalues] (their values, back to back) be a clip of a mesh of njoints joints (0: no skeleton) and ntargets morph targets?
inline MptClipVerdict mpt_clip_rule(int njoints, int ntargets, int ntracks, const int32_t *spec, const float *times, int64_t ntimes, const float *values,
                                    int64_t nvalues, char *why, size_t why_size) {
    auto say = [&](MptClipVerdict v, const char *fmt, long long a, long long b, long long c) {
        if (why && why_size) snprintf(why, why_size, fmt, a, b, c);
        return v;
    };
    if (why && why_size) why[0] = 0;
    if (ntracks < 0 || ntimes < 0 || nvalues < 0 || (ntracks > 0 && !spec) || (ntimes > 0 && !times) || (nvalues > 0 && !values))
        return say(MPT_CLIP_ARGS, "clip: tracks must hold [%lld][4] words, times %lld and values %lld floats", ntracks, ntimes, nvalues);
    int64_t time_at = 0, value_at = 0;
    for (int r = 0; r < ntracks; r++) {
        const int target = spec[4 * r], path = spec[4 * r + 1], interp = spec[4 * r + 2], nkeys = spec[4 * r + 3];
        if (path < MPT_ANIM_T || path > MPT_ANIM_W) return say(MPT_CLIP_KIND, "clip: tracks[%lld] has path %lld (0 T, 1 R, 2 S, 3 W)", r, path, 0);
        if (interp < MPT_ANIM_STEP || interp > MPT_ANIM_CUBICSPLINE)
            return say(MPT_CLIP_KIND, "clip: tracks[%lld] has interpolation %lld (0 STEP, 1 LINEAR, 2 CUBICSPLINE)", r, interp, 0);
        if (path == MPT_ANIM_W) {
            if (ntargets < 1) return say(MPT_CLIP_NO_TARGETS, "clip: tracks[%lld] animates the morph weights of a mesh without morph targets", r, 0, 0);
            if (target != -1) return say(MPT_CLIP_TARGET, "clip: tracks[%lld] animates the morph weights: its target must be -1, not %lld", r, target, 0);
        } else if (target < 0 || target >= njoints)
            return say(MPT_CLIP_TARGET, "clip: tracks[%lld] names joint %lld, beyond njoints %lld", r, target, njoints);
        if (nkeys < 1) return say(MPT_CLIP_NKEYS, "clip: tracks[%lld] has %lld keys: at least 1", r, nkeys, 0);
        for (int q = 0; q < r; q++)
            if (spec[4 * q] == target && spec[4 * q + 1] == path)
                return say(MPT_CLIP_DUPLICATE, "clip: tracks[%lld] and tracks[%lld] animate the same target and path", q, r, 0);
        const int64_t kf = mpt_anim_key_floats(path, interp, ntargets), floats = kf * nkeys;
        if (time_at + nkeys > ntimes || value_at + floats > nvalues)
            return say(MPT_CLIP_ARGS, "clip: times and values end before tracks[%lld] does (%lld times, %lld values)", r, ntimes, nvalues);
        for (int k = 0; k < nkeys; k++) {
            if (!std::isfinite(times[time_at + k])) return say(MPT_CLIP_TIME_NOT_FINITE, "clip: times[%lld] of tracks[%lld] is not finite", k, r, 0);
            if (k > 0 && !(times[time_at + k] > times[time_at + k - 1]))
                return say(MPT_CLIP_TIME_ORDER, "clip: times[%lld] of tracks[%lld] is not above the key before: key times must increase strictly", k, r, 0);
        }
        for (int64_t k = 0; k < floats; k++)
            if (!std::isfinite(values[value_at + k])) return say(MPT_CLIP_VALUE_NOT_FINITE, "clip: values[%lld] of tracks[%lld] is not finite", k, r, 0);
        if (path == MPT_ANIM_R)
            for (int k = 0; k < nkeys; k++) {
                const float *q = values + value_at + (int64_t)k * kf + (interp == MPT_ANIM_CUBICSPLINE ? 4 : 0);
                if (q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f)
                    return say(MPT_CLIP_ZERO_ROTATION, "clip: the rotation values of key %lld of tracks[%lld] are zero", k, r, 0);
            }
        time_at += nkeys; value_at += floats;
    }
    if (time_at != ntimes || value_at != nvalues)
        return say(MPT_CLIP_ARGS, "clip: the tracks hold %lld times and %lld values, not what was given", time_at, value_at, 0);
    return MPT_CLIP_OK;
}

// The tracks of a checked clip as the arenas hold them, with time_at / value_at counted from the clip's first time and value; the
// span [t0, t1]: the least first key to the greatest last key (0, 0 for a clip without tracks)
inline void mpt_anim_tracks(int ntargets, int ntracks, const int32_t *spec, const float *times, MptAnimTrack *tracks, double *t0, double *t1) {
    int64_t time_at = 0, value_at = 0;
    *t0 = *t1 = 0.0;
    for (int r = 0; r < ntracks; r++) {
        MptAnimTrack &tr = tracks[r];
        tr.target = spec[4 * r]; tr.path = spec[4 * r + 1]; tr.interp = spec[4 * r + 2]; tr.nkeys = spec[4 * r + 3];
        tr.time_at = time_at; tr.value_at = value_at;
        const double first = times[time_at], last = times[time_at + tr.nkeys - 1];
        if (r == 0 || first < *t0) *t0 = first;
        if (r == 0 || last > *t1) *t1 = last;
        time_at += tr.nkeys; value_at += (int64_t)mpt_anim_key_floats(tr.path, tr.interp, ntargets) * tr.nkeys;
    }
}

// ------------------------------------------------------------------ a binding's local time
// tau = (t - offset) * speed; with `loop` and t1 > t0 wrapped into the span: t0 + (x - floor(x / d) * d), x = tau - t0, d = t1 - t0.
// Otherwise left as it is: each track clamps for itself
MPT_HD double mpt_anim_local_time(double t, double offset, double speed, int loop, double t0, double t1) {
    MPT_NO_CONTRACT
    double tau = (t - offset) * speed;
    if (loop && t1 > t0) {
        const double x = tau - t0, d = t1 - t0;
        tau = t0 + (x - std::floor(x / d) * d);
    }
    return tau;
}

// ------------------------------------------------------------------ a track at tau
// Where tau lies among the key times T [nkeys].  Returns 0: at key *k itself (one key; tau at or before the first: key 0; at or behind
// the last: key nkeys - 1; a tau that is not a number counts as before the first); 1: between keys *k and *k + 1, *k the largest
// index with T[k] <= tau by binary search, *dt = T[k + 1] - T[k] and *u = (tau - T[k]) / dt
MPT_HD int mpt_anim_key(const float *T, int nkeys, double tau, int *k, double *dt, double *u) {
    MPT_NO_CONTRACT
    *k = 0;
    if (nkeys == 1 || !(tau > (double)T[0])) return 0;
    if (tau >= (double)T[nkeys - 1]) { *k = nkeys - 1; return 0; }
    int lo = 0, hi = nkeys - 1;                                   // T[lo] <= tau < T[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((double)T[mid] <= tau) lo = mid; else hi = mid;
    }
    *k = lo;
    *dt = (double)T[lo + 1] - (double)T[lo];
    *u = (tau - (double)T[lo]) / *dt;
    return 1;
}

MPT_HD void mpt_anim_normalise4(double q[4]) {
    MPT_NO_CONTRACT
    const double len = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int c = 0; c < 4; c++) q[c] = q[c] / len;
}

// LINEAR between the rotations a and b (xyzw, used as given): the shorter arc; nlerp above d = 0.9995, the slerp with acos and sin
// -- the rule's only library functions -- below
MPT_HD void mpt_anim_slerp(const double a[4], const double b_in[4], double u, double q[4]) {
    MPT_NO_CONTRACT
    double b[4] = { b_in[0], b_in[1], b_in[2], b_in[3] };
    double d = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3];
    if (d < 0.0) {
        for (int c = 0; c < 4; c++) b[c] = -b[c];
        d = -d;
    }
    if (d > 0.9995) {
        for (int c = 0; c < 4; c++) q[c] = a[c] + u * (b[c] - a[c]);
        mpt_anim_normalise4(q);
        return;
    }
    const double theta = std::acos(d);
    const double sa = std::sin((1.0 - u) * theta), sb = std::sin(u * theta), s = std::sin(theta);
    for (int c = 0; c < 4; c++) q[c] = (sa * a[c] + sb * b[c]) / s;
}

// The C = mpt_anim_components values of track tr at tau, to out [C] (T, S, W: componentwise; R: a rotation xyzw).  times and values
// are the arenas the track's time_at and value_at count in.
//   at a key (mpt_anim_key 0), or STEP: the key's values
//   LINEAR: v0 + u * (v1 - v0) per component; R: mpt_anim_slerp
//   CUBICSPLINE, glTF's Hermite form with the tangents scaled by dt, b0 the out-tangent of key k and a1 the in-tangent of key k + 1:
//       u2 = u * u, u3 = u2 * u
//       h00 = (2 u3 - 3 u2) + 1,  h10 = (u3 - 2 u2) + u,  h01 = 3 u2 - 2 u3,  h11 = u3 - u2
//       p = ((h00 * v0 + (h10 * dt) * b0) + h01 * v1) + (h11 * dt) * a1          per component; R: normalised
MPT_HD void mpt_anim_sample(const MptAnimTrack &tr, const float *times, const float *values, int ntargets, double tau, double *out) {
    MPT_NO_CONTRACT
    const int C = mpt_anim_components(tr.path, ntargets);
    const bool cubic = tr.interp == MPT_ANIM_CUBICSPLINE;
    const int stride = cubic ? 3 * C : C;
    int k;
    double dt = 0.0, u = 0.0;
    const int between = mpt_anim_key(times + tr.time_at, tr.nkeys, tau, &k, &dt, &u);
    const float *v0 = values + tr.value_at + (int64_t)k * stride + (cubic ? C : 0);
    if (!between || tr.interp == MPT_ANIM_STEP) {
        for (int c = 0; c < C; c++) out[c] = (double)v0[c];
        return;
    }
    const float *v1 = v0 + stride;
    if (!cubic) {
        if (tr.path != MPT_ANIM_R) {
            for (int c = 0; c < C; c++) out[c] = (double)v0[c] + u * ((double)v1[c] - (double)v0[c]);
            return;
        }
        const double a[4] = { v0[0], v0[1], v0[2], v0[3] }, b[4] = { v1[0], v1[1], v1[2], v1[3] };
        double q[4];
        mpt_anim_slerp(a, b, u, q);
        for (int c = 0; c < 4; c++) out[c] = q[c];
        return;
    }
    const float *b0 = v0 + C, *a1 = v1 - C;
    const double u2 = u * u, u3 = u2 * u;
    const double h00 = (2.0 * u3 - 3.0 * u2) + 1.0, h10 = (u3 - 2.0 * u2) + u, h01 = 3.0 * u2 - 2.0 * u3, h11 = u3 - u2;
    const double g10 = h10 * dt, g11 = h11 * dt;
    if (tr.path != MPT_ANIM_R) {
        for (int c = 0; c < C; c++) out[c] = ((h00 * (double)v0[c] + g10 * (double)b0[c]) + h01 * (double)v1[c]) + g11 * (double)a1[c];
        return;
    }
    double q[4];
    for (int c = 0; c < 4; c++) q[c] = ((h00 * (double)v0[c] + g10 * (double)b0[c]) + h01 * (double)v1[c]) + g11 * (double)a1[c];
    mpt_anim_normalise4(q);
    for (int c = 0; c < 4; c++) out[c] = q[c];
}

// ------------------------------------------------------------------ a joint's local matrix, the hierarchy and the palette
// [R(q) diag(s) | t] as 3x4 row-major of trs = translation3 rotation4 (x y z w) scale3
MPT_HD void mpt_anim_local(const double *trs, double *M) {
    MPT_NO_CONTRACT
    const double x = trs[3], y = trs[4], z = trs[5], w = trs[6];
    const double R[9] = { 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
                          2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                          2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y) };
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) M[4 * r + c] = R[3 * r + c] * trs[7 + c];
        M[4 * r + 3] = trs[r];
    }
}

// C = A . B of affine 3x4 matrices, the bottom rows 0 0 0 1 implied; C may be A or B
MPT_HD void mpt_anim_mul(const double *A, const double *B, double *C) {
    MPT_NO_CONTRACT
    double out[12];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) out[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
        out[4 * r + 3] = ((A[4 * r] * B[3] + A[4 * r + 1] * B[7]) + A[4 * r + 2] * B[11]) + A[4 * r + 3];
    }
    for (int k = 0; k < 12; k++) C[k] = out[k];
}

// The pose of an object at local time tau: pose [ntargets + 12 njoints], the layout deform.hip reads -- the morph weights (0 without
// a W track), then palette[j] = global[j] . inverse_bind[j] with global[j] = local[j] for a root, else global[parent] . local[j], and
// local[j] by mpt_anim_local of the joint's T, R and S: its track at tau, else its rest value.  Skeleton and clip have passed their
// rules; tracks count their times and values from `times` and `values`
inline void mpt_anim_pose(int njoints, int ntargets, const int32_t *parents, const double *rest, const double *inverse_bind, int ntracks,
                          const MptAnimTrack *tracks, const float *times, const float *values, double tau, double *pose) {
    std::vector<double> trs(rest, rest + (size_t)njoints * MPT_ANIM_REST), global((size_t)njoints * 12);
    for (int t = 0; t < ntargets; t++) pose[t] = 0.0;
    for (int r = 0; r < ntracks; r++) {
        const MptAnimTrack &tr = tracks[r];
        static const int at[3] = { 0, 3, 7 };
        mpt_anim_sample(tr, times, values, ntargets, tau, tr.path == MPT_ANIM_W ? pose : trs.data() + (size_t)tr.target * MPT_ANIM_REST + at[tr.path]);
    }
    for (int j = 0; j < njoints; j++) {
        double *G = global.data() + (size_t)j * 12;
        mpt_anim_local(trs.data() + (size_t)j * MPT_ANIM_REST, G);
        if (parents[j] >= 0) mpt_anim_mul(global.data() + (size_t)parents[j] * 12, G, G);
        mpt_anim_mul(G, inverse_bind + (size_t)j * 12, pose + ntargets + (size_t)j * 12);
    }
}

// ================================================================== two clips blended, and an object moved by a clip
// ------------------------------------------------------------------ A. the second binding of a bound object
// The weight of the second binding at SCENE time t: with fade_duration > 0, x = (t - fade_start) / fade_duration and s = 0 below 0,
// 1 above 1, else x; with fade_duration == 0, s = 1 from fade_start on, else 0.  s == 0: w0 itself; s == 1: w1 itself; else
// w0 + s * (w1 - w0)
MPT_HD double mpt_anim_blend_weight(double t, double w0, double w1, double fade_start, double fade_duration) {
    MPT_NO_CONTRACT
    double s;
    if (fade_duration > 0.0) {
        const double x = (t - fade_start) / fade_duration;
        s = x < 0.0 ? 0.0 : x > 1.0 ? 1.0 : x;
    } else
        s = t >= fade_start ? 1.0 : 0.0;
    if (s == 0.0) return w0;
    if (s == 1.0) return w1;
    return w0 + s * (w1 - w0);
}

// n values of T, S or W: a + w * (b - a) per component, into a
MPT_HD void mpt_anim_blend_values(double *a, const double *b, double w, int n) {
    MPT_NO_CONTRACT
    for (int c = 0; c < n; c++) a[c] = a[c] + w * (b[c] - a[c]);
}

// R: the normalised lerp over the shorter arc, into a.  No library function
MPT_HD void mpt_anim_blend_rotation(double a[4], const double b_in[4], double w) {
    MPT_NO_CONTRACT
    double b[4] = { b_in[0], b_in[1], b_in[2], b_in[3] };
    const double d = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3];
    if (d < 0.0)
        for (int c = 0; c < 4; c++) b[c] = -b[c];
    for (int c = 0; c < 4; c++) a[c] = a[c] + w * (b[c] - a[c]);
    mpt_anim_normalise4(a);
}

// A joint's T R S of clip A (a [10]) and of clip B (b [10]) blended into a, 0 < w < 1 (at w == 0 the result is a and at w == 1 it is
// b, bit for bit: the callers copy)
MPT_HD void mpt_anim_blend_joint(double *a, const double *b, double w) {
    mpt_anim_blend_values(a, b, w, 3);
    mpt_anim_blend_rotation(a + 3, b + 3, w);
    mpt_anim_blend_values(a + 7, b + 7, w, 3);
}

// What may be a second binding
enum MptBlendVerdict { MPT_BLEND_OK = 0, MPT_BLEND_NOT_FINITE, MPT_BLEND_DURATION, MPT_BLEND_WEIGHT };
inline MptBlendVerdict mpt_blend_rule(double offset, double speed, double w0, double w1, double fade_start, double fade_duration, char *why, size_t why_size) {
    auto say = [&](MptBlendVerdict v, const char *words) {
        if (why && why_size) snprintf(why, why_size, "%s", words);
        return v;
    };
    if (why && why_size) why[0] = 0;
    if (!std::isfinite(offset)) return say(MPT_BLEND_NOT_FINITE, "offset is not finite");
    if (!std::isfinite(speed)) return say(MPT_BLEND_NOT_FINITE, "speed is not finite");
    if (!std::isfinite(fade_start)) return say(MPT_BLEND_NOT_FINITE, "fade_start is not finite");
    if (!std::isfinite(fade_duration)) return say(MPT_BLEND_NOT_FINITE, "fade_duration is not finite");
    if (fade_duration < 0.0) return say(MPT_BLEND_DURATION, "fade_duration is negative");
    if (!(w0 >= 0.0 && w0 <= 1.0)) return say(MPT_BLEND_WEIGHT, "w0 lies outside [0, 1]");
    if (!(w1 >= 0.0 && w1 <= 1.0)) return say(MPT_BLEND_WEIGHT, "w1 lies outside [0, 1]");
    return MPT_BLEND_OK;
}

// T R S [njoints][10] and the weights [ntargets] of one clip at tau: a track's values, else the rest value, 0 for the weights
inline void mpt_anim_sample_clip(int njoints, int ntargets, const double *rest, int ntracks, const MptAnimTrack *tracks, const float *times, const float *values,
                                 double tau, double *trs, double *weights) {
    for (size_t k = 0; k < (size_t)njoints * MPT_ANIM_REST; k++) trs[k] = rest[k];
    for (int t = 0; t < ntargets; t++) weights[t] = 0.0;
    for (int r = 0; r < ntracks; r++) {
        const MptAnimTrack &tr = tracks[r];
        static const int at[3] = { 0, 3, 7 };
        mpt_anim_sample(tr, times, values, ntargets, tau, tr.path == MPT_ANIM_W ? weights : trs + (size_t)tr.target * MPT_ANIM_REST + at[tr.path]);
    }
}

// The pose of an object with two bindings: clip A at tau_a and clip B at tau_b (each with its own tracks, times and values), blended by
// w, then the local matrices, the hierarchy and the palette exactly as mpt_anim_pose does them
inline void mpt_anim_pose_blend(int njoints, int ntargets, const int32_t *parents, const double *rest, const double *inverse_bind, int ntracks_a,
                                const MptAnimTrack *tracks_a, const float *times_a, const float *values_a, double tau_a, int ntracks_b,
                                const MptAnimTrack *tracks_b, const float *times_b, const float *values_b, double tau_b, double w, double *pose) {
    const size_t n = (size_t)njoints * MPT_ANIM_REST;
    std::vector<double> A(n), B(n), wb((size_t)ntargets), global((size_t)njoints * 12);
    mpt_anim_sample_clip(njoints, ntargets, rest, ntracks_a, tracks_a, times_a, values_a, tau_a, A.data(), pose);
    mpt_anim_sample_clip(njoints, ntargets, rest, ntracks_b, tracks_b, times_b, values_b, tau_b, B.data(), wb.data());
    if (w == 1.0) {
        A = B;
        for (int t = 0; t < ntargets; t++) pose[t] = wb[t];
    } else if (!(w == 0.0)) {
        for (int j = 0; j < njoints; j++) mpt_anim_blend_joint(A.data() + (size_t)j * MPT_ANIM_REST, B.data() + (size_t)j * MPT_ANIM_REST, w);
        mpt_anim_blend_values(pose, wb.data(), w, ntargets);
    }
    for (int j = 0; j < njoints; j++) {
        double *G = global.data() + (size_t)j * 12;
        mpt_anim_local(A.data() + (size_t)j * MPT_ANIM_REST, G);
        if (parents[j] >= 0) mpt_anim_mul(global.data() + (size_t)parents[j] * 12, G, G);
        mpt_anim_mul(G, inverse_bind + (size_t)j * 12, pose + ntargets + (size_t)j * 12);
    }
}

// ------------------------------------------------------------------ B. the motion of an object
// An OBJECT CLIP is a clip without a mesh: its tracks name target 0, the object's node, on the paths T, R and S (mpt_clip_rule with
// njoints 1 and ntargets 0, which refuses a W track).  A MOTION BINDING holds rest [10] (translation3 rotation4 xyzw scale3) and base
// [16] (row-major 4x4: the node's static parents)
enum MptMotionVerdict { MPT_MOTION_OK = 0, MPT_MOTION_REST_NOT_FINITE, MPT_MOTION_ZERO_ROTATION, MPT_MOTION_BASE_NOT_FINITE, MPT_MOTION_NOT_FINITE };
inline MptMotionVerdict mpt_motion_binding_rule(double offset, double speed, const double *rest, const double *base, char *why, size_t why_size) {
    auto say = [&](MptMotionVerdict v, const char *fmt, long long a) {
        if (why && why_size) snprintf(why, why_size, fmt, a);
        return v;
    };
    if (why && why_size) why[0] = 0;
    if (!std::isfinite(offset)) return say(MPT_MOTION_NOT_FINITE, "offset is not finite", 0);
    if (!std::isfinite(speed)) return say(MPT_MOTION_NOT_FINITE, "speed is not finite", 0);
    for (int k = 0; rest && k < MPT_ANIM_REST; k++)
        if (!std::isfinite(rest[k])) return say(MPT_MOTION_REST_NOT_FINITE, "rest[%lld] is not finite", k);
    if (rest && rest[3] == 0.0 && rest[4] == 0.0 && rest[5] == 0.0 && rest[6] == 0.0) return say(MPT_MOTION_ZERO_ROTATION, "the rest rotation rest[3..6] is zero", 0);
    for (int k = 0; base && k < 16; k++)
        if (!std::isfinite(base[k])) return say(MPT_MOTION_BASE_NOT_FINITE, "base[%lld] is not finite", k);
    return MPT_MOTION_OK;
}

// world = base . [L; 0 0 0 1] for a row-major 4x4 base and a 3x4 L, all four rows by the one expression:
//   W[r][c] = (B[r][0] L[0][c] + B[r][1] L[1][c]) + B[r][2] L[2][c], c < 3;  W[r][3] = ((B[r][0] L[0][3] + B[r][1] L[1][3]) + B[r][2] L[2][3]) + B[r][3]
MPT_HD void mpt_anim_world(const double *B, const double *L, double *W) {
    MPT_NO_CONTRACT
    for (int r = 0; r < 4; r++) {
        for (int c = 0; c < 3; c++) W[4 * r + c] = (B[4 * r] * L[c] + B[4 * r + 1] * L[4 + c]) + B[4 * r + 2] * L[8 + c];
        W[4 * r + 3] = ((B[4 * r] * L[3] + B[4 * r + 1] * L[7]) + B[4 * r + 2] * L[11]) + B[4 * r + 3];
    }
}

// The world matrix [16] of an object bound to an object clip, at local time tau: trs [10] starts as the binding's rest -- the caller
// has copied it there; it is the function's workspace, so that the device keeps it where a track's values can be written by index --
// and is overwritten by the clip's (at most three) tracks
MPT_HD void mpt_anim_motion(int ntracks, const MptAnimTrack *tracks, const float *times, const float *values, double tau, double *trs, const double *base,
                            double *world) {
    for (int r = 0; r < ntracks; r++) {
        const MptAnimTrack tr = tracks[r];
        mpt_anim_sample(tr, times, values, 0, tau, trs + (tr.path == MPT_ANIM_T ? 0 : tr.path == MPT_ANIM_R ? 3 : 7));
    }
    double L[12];
    mpt_anim_local(trs, L);
    mpt_anim_world(base, L, world);
}

// ================================================================== objects parented to objects and to joints
// A PARENT BINDING of an object is (parent, joint): another object of the table, and -1 or a joint of the skin of the parent's mesh.
// A bound object's own matrix -- what mpt_object_add / mpt_object_set_world gave, or base . T R S of its motion binding, exactly as
// mpt_anim_motion computes it -- is its LOCAL matrix, and
//   joint -1:  world(child) = world(parent) . local
//   joint j:   world(child) = world(parent) . ([M_j; 0 0 0 1] . local),  the inner product first
// with M_j the 3x4 entry j of the parent's pose as it lies in the pose buffer (the skinning matrix global . inverse bind: the child
// moves as a vertex skinned to j with weight 1 does).  Every product is mpt_mat4_mul; neither factor need be affine.

// W = A . B of row-major 4x4 matrices, W[r][c] = ((A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c]) + A[r][3] B[3][c]; W is
// neither A nor B
MPT_HD void mpt_mat4_mul(const double *A, const double *B, double *W) {
    MPT_NO_CONTRACT
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++)
            W[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
}

// world(child) [16] of world(parent) P [16], the palette entry M [12] (null: joint -1) and the child's local matrix L [16]
MPT_HD void mpt_hier_world(const double *P, const double *M, const double *L, double *world) {
    if (!M) { mpt_mat4_mul(P, L, world); return; }
    double M4[16], X[16];
    for (int k = 0; k < 12; k++) M4[k] = M[k];
    M4[12] = 0.0; M4[13] = 0.0; M4[14] = 0.0; M4[15] = 1.0;
    mpt_mat4_mul(M4, L, X);
    mpt_mat4_mul(P, X, world);
}

// May object `obj` of a table of nobj objects be bound to (parent, joint)?  parent_of(o): the bindings as they stand (-1: a root);
// instance_of(o): not 0 for an instance of a scatter; njoints_of(o): the joints of the skin of the object's mesh (0: no skin);
// childless: the caller knows that nothing is bound to obj, so that the search for the height of its subtree, the one step that
// looks at every object, is left out.  parent -1 unparents and is refused for an unknown object alone.  The numbers are the C ABI's
// (mpt_parent_check)
enum MptParentVerdict { MPT_PARENT_OK = 0, MPT_PARENT_UNKNOWN = 1, MPT_PARENT_CYCLE = 2, MPT_PARENT_INSTANCE = 3, MPT_PARENT_NO_SKIN = 4, MPT_PARENT_JOINT = 5,
                        MPT_PARENT_DEPTH = 6 };
template <class ParentOf, class InstanceOf, class JointsOf>
inline MptParentVerdict mpt_parent_rule_of(int nobj, ParentOf parent_of, InstanceOf instance_of, JointsOf njoints_of, bool childless, int obj, int parent, int joint,
                                           char *why, size_t why_size) {
    auto say = [&](MptParentVerdict v, const char *fmt, long long a, long long b) {
        if (why && why_size) snprintf(why, why_size, fmt, a, b);
        return v;
    };
    if (why && why_size) why[0] = 0;
    if (obj < 0 || obj >= nobj) return say(MPT_PARENT_UNKNOWN, "unknown object %lld (%lld objects)", obj, nobj);
    if (parent == -1) return MPT_PARENT_OK;
    if (parent < 0 || parent >= nobj) return say(MPT_PARENT_UNKNOWN, "unknown parent %lld (%lld objects)", parent, nobj);
    if (instance_of(obj)) return say(MPT_PARENT_INSTANCE, "object %lld is an instance of a scatter, which places it on its surface", obj, 0);
    if (instance_of(parent)) return say(MPT_PARENT_INSTANCE, "the parent, object %lld, is an instance of a scatter, whose matrix is written behind the hierarchy", parent, 0);
    int above = 0;                                                    // the parent's depth: its ancestors (the bindings as they stand have no cycle)
    for (int a = parent; a >= 0 && above <= nobj; a = parent_of(a), above++)
        if (a == obj) return say(MPT_PARENT_CYCLE, "object %lld would be its own ancestor through object %lld", obj, parent);
    above--;
    if (joint < -1) return say(MPT_PARENT_JOINT, "joint %lld: -1, or a joint of the parent's skin", joint, 0);
    if (joint >= 0 && njoints_of(parent) == 0) return say(MPT_PARENT_NO_SKIN, "joint %lld named, and the mesh of the parent, object %lld, has no skin", joint, parent);
    if (joint >= njoints_of(parent) && joint >= 0) return say(MPT_PARENT_JOINT, "joint %lld outside the %lld joints of the parent's skin", joint, njoints_of(parent));
    int below = 0;                                                    // the height of obj's own subtree
    for (int o = 0; o < nobj && !childless; o++) {
        int d = 0, a = o;
        while (a >= 0 && a != obj && d <= nobj) { a = parent_of(a); d++; }
        if (a == obj && d > below) below = d;
    }
    if (above + 1 + below > MPT_HIER_MAX_DEPTH)
        return say(MPT_PARENT_DEPTH, "the chain would be %lld deep: at most %lld", above + 1 + below, MPT_HIER_MAX_DEPTH);
    return MPT_PARENT_OK;
}

// ... over arrays: parents, instance and njoints [nobj]
inline MptParentVerdict mpt_parent_rule(int nobj, const int32_t *parents, const int32_t *instance, const int32_t *njoints, int obj, int parent, int joint,
                                        char *why, size_t why_size) {
    if (nobj < 0 || (nobj > 0 && (!parents || !instance || !njoints))) {
        if (why && why_size) snprintf(why, why_size, "parents, instance and njoints must hold %d objects", nobj);
        return MPT_PARENT_UNKNOWN;
    }
    return mpt_parent_rule_of(nobj, [&](int o) { return parents[o]; }, [&](int o) { return instance[o]; }, [&](int o) { return njoints[o]; }, false, obj, parent,
                              joint, why, why_size);
}

// The world matrix [16] of the last link of a chain of n links, link 0 the root, at scene time t.  Link k has local [16] -- its local
// matrix, or with ntracks[k] >= 0 the base of its motion binding (offset, speed, loop) = binding [k][3], rest [k][10], whose object
// clip's ntracks[k] tracks stand at tracks + track_at[k] and count their times and values from times[k] and values[k] -- and, for
// k > 0, pal[k]: null, or the twelve doubles of the palette entry it follows.  The arrays have passed mpt_hierarchy_rule's checks
struct MptHierLink {
    const double *local; int ntracks; const MptAnimTrack *tracks; const float *times, *values; double t0, t1;
    double offset, speed; int loop; const double *rest; const double *pal;
};
inline void mpt_hier_chain(int n, const MptHierLink *links, double t, double *world) {
    double W[16], L[16], trs[MPT_ANIM_REST];
    for (int k = 0; k < n; k++) {
        const MptHierLink &ln = links[k];
        if (ln.ntracks >= 0) {
            for (int i = 0; i < MPT_ANIM_REST; i++) trs[i] = ln.rest[i];
            mpt_anim_motion(ln.ntracks, ln.tracks, ln.times, ln.values, mpt_anim_local_time(t, ln.offset, ln.speed, ln.loop, ln.t0, ln.t1), trs, ln.local, L);
        } else
            for (int i = 0; i < 16; i++) L[i] = ln.local[i];
        if (k == 0) { for (int i = 0; i < 16; i++) world[i] = L[i]; continue; }
        for (int i = 0; i < 16; i++) W[i] = world[i];
        mpt_hier_world(W, ln.pal, L, world);
    }
}

// deform_rule.h -- the pure piece of mesh deformation's host side (scene_deform.cpp): the validation of a skin's arrays (the run
// table of a deform launch is run_table.h's).  Plain C++17 with nothing of HIP and no context (as refit_rule.h), so that a
// stand-alone program can run it under a sanitizer (tools/deform_rule_check.cpp); the C ABI has it as mpt_skin_check.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "mpt_types.h"          // MPT_DEFORM_* (plain structures and constants)

enum MptSkinVerdict { MPT_SKIN_OK = 0, MPT_SKIN_ARGS, MPT_SKIN_NJOINTS, MPT_SKIN_INDEX, MPT_SKIN_NOT_FINITE, MPT_SKIN_NEGATIVE };

// May joints [ncorners][4] and weights [ncorners][4] be the skin of a mesh over `njoints` joints?  A refusal writes its words,
// which name the argument, to `why` (always terminated).
inline MptSkinVerdict mpt_skin_rule(const uint16_t *joints, const float *weights, int64_t ncorners, int njoints, char *why, size_t why_size) {
    auto say = [&](MptSkinVerdict v, const char *fmt, long long a, long long b, long long c) {
        if (why && why_size) snprintf(why, why_size, fmt, a, b, c);
        return v;
    };
    if (why && why_size) why[0] = 0;
    if (ncorners < 0 || (ncorners > 0 && (!joints || !weights)))
        return say(MPT_SKIN_ARGS, "skin: joints and weights must hold [%lld][4] values", ncorners, 0, 0);
    if (njoints < 1 || njoints > MPT_DEFORM_MAX_JOINTS)
        return say(MPT_SKIN_NJOINTS, "skin: njoints %lld outside [1, %lld]", njoints, MPT_DEFORM_MAX_JOINTS, 0);
    for (int64_t k = 0; k < ncorners * 4; k++) {
        if (joints[k] >= njoints)
            return say(MPT_SKIN_INDEX, "skin: joints[%lld][%lld] names joint %lld, beyond njoints", k / 4, k % 4, joints[k]);
        if (!std::isfinite(weights[k]))
            return say(MPT_SKIN_NOT_FINITE, "skin: weights[%lld][%lld] is not finite", k / 4, k % 4, 0);
        if (weights[k] < 0.0f)
            return say(MPT_SKIN_NEGATIVE, "skin: weights[%lld][%lld] is negative", k / 4, k % 4, 0);
    }
    return MPT_SKIN_OK;
}

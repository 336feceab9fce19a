// displace_rule.h -- the pure piece of texture displacement's host side (scene_subdiv.cpp): the first-corner
// table of a level's vertices, which displace.hip reads a vertex's uv through, and the admission check of a mesh's corner uvs.
// Plain C++17 with nothing of HIP and no context (as subdiv_rule.h), so that a stand-alone program can run it under a sanitizer
// (tools/displace_rule_check.cpp); the C ABI has the table as mpt_displace_corners.  The definition it follows is stated in
// include/miptina.h and at the top of displace.hip.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#define MPT_DISPLACE_MAX_UV 1048576.0f      // 2^20: the largest magnitude of a corner uv a displaced mesh may carry

// corner[v], v < nverts: the lowest index 3 g + c into faces [nfaces][3] with faces[g][c] == v.  Returns 0, or 1 for arguments that
// name no table (a negative count, a null array that would be read or written, more than 2^31 - 1 corners), 2 for an id outside
// [0, nverts) (corner[0] then holds its index, where there is room), 3 for a vertex no face touches (corner[0] then holds the vertex)
inline int mpt_displace_corners_of(const int32_t *faces, int64_t nfaces, int32_t nverts, int32_t *corner) {
    if (nfaces < 0 || nverts < 0 || nfaces * 3 > 0x7fffffffLL || (nfaces > 0 && !faces) || (nverts > 0 && !corner)) return 1;
    for (int32_t v = 0; v < nverts; v++) corner[v] = -1;
    for (int64_t s = nfaces * 3 - 1; s >= 0; s--) {       // (downwards: the lowest index is written last)
        const int32_t v = faces[s];
        if (v < 0 || v >= nverts) { if (nverts > 0) corner[0] = (int32_t)s; return 2; }
        corner[v] = (int32_t)s;
    }
    for (int32_t v = 0; v < nverts; v++)
        if (corner[v] < 0) { corner[0] = v; return 3; }
    return 0;
}

// The uvs of the records verts [3k][8] (pos3 nrm3 uv2, f32) a displaced mesh may carry: every one finite and at most 2^20 in
// magnitude, so that the midpoints of admitted uvs are admitted and u * (nx - 1) stays far inside 64-bit integers.  Returns 0, or 1
// with the words, which name the corner, in why[why_size] (always terminated; may be null)
inline int mpt_displace_uv_check_of(const float *verts, int64_t k, char *why, size_t why_size) {
    if (why && why_size) why[0] = 0;
    if (k < 0 || (k > 0 && !verts)) {
        if (why && why_size) snprintf(why, why_size, "displacement: verts must hold [%lld][8] values", 3LL * (long long)k);
        return 1;
    }
    for (int64_t s = 0; s < k * 3; s++)
        for (int a = 6; a < 8; a++) {
            const float t = verts[(size_t)s * 8 + (size_t)a];
            if (std::isfinite(t) && std::fabs(t) <= MPT_DISPLACE_MAX_UV) continue;
            if (why && why_size)
                snprintf(why, why_size, "displacement: the uv of corner %lld of face %lld is not finite or exceeds 2^20 in magnitude", (long long)(s % 3),
                         (long long)(s / 3));
            return 1;
        }
    return 0;
}

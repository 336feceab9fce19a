// hit_point.h -- the production build's second evaluation of a closest hit, shared by the kernels that hand a hit's depth and
// barycentrics to a caller (query_kernel.hip, history_kernel.hip).  Included after path_common.h; the strict build has no use for it.
#pragma once

#if !MPT_STRICT
// Which triangle is hit, the walk decides; how far and where on it, the production build's answer evaluates once more for that one
// triangle: Moller-Trumbore in f64 over the vertex and edges of its reference-order record and the caller's ray AS GIVEN, its
// direction not normalised (u and v do not depend on its length; depth = t |d|).  The f32 normalisation alone turns a ray by up to
// 6e-8 rad, which at a grazing angle onto a sliver moves the hit's u and v in the fourth digit whatever arithmetic follows
// (measured on the 300-triangle test scene: 5.6e-4 by the walk's own f32 values, 4.5e-4 by f64 behind the f32 normalisation, 1e-4
// by the reference's Face.intersect, which on a model far from the origin is itself 1.2e-3 off: DESIGN.md 3.15) -- harmless to a
// path, not to a caller who asked for the point.  One 64-byte read and some seventy f64 operations per ray that hits.  The strict
// build reports the reference's own f32 numbers.  (det = -n . d, which the walk's test found to be at least MPT_EPS |d| in size.)
DEV void hit_point_f64(const MptVec4 *g, V3 ro, V3 rd_given, float *depth, float *u, float *v) {
    const MptVec4 g0 = g[0], g1 = g[1], g2 = g[2];
    const double e1[3] = { g1.x, g1.y, g1.z }, e2[3] = { g2.x, g2.y, g2.z }, d[3] = { rd_given.x, rd_given.y, rd_given.z };
    const double s[3] = { (double)ro.x - g0.x, (double)ro.y - g0.y, (double)ro.z - g0.z };
    const double px = d[1] * e2[2] - d[2] * e2[1], py = d[2] * e2[0] - d[0] * e2[2], pz = d[0] * e2[1] - d[1] * e2[0];
    const double qx = s[1] * e1[2] - s[2] * e1[1], qy = s[2] * e1[0] - s[0] * e1[2], qz = s[0] * e1[1] - s[1] * e1[0];
    const double inv = 1.0 / (e1[0] * px + e1[1] * py + e1[2] * pz);
    *u = (float)((s[0] * px + s[1] * py + s[2] * pz) * inv);
    *v = (float)((d[0] * qx + d[1] * qy + d[2] * qz) * inv);
    *depth = (float)((e2[0] * qx + e2[1] * qy + e2[2] * qz) * inv * sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
}
#endif

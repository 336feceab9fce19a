// subdiv.hip -- Loop subdivision on the device: a mesh of the pool that carries a subdivision level L gets a
// SUBDIVIDED COPY, an ordinary object-space mesh record [3 k 4^L][8] (pos3 nrm3 uv2, f32) that compose_kernel then reads as it reads
// any mesh.  It is evaluated behind morph targets and skinning (deform.hip) and before composition.
//
// The definition (also include/miptina.h).  All arithmetic is f64, every sum in the order written, without contraction
// (-ffp-contract=off, the Makefile's rule for this file); a value is rounded to f32 once, when a record is written.
//   Control vertices: corners whose f32 positions are equal as values (-0 equals +0) are one vertex; ids are ranks of first
//     appearance in corner order; a vertex's position is its FIRST corner's, widened to f64, read from the mesh or -- a mesh with
//     targets or a skin -- from the object's deformed copy.  A pose that pulls welded corners apart leaves the first corner
//     speaking for the vertex: no cracks.  The mesh's own normals are not used.
//   Level l -> l + 1: even vertices keep their ids 0 .. V_l - 1; the vertex of edge e is V_l + e, edges numbered in lexicographic
//     order of (lower endpoint id, higher endpoint id); face f = (v0, v1, v2) becomes faces 4f .. 4f + 3:
//     (v0, e01, e20), (v1, e12, e01), (v2, e20, e12), (e01, e12, e20).
//   Ring of a vertex: its neighbours in the order of the faces' winding (in face (v, a, b), a comes before b); an interior vertex's
//     ring starts at the neighbour with the lowest id, a boundary vertex's at the boundary neighbour that begins the fan.
//   Rules (a the lower endpoint id, b the higher; c opposite in the face that runs a -> b, d opposite in the other):
//     interior edge      (0.375 * (a + b)) + (0.125 * (c + d))
//     boundary edge      0.5 * (a + b)
//     interior vertex    (w * v) + (beta * s),  s = ((r_0 + r_1) + r_2) + ... the ring left to right,  n its length,
//                        beta = 0.1875 for n = 3, else 3.0 / (8.0 * n);  w = 1.0 - n * beta    (Warren's weights)
//     boundary vertex    (0.75 * v) + (0.125 * (p + q)),  p and q the first and the last of its ring.  There is no corner rule: a
//                        corner of an open mesh shrinks.
//   Normals, per vertex of the last level, on the unrounded positions: N = 0; for the vertex's faces (v, r_i, r_i+1) in ring order
//     (an interior ring closes, a boundary ring does not): A = r_i - v, B = r_i+1 - v,
//     N += (Ay Bz - Az By, Az Bx - Ax Bz, Ax By - Ay Bx);  nrm = N / sqrt((Nx Nx + Ny Ny) + Nz Nz).  A zero N gives NaN.  Every
//     corner on a vertex gets that vertex's normal: the surface is smooth.
//   Texcoords are face-varying: a child face takes its corners' uv from its parent's three corner uvs by the face rule above, the
//     midpoints m_ij = 0.5 * (u_i + u_j) in f64, level by level.
//
// Semi-sharp creases, corners and hard edges (also include/miptina.h).  Weld, ids, edge numbering, face
// split, uv rule and arithmetic are those of above; a mesh may state a sharpness per face edge and a flag per face corner.
//   Sharpness per level: an edge of cage sharpness s0 (f32 widened to f64; the larger of what its two faces state) has at level l
//     s_l = s0 - l if that is positive, else 0; inf stays inf.  Both halves of a split edge inherit s_{l+1}; the three edges new
//     inside a face have 0; a boundary edge counts as inf everywhere.  Corner flags pass to even vertices only.
//   Edge point (interior edge, sharpness s at the level below; E the interior rule above, H = 0.5 * (a + b)):
//     s == 0: E        s >= 1: H        otherwise ((1 - s) * E) + (s * H), componentwise.   A boundary edge keeps its rule.
//   Vertex point.  S: the sharpnesses > 0 of its incident edges in ring order from the ring's start, k = |S|, M the interior rule:
//     a flagged corner   v
//     k <= 1             M   (a dart's end included)
//     k == 2             p, q the far ends of the two sharp edges, C = (0.75 * v) + (0.125 * (p + q)), f = 0.5 * (s1 + s2):
//                        C if f >= 1, else ((1 - f) * M) + (f * C)
//     k >= 3             f = ((s1 + s2) + s3 + ...) / k:  v if f >= 1, else ((1 - f) * M) + (f * v)
//     Where f >= 1 the blend is not evaluated (no 0 * inf, no signed zeros).  A boundary vertex has k >= 2 with an inf in S: with
//     its two boundary edges alone it is the boundary rule above exactly; a crease that reaches the boundary makes it a corner.
//   Normals at the last level L: an edge is HARD if its sharpness at level L is > 0 (s0 > L, inf, or a boundary edge).  The hard
//     edges cut a vertex's fan into sectors; a corner of face (v, r_i, r_i+1) takes the normal sum above over the faces of its own
//     sector, in ring order from the sector's first hard edge.  A vertex without a hard interior edge keeps its single normal in
//     the order above; an interior vertex with one hard edge has one sector of all its faces, starting behind that edge.
//   A displacement (section 3.20) keeps taking its direction from the whole ring, so a creased surface does not crack; the sector
//     normals are then taken on the displaced positions.
// The host decides every case (subdiv_rule.h, which documents the words): the kernels see a rule's variant in its head, the blend's
// f or s as an f64 behind the rule's ids, and, for the last level of a creased mesh, one rule per RECORD -- a sector, an open ring
// as a boundary vertex's is, with its vertex's id in a table behind the rules -- which the face table then indexes.  An uncreased
// mesh has variant 0 everywhere and its vertices for records: the words and the results of before.
//
// Catmull-Clark subdivision of a cage of quads and polygons (also include/miptina.h), the second scheme a
// mesh may carry.  Arithmetic, weld, first-corner rule, ids of control vertices and edge numbering are those of above.  Polygon j of
// n_j corners (3 to 64) is stored as n_j - 2 consecutive triangles of the mesh, a fan about its first corner: (c_0, c_i+1, c_i+2).
//   Level l -> l + 1, ids: even vertices keep their ids; the edge point of edge e is V_l + e; the face point of face j is
//     V_l + E_l + j.
//   Face split: polygon or quad j of corners c_0 .. c_n-1 becomes n quads, quad i (c_i, e(c_i, c_i+1), f_j, e(c_i-1, c_i)); at level
//     1 the quads of polygon j start at the sum of n_j' over j' < j, from level 1 on quad q becomes 4q .. 4q + 3.  Windings are kept.
//   Emitted triangles: quad q = (v0, v1, v2, v3) of the last level is faces 2q (v0, v1, v2) and 2q + 1 (v0, v2, v3), so face g of an
//     object descends from level-1 quad (g >> 1) >> 2 (L - 1), and an object has 2 (sum n_j) 4^(L - 1) faces.
//   Face point         F = (((c_0 + c_1) + c_2) + ...) / n
//   interior edge      E = 0.25 * ((a + b) + (F1 + F2)),  a the lower endpoint id, b the higher, F1 the face that runs a -> b
//   boundary edge      0.5 * (a + b)
//   Ring of a vertex: its EDGE neighbours in winding order (in face (v, a, ..., b), a comes before b), the start as above.
//   interior vertex    M = (((n - 2.0) / n) * v) + ((1.0 / (n * n)) * (S_r + S_f)),  S_r the ring summed left to right, S_f the face
//                      points summed in the same order, F_i the face between r_i and r_i+1
//   boundary vertex    (0.75 * v) + (0.125 * (p + q)); no corner rule unless the corner is flagged.
//   A face point in an edge's or a vertex's rule is the value the face rule gives, bit for bit: the lane evaluates the face rule
//     again (sd_face_point) from the same words in the same order, so that face points need no launch of their own.
//   Creases and corners: the text of above with E and M as here; the edges new inside a face (edge point to face point) have
//     sharpness 0.  Normals at the last level: the sum of above over the ring of edge neighbours, one term per quad on the vertex,
//     cut into sectors by the hard edges as above; a displacement takes its direction from the whole ring.
//   Texcoords are face-varying: a face point's uv is ((u_0 + u_1) + ...) / n, an edge's 0.5 * (u_i + u_j); a child quad takes its uvs
//     by the split rule, level by level from the polygon's corner uvs -- c_0's and c_1's read from triangle 0 of the fan, c_i+2's
//     from corner 2 of triangle i (subdiv_walk.h: sd_quad_uv, through the mesh's table of level-1 quads).
// The rules that are Catmull-Clark's own carry MPT_SUBDIV_CC in their head's variant (subdiv_rule.h): the face point (its lane is
// item V_l + E_l + j of the refine launch), the interior edge, the interior vertex; a boundary vertex, a boundary or sharp edge, a
// vertex that stays and every rule of the last level are Loop's words, and the normal kernel does not know the scheme.  The job
// names the table of level-1 quads (rule_at[0]; 0: a Loop mesh), by which the record kernel and displace.hip pick the uv walk.
//
// Three kernels, each one lane per item (a workgroup of 256 lanes takes MPT_SUBDIV_CHUNK items of ONE job; a run table maps blocks to
// (job, chunk): run_table.h), so the number of launches of an mpt_compose is L_max + 2 whatever the
// number of copies; a job of fewer levels has no blocks in the later refine launches.  Levels are separate launches: nothing is
// handed from workgroup to workgroup inside a launch.
//   subdiv_refine_kernel   level l - 1 -> l: a lane reads its vertex's rule (two words), gathers 2 to n + 1 positions of the level
//                          below -- level 0 from the pool through the first-corner table, else 24-byte f64 records of the
//                          workspace -- and writes one.  (Catmull-Clark: the lanes are the vertices, the edges and then the faces
//                          of the level below; an interior vertex gathers its n neighbours and the corners of its n faces.)
//   subdiv_normal_kernel   the last level: a lane walks its vertex's ring (a creased mesh: its record's sector) and writes the record
//                          (pos3 nrm3 as f32: the one rounding), 32 bytes, two 16-byte stores.  The positions are those the job points at (npos_at): the
//                          last level's, or the displaced ones of a copy that carries a displacement (displace.hip, launched
//                          between the last refine level and this kernel; section 3.20).
//   subdiv_emit_kernel     a lane per refined face: three record ids, three 32-byte gathers (a vertex is shared by six corners, so
//                          they hit in L2), the parent's three uvs and L midpoint steps (a Catmull-Clark copy: its polygon's n uvs
//                          and L - 1 quad steps), six 16-byte stores: 96 bytes.
// Vector stores only, no atomics, no LDS.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "mpt_types.h"
#include "run_table.h"
#include "subdiv_walk.h"

enum { SD_BLOCK = MPT_SUBDIV_CHUNK };
static_assert(sizeof(MptSubdivJob) == 128, "the job record is 128 bytes");

// the position of vertex v of the level below `level`
static __device__ __forceinline__ SdVec sd_pos(const MptSubdivJob &o, int level, const float4 *pool, const int32_t *__restrict__ T,
                                               const double *work, int v) {
    if (level == 1) {
        const float4 q = pool[((size_t)o.src_vert + (size_t)T[v]) * 2];
        return { (double)q.x, (double)q.y, (double)q.z };
    }
    const double *p = work + o.work_at + o.pos_at[level - 1] + (size_t)v * 3;
    return { p[0], p[1], p[2] };
}

// Catmull-Clark: the point of the face whose rule is rule `id` of this launch, F = (((c_0 + c_1) + c_2) + ...) / n -- evaluated by every
// lane that needs it, the face's own lane included, so that it is one value bit for bit
static __device__ __forceinline__ SdVec sd_face_point(const MptSubdivJob &o, int level, const float4 *pool, const int32_t *__restrict__ T,
                                                      const double *work, int32_t id) {
    const int32_t head = T[o.rule_at[level] + 2 * id], at = T[o.rule_at[level] + 2 * id + 1];
    const int n = head >> 2 & MPT_SUBDIV_N_MASK;
    const int32_t *__restrict__ c = T + at;
    SdVec s = sd_add(sd_pos(o, level, pool, T, work, c[0]), sd_pos(o, level, pool, T, work, c[1]));
    for (int k = 2; k < n; k++) s = sd_add(s, sd_pos(o, level, pool, T, work, c[k]));
    const double nd = (double)n;
    return { s.x / nd, s.y / nd, s.z / nd };
}

// CC: the launch has a Catmull-Clark job.  One without is built without those rules -- Loop's kernel as it was, so that a scene of
// Loop meshes does not pay for their registers and code (DESIGN.md section 3.19.2 has the measurement)
template <bool CC>
__global__ __launch_bounds__(SD_BLOCK) void subdiv_refine_kernel(const float4 *pool, const MptSubdivJob *__restrict__ jobs,
                                                                 const MptRun *__restrict__ runs, int nruns, int level,
                                                                 const int32_t *__restrict__ topo, double *work) {
    const int r = mpt_run_of(runs, nruns);
    const MptSubdivJob &o = jobs[runs[r].item];          // (fields read through the scalar cache: a copy indexed by the level would live in scratch)
    const int i = ((int)blockIdx.x - runs[r].block) * SD_BLOCK + (int)threadIdx.x;
    if (i >= o.nv[level]) return;
    const int32_t *__restrict__ T = topo + o.topo_at;
    const int32_t head = T[o.rule_at[level] + 2 * i], at = T[o.rule_at[level] + 2 * i + 1];
    const int kind = head & 3, variant = head >> MPT_SUBDIV_VARIANT_SHIFT & 7, n = head >> 2 & MPT_SUBDIV_N_MASK;
    const int32_t *__restrict__ ring = T + at;
    SdVec out;
    if (CC && (variant & MPT_SUBDIV_CC)) {
        // Catmull-Clark's own rules (the boundary vertex, the boundary or sharp edge and the vertex that stays are the branches below)
        const int blend = variant & 3;
        if (kind == MPT_SUBDIV_EDGE_BND) {
            out = sd_face_point(o, level, pool, T, work, i);
        } else if (kind == MPT_SUBDIV_EDGE_INT) {
            const SdVec a = sd_pos(o, level, pool, T, work, ring[0]), b = sd_pos(o, level, pool, T, work, ring[1]);
            const SdVec F1 = sd_face_point(o, level, pool, T, work, ring[2]), F2 = sd_face_point(o, level, pool, T, work, ring[3]);
            out = sd_mul(0.25, sd_add(sd_add(a, b), sd_add(F1, F2)));
            if (blend == MPT_SUBDIV_BLEND_EDGE) {
                const double s = __hiloint2double(ring[5], ring[4]);
                out = sd_add(sd_mul(1.0 - s, out), sd_mul(s, sd_mul(0.5, sd_add(a, b))));
            }
        } else {
            const SdVec v = sd_pos(o, level, pool, T, work, i);
            SdVec sr = sd_pos(o, level, pool, T, work, ring[0]), sf = sd_face_point(o, level, pool, T, work, ring[n]);
            for (int k = 1; k < n; k++) {
                sr = sd_add(sr, sd_pos(o, level, pool, T, work, ring[k]));
                sf = sd_add(sf, sd_face_point(o, level, pool, T, work, ring[n + k]));
            }
            const double nd = (double)n;
            out = sd_add(sd_mul((nd - 2.0) / nd, v), sd_mul(1.0 / (nd * nd), sd_add(sr, sf)));
            if (blend == MPT_SUBDIV_BLEND_CREASE) {
                const SdVec p = sd_pos(o, level, pool, T, work, ring[2 * n]), q = sd_pos(o, level, pool, T, work, ring[2 * n + 1]);
                const double f = __hiloint2double(ring[2 * n + 3], ring[2 * n + 2]);
                const SdVec C = sd_add(sd_mul(0.75, v), sd_mul(0.125, sd_add(p, q)));
                out = sd_add(sd_mul(1.0 - f, out), sd_mul(f, C));
            } else if (blend == MPT_SUBDIV_BLEND_CORNER) {
                const double f = __hiloint2double(ring[2 * n + 1], ring[2 * n]);
                out = sd_add(sd_mul(1.0 - f, out), sd_mul(f, v));
            }
        }
    } else if (kind == MPT_SUBDIV_EDGE_INT) {
        const SdVec a = sd_pos(o, level, pool, T, work, ring[0]), b = sd_pos(o, level, pool, T, work, ring[1]);
        const SdVec c = sd_pos(o, level, pool, T, work, ring[2]), d = sd_pos(o, level, pool, T, work, ring[3]);
        out = sd_add(sd_mul(0.375, sd_add(a, b)), sd_mul(0.125, sd_add(c, d)));
        if (variant == MPT_SUBDIV_BLEND_EDGE) {
            const double s = __hiloint2double(ring[5], ring[4]);
            out = sd_add(sd_mul(1.0 - s, out), sd_mul(s, sd_mul(0.5, sd_add(a, b))));
        }
    } else if (kind == MPT_SUBDIV_EDGE_BND) {
        const SdVec a = sd_pos(o, level, pool, T, work, ring[0]), b = sd_pos(o, level, pool, T, work, ring[1]);
        out = sd_mul(0.5, sd_add(a, b));
    } else if (kind == MPT_SUBDIV_VERT_BND) {
        const SdVec v = sd_pos(o, level, pool, T, work, i);
        const SdVec p = sd_pos(o, level, pool, T, work, ring[0]), q = sd_pos(o, level, pool, T, work, ring[n - 1]);
        out = sd_add(sd_mul(0.75, v), sd_mul(0.125, sd_add(p, q)));
    } else if (variant == MPT_SUBDIV_FIXED) {
        out = sd_pos(o, level, pool, T, work, i);
    } else {
        const SdVec v = sd_pos(o, level, pool, T, work, i);
        SdVec s = sd_pos(o, level, pool, T, work, ring[0]);
        for (int k = 1; k < n; k++) s = sd_add(s, sd_pos(o, level, pool, T, work, ring[k]));
        const double beta = n == 3 ? 0.1875 : 3.0 / (8.0 * (double)n), w = 1.0 - (double)n * beta;
        out = sd_add(sd_mul(w, v), sd_mul(beta, s));
        if (variant == MPT_SUBDIV_BLEND_CREASE) {
            const SdVec p = sd_pos(o, level, pool, T, work, ring[n]), q = sd_pos(o, level, pool, T, work, ring[n + 1]);
            const double f = __hiloint2double(ring[n + 3], ring[n + 2]);
            const SdVec C = sd_add(sd_mul(0.75, v), sd_mul(0.125, sd_add(p, q)));
            out = sd_add(sd_mul(1.0 - f, out), sd_mul(f, C));
        } else if (variant == MPT_SUBDIV_BLEND_CORNER) {
            const double f = __hiloint2double(ring[n + 1], ring[n]);
            out = sd_add(sd_mul(1.0 - f, out), sd_mul(f, v));
        }
    }
    double *dst = work + o.work_at + o.pos_at[level] + (size_t)i * 3;
    dst[0] = out.x; dst[1] = out.y; dst[2] = out.z;
}

__global__ __launch_bounds__(SD_BLOCK) void subdiv_normal_kernel(const MptSubdivJob *__restrict__ jobs, const MptRun *__restrict__ runs,
                                                                 int nruns, const int32_t *__restrict__ topo, const double *work_in, double *work_out) {
    const int r = mpt_run_of(runs, nruns);
    const MptSubdivJob &o = jobs[runs[r].item];          // (fields read through the scalar cache: a copy indexed by the level would live in scratch)
    const int i = ((int)blockIdx.x - runs[r].block) * SD_BLOCK + (int)threadIdx.x;
    if (i >= o.nrec) return;
    const int32_t *__restrict__ T = topo + o.topo_at;
    const double *P = work_in + o.work_at + o.npos_at;       // (a displaced copy's normals are the displaced surface's: displace.hip)
    // record i is vertex i's; a creased mesh's record is a sector's, whose vertex stands in the table behind the sectors' rules
    const int32_t vert = o.srule_at == o.nrule_at ? i : T[o.srule_at + 2 * o.nrec + i];
    const SdVec v = sd_at(P, vert);
    const SdVec N = sd_ring_normal(T, o.srule_at, P, i, v);
    const double len = sqrt((N.x * N.x + N.y * N.y) + N.z * N.z);
    float4 *dst = (float4 *)(work_out + o.work_at + o.vrec_at) + (size_t)i * 2;
    dst[0] = make_float4((float)v.x, (float)v.y, (float)v.z, (float)(N.x / len));
    dst[1] = make_float4((float)(N.y / len), (float)(N.z / len), 0.0f, 0.0f);
}

__global__ __launch_bounds__(SD_BLOCK) void subdiv_emit_kernel(const float4 *pool_in, float4 *pool_out, const MptSubdivJob *__restrict__ jobs,
                                                               const MptRun *__restrict__ runs, int nruns, const int32_t *__restrict__ topo,
                                                               const double *__restrict__ work) {
    const int r = mpt_run_of(runs, nruns);
    const MptSubdivJob &o = jobs[runs[r].item];          // (fields read through the scalar cache: a copy indexed by the level would live in scratch)
    const int g = ((int)blockIdx.x - runs[r].block) * SD_BLOCK + (int)threadIdx.x;
    if (g >= o.nfaces) return;
    const int32_t *__restrict__ F = topo + o.topo_at + o.face_at + (size_t)g * 3;
    const float4 *__restrict__ vrec = (const float4 *)(work + o.work_at + o.vrec_at);
    const int32_t i0 = F[0], i1 = F[1], i2 = F[2];
    const float4 a0 = vrec[(size_t)i0 * 2], a1 = vrec[(size_t)i0 * 2 + 1];
    const float4 b0 = vrec[(size_t)i1 * 2], b1 = vrec[(size_t)i1 * 2 + 1];
    const float4 c0 = vrec[(size_t)i2 * 2], c1 = vrec[(size_t)i2 * 2 + 1];
    const SdFaceUv t = sd_copy_face_uv(pool_in, o, topo, g);
    const double u0 = t.u0, v0 = t.v0, u1 = t.u1, v1 = t.v1, u2 = t.u2, v2 = t.v2;
    float4 *dst = pool_out + ((size_t)o.dst_vert + (size_t)g * 3) * 2;
    dst[0] = a0; dst[1] = make_float4(a1.x, a1.y, (float)u0, (float)v0);
    dst[2] = b0; dst[3] = make_float4(b1.x, b1.y, (float)u1, (float)v1);
    dst[4] = c0; dst[5] = make_float4(c1.x, c1.y, (float)u2, (float)v2);
}

// ---------------------------------------------------------------- launchers
// runs[nruns] and blocks: mpt_subdiv_plan's table over the jobs' items of this launch and the sum of its blocks; cc: one of the
// launch's jobs is of a Catmull-Clark mesh.  The pool is read at the jobs' src_vert and written at their dst_vert, the workspace
// read at one level and written at the next: ranges that never overlap
MPT_KERNEL_API hipError_t mpt_launch_subdiv_refine(const float *pool, const MptSubdivJob *jobs, const MptRun *runs, int nruns, int blocks,
                                                   int level, int cc, const int32_t *topo, double *work, hipStream_t stream) {
    if (nruns < 1 || blocks < 1 || level < 1 || level > MPT_SUBDIV_MAX_LEVELS) return hipErrorInvalidValue;
    if (cc) hipLaunchKernelGGL(subdiv_refine_kernel<true>, dim3((unsigned)blocks), dim3(SD_BLOCK), 0, stream, (const float4 *)pool, jobs, runs, nruns, level, topo, work);
    else hipLaunchKernelGGL(subdiv_refine_kernel<false>, dim3((unsigned)blocks), dim3(SD_BLOCK), 0, stream, (const float4 *)pool, jobs, runs, nruns, level, topo, work);
    return hipGetLastError();
}

MPT_KERNEL_API hipError_t mpt_launch_subdiv_normals(const MptSubdivJob *jobs, const MptRun *runs, int nruns, int blocks, const int32_t *topo,
                                                    double *work, hipStream_t stream) {
    if (nruns < 1 || blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(subdiv_normal_kernel, dim3((unsigned)blocks), dim3(SD_BLOCK), 0, stream, jobs, runs, nruns, topo, (const double *)work, work);
    return hipGetLastError();
}

MPT_KERNEL_API hipError_t mpt_launch_subdiv_emit(float *pool, const MptSubdivJob *jobs, const MptRun *runs, int nruns, int blocks,
                                                 const int32_t *topo, const double *work, hipStream_t stream) {
    if (nruns < 1 || blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(subdiv_emit_kernel, dim3((unsigned)blocks), dim3(SD_BLOCK), 0, stream, (const float4 *)pool, (float4 *)pool, jobs, runs, nruns, topo,
                       work);
    return hipGetLastError();
}

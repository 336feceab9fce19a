// displace.hip -- texture displacement of a subdivided copy on the device: a subdivided mesh of the pool
// that carries a displacement has the vertices of its last level moved by an image of the image pool, between the last refine
// launch and the normals of subdiv.hip, so that the copy's normals are the displaced surface's.  Topology and face count stay as
// they are: a change of strength costs this launch, the normals, the records, the partial compose and a refit.
//
// The definition (also include/miptina.h).  All arithmetic is f64, every sum and product in the order written, without contraction
// (-ffp-contract=off, the Makefile's rule for this file); a value is rounded to f32 once, when a record is written (by subdiv.hip).
//   Vertex uv: the FIRST CORNER of a last-level vertex i is the lowest index 3 g + c into the last level's face table with
//     F[g][c] == i; the vertex's uv is that corner's face-varying uv as subdiv_emit_kernel derives it -- from the control records (the
//     mesh or the deformed copy), down the base-4 digits of g, midpoints 0.5 * (u_i + u_j), unrounded.  The first corner to touch a
//     vertex speaks for it (the rule of Blender's Displace modifier with UV coordinates, and of 3.19's weld): a uv seam cannot crack
//     the surface.
//   Height: the image [nx][ny] holds f32 rgba texels at base + x * ny + y, x and y wrapped by Python's modulo (the reference's
//     Image.subscript and Image.__call__, ptina/image.py:137-148).  px = u * (nx - 1), py = v * (ny - 1); fx = floor(px),
//     fy = floor(py), their integer parts 64-bit; x0 = px - fx, x1 = py - fy, y0 = 1 - x0, y1 = 1 - x1; per channel
//     t = (((t11 * x0) * x1 + (t10 * x0) * y1) + (t00 * y0) * y1) + (t01 * y0) * x1, texels widened to f64, t11 the texel at
//     (fx + 1, fy + 1), t10 at (fx + 1, fy), t00 at (fx, fy), t01 at (fx, fy + 1): the order of image_sample in pt_device.h.
//     Channel 0 to 3 picks r, g, b or a; channel 4 is ((r + g) + b) / 3.0.
//   MPT_DISPLACE_NORMAL: p' = p + (strength * (h - midlevel)) * n, n = N / sqrt((Nx Nx + Ny Ny) + Nz Nz) the unrounded smooth normal
//     of the UNDISPLACED last level by 3.19's normal rule; a zero N gives a NaN position.
//   MPT_DISPLACE_VECTOR: p' = p + strength * ((r, g, b) - midlevel), component by component in object space; the channel is ignored.
//   The copy's normals are 3.19's rule on p'; texcoords are untouched.
//
// One kernel, one lane per last-level vertex, a workgroup of 256 lanes taking MPT_SUBDIV_CHUNK vertices of ONE job (run_table.h), so
// that a compose with displaced copies costs one launch more whatever their number.  A lane walks its ring over the undisplaced
// positions (normal mode; the mode is uniform in a job, so in a wave), reads its first corner, walks that face's uvs down L digits,
// gathers four 16-byte texels and writes 24 bytes to an array of its own: its neighbours read the undisplaced positions, so the step
// cannot run in place.  Vector stores only, no atomics, no LDS.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/miptina.h"
#include "mpt_types.h"
#include "run_table.h"
#include "subdiv_walk.h"

enum { DP_BLOCK = MPT_SUBDIV_CHUNK };
static_assert(sizeof(MptDisplaceJob) == 48, "the displacement record is 48 bytes");

static __device__ __forceinline__ int64_t dp_pymod(int64_t a, int64_t b) { const int64_t r = a % b; return r < 0 ? r + b : r; }

__global__ __launch_bounds__(DP_BLOCK) void displace_kernel(const float4 *__restrict__ pool, const MptSubdivJob *__restrict__ jobs,
                                                            const MptDisplaceJob *__restrict__ djobs, const MptRun *__restrict__ runs, int nruns,
                                                            const int32_t *__restrict__ topo, const float4 *__restrict__ texels,
                                                            const double *work_in, double *work_out) {
    const int r = mpt_run_of(runs, nruns);
    const MptSubdivJob &o = jobs[runs[r].item];          // (fields read through the scalar cache: a copy indexed by the level would live in scratch)
    const MptDisplaceJob &q = djobs[runs[r].item];
    const int i = ((int)blockIdx.x - runs[r].block) * DP_BLOCK + (int)threadIdx.x;
    if (i >= o.nv[o.levels]) return;
    const double *P = work_in + o.work_at + o.pos_at[o.levels];
    const SdVec p = sd_at(P, i);
    // the height: the first corner's uv, then the four texels around it
    const int32_t corner = topo[q.corner_at + i];
    const int g = corner / 3, c = corner - 3 * g;
    const SdFaceUv t = sd_copy_face_uv(pool, o, topo, g);            // (by the mesh's scheme: a Catmull-Clark copy's quads, section 3.19.2)
    const double u = c == 0 ? t.u0 : c == 1 ? t.u1 : t.u2, v = c == 0 ? t.v0 : c == 1 ? t.v1 : t.v2;
    const double px = u * (double)(q.nx - 1), py = v * (double)(q.ny - 1);
    const double fx = floor(px), fy = floor(py);
    const int64_t ix = (int64_t)fx, iy = (int64_t)fy;
    const double x0 = px - fx, x1 = py - fy, y0 = 1.0 - x0, y1 = 1.0 - x1;
    const int64_t xa = dp_pymod(ix, q.nx) * q.ny, xb = dp_pymod(ix + 1, q.nx) * q.ny, ya = dp_pymod(iy, q.ny), yb = dp_pymod(iy + 1, q.ny);
    const float4 *__restrict__ I = texels + q.texel_at;
    const float4 t11 = I[xb + yb], t10 = I[xb + ya], t00 = I[xa + ya], t01 = I[xa + yb];
#define DP_MIX(k) ((((double)t11.k * x0) * x1 + ((double)t10.k * x0) * y1) + ((double)t00.k * y0) * y1) + ((double)t01.k * y0) * x1
    SdVec out;
    if (q.mode == MPT_DISPLACE_VECTOR) {
        const double hr = DP_MIX(x), hg = DP_MIX(y), hb = DP_MIX(z);
        out = { p.x + q.strength * (hr - q.midlevel), p.y + q.strength * (hg - q.midlevel), p.z + q.strength * (hb - q.midlevel) };
    } else {
        double h;
        if (q.channel == MPT_DISPLACE_MEAN) { const double hr = DP_MIX(x), hg = DP_MIX(y), hb = DP_MIX(z); h = ((hr + hg) + hb) / 3.0; }
        else if (q.channel == MPT_DISPLACE_R) h = DP_MIX(x);
        else if (q.channel == MPT_DISPLACE_G) h = DP_MIX(y);
        else if (q.channel == MPT_DISPLACE_B) h = DP_MIX(z);
        else h = DP_MIX(w);
        const SdVec N = sd_ring_normal(topo + o.topo_at, o.nrule_at, P, i, p);
        const double len = sqrt((N.x * N.x + N.y * N.y) + N.z * N.z);
        const double s = q.strength * (h - q.midlevel);
        out = { p.x + s * (N.x / len), p.y + s * (N.y / len), p.z + s * (N.z / len) };
    }
#undef DP_MIX
    double *dst = work_out + o.work_at + o.pos_at[0] + (size_t)i * 3;
    dst[0] = out.x; dst[1] = out.y; dst[2] = out.z;
}

// runs[nruns] and blocks: the plan over the dirty displaced jobs' last-level vertices; jobs and djobs are rows of the same copies.
// The workspace is read at the last level's positions and written at the displaced ones: ranges that never overlap
MPT_KERNEL_API hipError_t mpt_launch_displace(const float *pool, const MptSubdivJob *jobs, const MptDisplaceJob *djobs, const MptRun *runs, int nruns,
                                              int blocks, const int32_t *topo, const MptVec4 *texels, double *work, hipStream_t stream) {
    if (nruns < 1 || blocks < 1 || !texels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(displace_kernel, dim3((unsigned)blocks), dim3(DP_BLOCK), 0, stream, (const float4 *)pool, jobs, djobs, runs, nruns, topo,
                       (const float4 *)texels, (const double *)work, work);
    return hipGetLastError();
}

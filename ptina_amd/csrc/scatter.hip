// scatter.hip -- instances scattered over a surface of the object table on the device: an instance is born
// on a face of the surface object S, at a barycentric point, with a scale and a yaw, and remembers them (its STICKY RECORD); when S
// is posed, displaced or moved again the placement kernel alone runs again, inside mpt_compose, and writes the instances' world
// matrices into the device's object table, which compose_kernel reads next.  Instance and face counts stay as they are: the tree is refitted.
//
// The definition (also include/miptina.h; scatter_rule.h is its arithmetic, compose_rule.h the point rule it shares with compose.hip).
// All arithmetic is f64, every sum and product in the order written, without contraction (-ffp-contract=off, the Makefile's rule).
//   Draws: mix(z) is SplitMix64's finaliser (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
//     z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31, modulo 2^64); draw(i, k) = mix(mix(seed) + 16 i + k);
//     unit(i, k) = ((draw(i, k) >> 11) + 0.5) * 2^-53.
//   World points: corner c of face g of S is record 3 g + c of S's final object-space copy in the pool (what compose_kernel reads
//     for S), placed by S's world matrix W with compose_vertex's expressions: ph = (p, 1) . W^T, P = ph.xyz / ph.w, NOT rounded to f32.
//   Weights: area(g) = 0.5 * |cross(P1 - P0, P2 - P0)|; dens(g) = 1, or with a density image its channel sampled at the mean
//     ((u0 + u1) + u2) / 3.0 of the face's corner uvs by displace.hip's bilinear rule and channel codes, clamped to [0, 1], NaN
//     counting as 0; w(g) = area(g) * dens(g), 0 where that is not finite; wmax = the largest; q(g) = (uint32) floor(w(g) / wmax * 2^24).
//     A face below 2^-24 of the largest gets no instance.
//   Selection: cdf = the exclusive scan of q in u64, T = cdf[F]; t = draw(i, 0) mod T, g the largest face with cdf[g] <= t;
//     su = sqrt(unit(i, 1)), v = unit(i, 2), b1 = su * (1 - v), b2 = su * v, b0 = (1 - b1) - b2;
//     scale = smin + (smax - smin) * unit(i, 3); yaw: for j = 0..7, x = 2 unit(i, 4 + 2j) - 1, y = 2 unit(i, 5 + 2j) - 1, the first
//     pair with 2^-20 < x x + y y <= 1 gives (cy, sy) = (x, y) / sqrt(x x + y y); none, or random_yaw off: (1, 0).
//   Placement: P = (b0 P0 + b1 P1) + b2 P2; N = cross(P1 - P0, P2 - P0) / its length (align normal), or `up` at unit length;
//     s = copysign(1, N.z), a = -1 / (s + N.z), b = (N.x N.y) a, B0 = (1 + (s (N.x N.x)) a, s b, -(s N.x)),
//     T0 = (b, s + (N.y N.y) a, -N.y) (Duff et al.); Tn = cy T0 + sy B0, Bn = cy B0 - sy T0; the matrix has the columns scale Tn,
//     scale N, scale Bn, P and the bottom row 0 0 0 1.  A collapsed face gives NaN.
//
// Kernels, one lane per item, a workgroup of 256 lanes taking MPT_SCATTER_CHUNK items of ONE scatter (run_table.h), so that a compose
// costs one launch of each kind whatever the number of scatters:
//   scatter_weight_kernel   per face: w(g), and the workgroup's largest to part[block] (fmax: exact, order-free)
//   scatter_fold_kernel     one workgroup per scatter of the launch: wmax of its blocks' partials, also to the host's mapped record
//   scatter_scan_kernel     per face: q(g), the exclusive scan of the workgroup's q (wave shuffles, the waves' sums through LDS) and
//                           the workgroup's sum; scatter_sums_kernel, one workgroup per scatter, scans those sums and writes T;
//                           scatter_add_kernel adds a workgroup's offset back.  Integers: the result does not depend on the shape
//   scatter_select_kernel   per instance: the sticky record
//   scatter_place_kernel    per instance: world[16] as eight 16-byte stores, and the epoch, into the instance's row of the object table
// A SPACED scatter (a minimum distance; scatter_space.hip) has its M candidates drawn by scatter_select_kernel through a view of
// its job with count = M; the elimination between selection and placement leaves `count` of them as its sticky records.
// No atomics, vector stores only.  The job and the surface's row are uniform in a workgroup: they are read through the scalar cache.

#include <math.h>
#include "scatter_dev.h"

static_assert(sizeof(MptScatterJob) == 112 && sizeof(MptScatterPoint) == 48 && sizeof(MptComposeObj) == 160, "the records scatter.hip reads and writes");

__global__ __launch_bounds__(SC_BLOCK) void scatter_weight_kernel(const float4 *__restrict__ pool, const MptComposeObj *__restrict__ objs,
                                                                  const MptScatterJob *__restrict__ jobs, const MptRun *__restrict__ runs, int nruns,
                                                                  const float *__restrict__ texels, double *__restrict__ w, double *__restrict__ part) {
    __shared__ double s_max[SC_WAVES];
    const int r = mpt_run_of(runs, nruns);
    const MptScatterJob &o = jobs[runs[r].item];
    const MptComposeObj &S = objs[o.surf_obj];
    const int g = ((int)blockIdx.x - runs[r].block) * SC_BLOCK + (int)threadIdx.x;
    double wg = 0.0;
    if (g < o.nfaces) {
        double P[3][3];
        float uv[3][2];
        sc_corners(pool, S, g, P, o.density ? uv : nullptr);
        const double dens = o.density ? mpt_scatter_density(texels + o.texel_at * 4, o.nx, o.ny, o.channel, uv) : 1.0;
        wg = mpt_scatter_weight(P[0], P[1], P[2], dens);
        w[o.face_at + g] = wg;
    }
#pragma unroll
    for (int d = SC_WAVE / 2; d > 0; d >>= 1) wg = fmax(wg, __shfl_xor(wg, d, SC_WAVE));
    if (((int)threadIdx.x & (SC_WAVE - 1)) == 0) s_max[(int)threadIdx.x / SC_WAVE] = wg;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < SC_WAVES; k++) wg = fmax(wg, s_max[k]);
        part[blockIdx.x] = wg;
    }
}

__global__ __launch_bounds__(SC_BLOCK) void scatter_fold_kernel(const MptRun *__restrict__ runs, int nruns, int blocks, const double *__restrict__ part,
                                                                double *__restrict__ wmax, double *__restrict__ wmax_host) {
    __shared__ double s_max[SC_WAVES];
    const int r = (int)blockIdx.x;
    int b0, b1;
    sc_run_blocks(runs, nruns, blocks, r, &b0, &b1);
    double m = 0.0;
    for (int b = b0 + (int)threadIdx.x; b < b1; b += SC_BLOCK) m = fmax(m, part[b]);
#pragma unroll
    for (int d = SC_WAVE / 2; d > 0; d >>= 1) m = fmax(m, __shfl_xor(m, d, SC_WAVE));
    if (((int)threadIdx.x & (SC_WAVE - 1)) == 0) s_max[(int)threadIdx.x / SC_WAVE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < SC_WAVES; k++) m = fmax(m, s_max[k]);
        wmax[runs[r].item] = m;
        wmax_host[runs[r].item] = m;
    }
}

__global__ __launch_bounds__(SC_BLOCK) void scatter_scan_kernel(const MptScatterJob *__restrict__ jobs, const MptRun *__restrict__ runs, int nruns,
                                                                const double *__restrict__ w, const double *__restrict__ wmax,
                                                                uint32_t *__restrict__ q, uint64_t *__restrict__ cdf, uint64_t *__restrict__ bsum) {
    __shared__ uint64_t s_sum[SC_WAVES];
    const int r = mpt_run_of(runs, nruns);
    const MptScatterJob &o = jobs[runs[r].item];
    const int g = ((int)blockIdx.x - runs[r].block) * SC_BLOCK + (int)threadIdx.x;
    const bool in = g < o.nfaces;
    const uint32_t qg = in ? mpt_scatter_quantise(w[o.face_at + g], wmax[runs[r].item]) : 0u;
    uint64_t total;
    const uint64_t before = sc_block_scan(qg, s_sum, &total);
    if (in) { q[o.face_at + g] = qg; cdf[o.face_at + g] = before; }
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// bsum[b0 .. b1) of every run: the exclusive scan in place, 256 at a time with the sum so far carried along; T goes behind the run's cdf
__global__ __launch_bounds__(SC_BLOCK) void scatter_sums_kernel(const MptScatterJob *__restrict__ jobs, const MptRun *__restrict__ runs, int nruns, int blocks,
                                                                uint64_t *__restrict__ bsum, uint64_t *__restrict__ cdf) {
    __shared__ uint64_t s_sum[SC_WAVES];
    const int r = (int)blockIdx.x;
    const MptScatterJob &o = jobs[runs[r].item];
    int b0, b1;
    sc_run_blocks(runs, nruns, blocks, r, &b0, &b1);
    uint64_t carry = 0;
    for (int base = b0; base < b1; base += SC_BLOCK) {
        const int b = base + (int)threadIdx.x;
        const uint64_t x = b < b1 ? bsum[b] : 0;
        uint64_t total;
        const uint64_t before = sc_block_scan(x, s_sum, &total);
        if (b < b1) bsum[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) cdf[o.face_at + o.nfaces] = carry;
}

__global__ __launch_bounds__(SC_BLOCK) void scatter_add_kernel(const MptScatterJob *__restrict__ jobs, const MptRun *__restrict__ runs, int nruns,
                                                               const uint64_t *__restrict__ bsum, uint64_t *__restrict__ cdf) {
    const int r = mpt_run_of(runs, nruns);
    const MptScatterJob &o = jobs[runs[r].item];
    const int g = ((int)blockIdx.x - runs[r].block) * SC_BLOCK + (int)threadIdx.x;
    if (g < o.nfaces) cdf[o.face_at + g] += bsum[blockIdx.x];
}

__global__ __launch_bounds__(SC_BLOCK) void scatter_select_kernel(const MptScatterJob *__restrict__ jobs, const MptRun *__restrict__ runs, int nruns,
                                                                  const uint64_t *__restrict__ cdf, MptScatterPoint *__restrict__ points) {
    const int r = mpt_run_of(runs, nruns);
    const MptScatterJob &o = jobs[runs[r].item];
    const int i = ((int)blockIdx.x - runs[r].block) * SC_BLOCK + (int)threadIdx.x;
    if (i >= o.count) return;
    MptScatterPoint p;
    mpt_scatter_select(cdf + o.face_at, o.nfaces, o.key, (uint64_t)i, o.smin, o.smax, o.random_yaw, &p);
    points[o.point_at + i] = p;
}

// `surf` and `rows` are the one object table: the surface's row is read, the instances' rows are written (a surface is never an instance)
__global__ __launch_bounds__(SC_BLOCK) void scatter_place_kernel(const float4 *__restrict__ pool, const MptComposeObj *surf, MptComposeObj *rows,
                                                                 const MptScatterJob *__restrict__ jobs, const MptRun *__restrict__ runs, int nruns,
                                                                 const MptScatterPoint *__restrict__ points, unsigned epoch) {
    const int r = mpt_run_of(runs, nruns);
    const MptScatterJob &o = jobs[runs[r].item];
    const MptComposeObj &S = surf[o.surf_obj];
    const int i = ((int)blockIdx.x - runs[r].block) * SC_BLOCK + (int)threadIdx.x;
    if (i >= o.count) return;
    const MptScatterPoint p = points[o.point_at + i];
    double world[16];
    if ((unsigned)p.face < (unsigned)o.nfaces) {
        double P[3][3];
        sc_corners(pool, S, p.face, P, nullptr);
        mpt_scatter_place(P[0], P[1], P[2], p, o.align, o.up, world);
    } else {                                   // (a guard of the reads below: the records are the selection kernel's own)
        for (int k = 0; k < 16; k++) world[k] = NAN;
    }
    MptComposeObj *row = rows + o.first_obj + i;
    double2 *dst = (double2 *)row->world;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = make_double2(world[2 * k], world[2 * k + 1]);
    row->epoch = epoch;
}

// ---------------------------------------------------------------- launchers
// runs[nruns] and blocks: the plan over the selecting scatters' faces (run_table.h); part and bsum hold `blocks` entries; wmax
// and wmax_host a value per scatter of the table
MPT_KERNEL_API hipError_t mpt_launch_scatter_weights(const float *pool, const MptComposeObj *objs, const MptScatterJob *jobs, const MptRun *runs, int nruns,
                                                     int blocks, const MptVec4 *texels, double *w, double *part, double *wmax, double *wmax_host,
                                                     hipStream_t stream) {
    if (nruns < 1 || blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scatter_weight_kernel, dim3((unsigned)blocks), dim3(SC_BLOCK), 0, stream, (const float4 *)pool, objs, jobs, runs, nruns,
                       (const float *)texels, w, part);
    hipLaunchKernelGGL(scatter_fold_kernel, dim3((unsigned)nruns), dim3(SC_BLOCK), 0, stream, runs, nruns, blocks, (const double *)part, wmax, wmax_host);
    return hipGetLastError();
}

MPT_KERNEL_API hipError_t mpt_launch_scatter_scan(const MptScatterJob *jobs, const MptRun *runs, int nruns, int blocks, const double *w, const double *wmax,
                                                  uint32_t *q, uint64_t *cdf, uint64_t *bsum, hipStream_t stream) {
    if (nruns < 1 || blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scatter_scan_kernel, dim3((unsigned)blocks), dim3(SC_BLOCK), 0, stream, jobs, runs, nruns, w, wmax, q, cdf, bsum);
    hipLaunchKernelGGL(scatter_sums_kernel, dim3((unsigned)nruns), dim3(SC_BLOCK), 0, stream, jobs, runs, nruns, blocks, bsum, cdf);
    hipLaunchKernelGGL(scatter_add_kernel, dim3((unsigned)blocks), dim3(SC_BLOCK), 0, stream, jobs, runs, nruns, (const uint64_t *)bsum, cdf);
    return hipGetLastError();
}

// runs[nruns] and blocks: the plan over the scatters' instances
MPT_KERNEL_API hipError_t mpt_launch_scatter_select(const MptScatterJob *jobs, const MptRun *runs, int nruns, int blocks, const uint64_t *cdf,
                                                    MptScatterPoint *points, hipStream_t stream) {
    if (nruns < 1 || blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scatter_select_kernel, dim3((unsigned)blocks), dim3(SC_BLOCK), 0, stream, jobs, runs, nruns, cdf, points);
    return hipGetLastError();
}

MPT_KERNEL_API hipError_t mpt_launch_scatter_place(const float *pool, MptComposeObj *objs, const MptScatterJob *jobs, const MptRun *runs, int nruns,
                                                   int blocks, const MptScatterPoint *points, unsigned epoch, hipStream_t stream) {
    if (nruns < 1 || blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scatter_place_kernel, dim3((unsigned)blocks), dim3(SC_BLOCK), 0, stream, (const float4 *)pool, (const MptComposeObj *)objs, objs, jobs,
                       runs, nruns, points, epoch);
    return hipGetLastError();
}

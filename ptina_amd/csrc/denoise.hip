// denoise.hip -- edge-avoiding A-Trous wavelet filter of film pass 0, guided by the albedo and normal passes the PreviewEngine
// renders into passes 1 and 2 (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global
// Illumination Filtering", HPG 2010).  The reference renders those two passes as denoiser AOVs and leaves the filter to Blender's
// compositor; here it runs on the device.  The definition (include/miptina.h, mpt_get_denoised):
//
//   prologue   e_0 = (F0.rgb / F0.w) / m, valid = F0.w != 0;  a = F1.rgb / F1.w, n = F2.rgb / F2.w (0 where the pass is empty);
//              m = max(a, 1e-2) per channel when demodulating, else 1
//   iteration  i = 0 .. iterations - 1, s = 2^i: for every valid p, over the 25 taps q = p + s (dx, dy), dx outer, dy inner, both
//              ascending, skipping q outside the film or not valid:
//                  w = h[dx] h[dy] exp(-((|e(p) - e(q)|^2 kc + |a(p) - a(q)|^2 ka) + |n(p) - n(q)|^2 kn)),  |d|^2 = (dx dx + dy dy) + dz dz
//                  e'(p) = (sum w e(q)) / (sum w)
//   epilogue   (e m, 1) for valid pixels, FilmTable's empty marker otherwise
//
// All f32, compiled without contraction, a pure gather: the result repeats bit for bit, and the two stencil kernels below (tile in
// LDS for the strides 1 and 2, 16-byte gathers for the larger ones) run the same arithmetic in the same order, so which of them
// serves an iteration never changes a bit (option "denoise_lds"; tests/test_denoise_gpu.py).
//
// Variance guidance (mpt_denoise_set_variance; the definition is in include/miptina.h; the numpy
// restatement tests/denoise_var_ref.py): the prologue also reads the film's mark M and writes v_0, the squared standard error
// of e_0 from the two groups of samples the mark splits a pixel's into (noise.hip's estimate, in the filter's demodulated space);
// every iteration takes the colour tolerance of a pixel from a 3x3 prefilter g of v around it -- kc(p) = 1 / (sigma_variance^2 g(p)
// + 1e-10) in place of the global kc -- and carries the variance along: v'(p) = sum w^2 v(q) / (sum w)^2.  v is one float plane
// beside e, in two copies like e.  The stencil kernels are templated on the mode; the fixed instantiations (VAR = false) are the
// kernels as they were, operation for operation.
// Film element x * ny + y: lanes run along y, so every tap of a wave is one contiguous run of 64 float4.

#include <hip/hip_runtime.h>
#include <math.h>
#include "mpt_types.h"
#include "film_ops.h"

enum { DN_LANES = 64, DN_ROWS = 4, DN_TILE_X = 8 };     // a block is 64 lanes along y times 4 film columns; the LDS kernel's tile is 8 columns

__device__ __forceinline__ float dn_tap_weight(int d) {      // h = [1/16, 1/4, 3/8, 1/4, 1/16] at d = 0 .. 4 (all products exact in f32)
    return d == 2 ? 0.375f : ((d == 1 || d == 3) ? 0.25f : 0.0625f);
}

__device__ __forceinline__ float dn_dist2(const float4 p, const float4 q) {
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return (dx * dx + dy * dy) + dz * dz;
}

struct DnSum { float w, r, g, b; };

// one tap: `ok` = q lies in the film and is valid (e.w is the valid flag)
// (returns the tap's weight: the guided mode squares it for the variance)
__device__ __forceinline__ float dn_tap(DnSum &s, float hw, bool ok, const float4 ep, const float4 ap, const float4 np,
                                        const float4 eq, const float4 aq, const float4 nq, float kc, float ka, float kn) {
    const float arg = (dn_dist2(ep, eq) * kc + dn_dist2(ap, aq) * ka) + dn_dist2(np, nq) * kn;
    const float w = ok ? hw * expf(-arg) : 0.0f;
    s.w += w; s.r += w * eq.x; s.g += w * eq.y; s.b += w * eq.z;
    return w;
}

__device__ __forceinline__ float4 dn_finish(const DnSum s) {      // the centre tap alone gives s.w >= 9/64
    return make_float4(s.r / s.w, s.g / s.w, s.b / s.w, 1.0f);
}

// guided mode: the prefilter g of the variance plane, b = [1/4, 1/2, 1/4] at d = 0 .. 2 (products and their sums exact in f32) ...
struct DnPre { float num, den; };

__device__ __forceinline__ float dn_pre_weight(int d) { return d == 1 ? 0.5f : 0.25f; }

__device__ __forceinline__ void dn_pre_tap(DnPre &g, float bw, bool ok, float vq) {
    if (ok) { g.num += bw * vq; g.den += bw; }
}

// ... and the colour tolerance it gives the pixel (the centre tap alone gives g.den >= 1/4); sv2 = sigma_variance^2
__device__ __forceinline__ float dn_pre_kc(const DnPre g, float sv2) { return 1.0f / (sv2 * (g.num / g.den) + 1e-10f); }

// ---------------------------------------------------------------- prologue / epilogue: streaming passes like resolve_kernel
// VAR: also v_0 from the mark (x / 1 is x: without demodulation the division by m is left out)
template <bool VAR>
__global__ __launch_bounds__(256) void dn_prologue_kernel(const float4 *__restrict__ f0, const float4 *__restrict__ f1,
                                                          const float4 *__restrict__ f2, float4 *__restrict__ e,
                                                          float4 *__restrict__ a, float4 *__restrict__ n, size_t npix, int demodulate,
                                                          const float4 *__restrict__ mark, float *__restrict__ v) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npix) return;
    const float4 c = f0[t], g1 = f1[t], g2 = f2[t];
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f), nv = av, ev = av;
    if (g1.w != 0.0f) { av.x = g1.x / g1.w; av.y = g1.y / g1.w; av.z = g1.z / g1.w; }
    if (g2.w != 0.0f) { nv.x = g2.x / g2.w; nv.y = g2.y / g2.w; nv.z = g2.z / g2.w; }
    if (c.w != 0.0f) {
        ev.x = c.x / c.w; ev.y = c.y / c.w; ev.z = c.z / c.w; ev.w = 1.0f;
        if (demodulate) { ev.x = ev.x / fmaxf(av.x, 1e-2f); ev.y = ev.y / fmaxf(av.y, 1e-2f); ev.z = ev.z / fmaxf(av.z, 1e-2f); }
    }
    e[t] = ev; a[t] = av; n[t] = nv;
    if constexpr (VAR) {
        const float4 M = mark[t];
        const float nA = M.w, nB = c.w - nA;
        float v0 = 0.0f;
        if (c.w != 0.0f && nA > 0.0f && nB > 0.0f) {
            float dr = c.x / c.w - M.x / nA, dg = c.y / c.w - M.y / nA, db = c.z / c.w - M.z / nA;
            if (demodulate) { dr = dr / fmaxf(av.x, 1e-2f); dg = dg / fmaxf(av.y, 1e-2f); db = db / fmaxf(av.z, 1e-2f); }
            v0 = fminf(fmaxf(((dr * dr + dg * dg) + db * db) * (nA / nB), 0.0f), 3.0e38f);
        }
        v[t] = v0;
    }
}

__global__ __launch_bounds__(256) void dn_epilogue_kernel(const float4 *__restrict__ e, const float4 *__restrict__ a,
                                                          float4 *__restrict__ out, size_t npix, int demodulate) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npix) return;
    float4 v = e[t];
    if (v.w != 0.0f) {
        if (demodulate) {
            const float4 av = a[t];
            v.x = v.x * fmaxf(av.x, 1e-2f); v.y = v.y * fmaxf(av.y, 1e-2f); v.z = v.z * fmaxf(av.z, 1e-2f);
        }
        v.w = 1.0f;
    } else {
        v = make_float4(0.9f, 0.4f, 0.9f, 0.0f);               // FilmTable._get_image's empty pixel, filmtable.py:53-63
    }
    out[t] = v;
}

// ---------------------------------------------------------------- stencil, any stride: 75 coalesced 16-byte gathers per pixel
// Block b covers columns [4 (b / by), +4) and rows [64 (b % by), +64), by = blocks along y (a one-dimensional grid: a film may be
// wider than a grid's y extent allows).  VAR: kc arrives as sigma_variance^2 and becomes the pixel's own; 9 + 25 4-byte gathers
// of v_in more, and 9 of the valid flags around the centre.
template <bool VAR>
__global__ __launch_bounds__(256) void dn_atrous_gather_kernel(const float4 *__restrict__ e_in, float4 *__restrict__ e_out,
                                                               const float4 *__restrict__ a, const float4 *__restrict__ n,
                                                               int nx, int ny, int by, int s, float kc, float ka, float kn,
                                                               const float *__restrict__ v_in, float *__restrict__ v_out) {
    const int x = (int)(blockIdx.x / by) * DN_ROWS + (int)threadIdx.y;
    const int y = (int)(blockIdx.x % by) * DN_LANES + (int)threadIdx.x;
    if (x >= nx || y >= ny) return;
    const size_t p = (size_t)x * ny + y;
    const float4 ep = e_in[p];
    if (ep.w == 0.0f) {
        e_out[p] = ep;
        if constexpr (VAR) v_out[p] = 0.0f;
        return;
    }
    const float4 ap = a[p], np = n[p];
    DnSum sum = { 0.f, 0.f, 0.f, 0.f };
    float sum_v = 0.0f;
    if constexpr (VAR) {
        DnPre g = { 0.f, 0.f };
#pragma unroll
        for (int dx = 0; dx < 3; dx++) {
            const int qx = x + dx - 1;
#pragma unroll
            for (int dy = 0; dy < 3; dy++) {
                const int qy = y + dy - 1;
                const bool in = qx >= 0 && qx < nx && qy >= 0 && qy < ny;
                const size_t q = in ? (size_t)qx * ny + qy : p;
                dn_pre_tap(g, dn_pre_weight(dx) * dn_pre_weight(dy), in && e_in[q].w != 0.0f, v_in[q]);
            }
        }
        kc = dn_pre_kc(g, kc);
    }
#pragma unroll 1
    for (int dx = 0; dx < 5; dx++) {
        const int qx = x + (dx - 2) * s;
        const bool okx = qx >= 0 && qx < nx;
        const float hx = dn_tap_weight(dx);
#pragma unroll
        for (int dy = 0; dy < 5; dy++) {
            const int qy = y + (dy - 2) * s;
            const bool in = okx && qy >= 0 && qy < ny;
            const size_t q = in ? (size_t)qx * ny + qy : p;    // a tap outside the film reads the centre and weighs nothing
            const float4 eq = e_in[q], aq = a[q], nq = n[q];
            const float w = dn_tap(sum, hx * dn_tap_weight(dy), in && eq.w != 0.0f, ep, ap, np, eq, aq, nq, kc, ka, kn);
            if constexpr (VAR) sum_v += (w * w) * v_in[q];
        }
    }
    e_out[p] = dn_finish(sum);
    if constexpr (VAR) v_out[p] = sum_v / (sum.w * sum.w);
}

// ---------------------------------------------------------------- stencil, strides 1 and 2: the tile and its halo in LDS
// Tile: 8 columns x 64 rows; with the halo of 2 S on every side (8 + 4 S) x (64 + 4 S) records of e, a, n: 38 KiB at S = 1, 54 KiB at
// S = 2.  Lanes read consecutive 16-byte records (ds_read_b128 over a contiguous run: no bank conflict).  Records outside the film
// are written as zeros, whose valid flag is 0.  VAR: one float plane of v over the same tile and halo more (3.2 KiB, 4.5 KiB; the
// prefilter's reach of 1 lies inside the halo), kc as in the gather kernel.
template <int S, bool VAR>
__global__ __launch_bounds__(256) void dn_atrous_lds_kernel(const float4 *__restrict__ e_in, float4 *__restrict__ e_out,
                                                            const float4 *__restrict__ a, const float4 *__restrict__ n,
                                                            int nx, int ny, int by, float kc_in, float ka, float kn,
                                                            const float *__restrict__ v_in, float *__restrict__ v_out) {
    constexpr int R = 2 * S, W = DN_LANES + 2 * R, H = DN_TILE_X + 2 * R;
    __shared__ float4 se[H * W], sa[H * W], sn[H * W];
    __shared__ float sv[VAR ? H * W : 1];
    const int x0 = (int)(blockIdx.x / by) * DN_TILE_X, y0 = (int)(blockIdx.x % by) * DN_LANES;
    const int tid = (int)threadIdx.y * DN_LANES + (int)threadIdx.x;
    for (int t = tid; t < H * W; t += DN_LANES * DN_ROWS) {
        const int lx = t / W, ly = t - lx * W;
        const int gx = x0 - R + lx, gy = y0 - R + ly;
        float4 ev = make_float4(0.f, 0.f, 0.f, 0.f), av = ev, nv = ev;
        float vv = 0.0f;
        if (gx >= 0 && gx < nx && gy >= 0 && gy < ny) {
            const size_t q = (size_t)gx * ny + gy;
            ev = e_in[q]; av = a[q]; nv = n[q];
            if constexpr (VAR) vv = v_in[q];
        }
        se[t] = ev; sa[t] = av; sn[t] = nv;
        if constexpr (VAR) sv[t] = vv;
    }
    __syncthreads();
    const int y = y0 + (int)threadIdx.x;
    if (y >= ny) return;
#pragma unroll 1
    for (int k = 0; k < DN_TILE_X / DN_ROWS; k++) {
        const int lx = (int)threadIdx.y + DN_ROWS * k, x = x0 + lx;
        if (x >= nx) break;
        const size_t p = (size_t)x * ny + y;
        const int c = (lx + R) * W + (int)threadIdx.x + R;
        const float4 ep = se[c];
        if (ep.w == 0.0f) {
            e_out[p] = ep;
            if constexpr (VAR) v_out[p] = 0.0f;
            continue;
        }
        const float4 ap = sa[c], np = sn[c];
        DnSum sum = { 0.f, 0.f, 0.f, 0.f };
        float sum_v = 0.0f, kc = kc_in;
        if constexpr (VAR) {
            DnPre g = { 0.f, 0.f };
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
#pragma unroll
                for (int dy = 0; dy < 3; dy++) {
                    const int t = c + (dx - 1) * W + (dy - 1);
                    dn_pre_tap(g, dn_pre_weight(dx) * dn_pre_weight(dy), se[t].w != 0.0f, sv[t]);
                }
            }
            kc = dn_pre_kc(g, kc_in);
        }
#pragma unroll 1
        for (int dx = 0; dx < 5; dx++) {
            const float hx = dn_tap_weight(dx);
            const int row = c + (dx - 2) * S * W;
#pragma unroll
            for (int dy = 0; dy < 5; dy++) {
                const int t = row + (dy - 2) * S;
                const float4 eq = se[t], aq = sa[t], nq = sn[t];
                const float w = dn_tap(sum, hx * dn_tap_weight(dy), eq.w != 0.0f, ep, ap, np, eq, aq, nq, kc, ka, kn);
                if constexpr (VAR) sum_v += (w * w) * sv[t];
            }
        }
        e_out[p] = dn_finish(sum);
        if constexpr (VAR) v_out[p] = sum_v / (sum.w * sum.w);
    }
}

// ---------------------------------------------------------------- launchers
// mark and v: both null (the fixed filter) or both given (the guided one: v [npix] takes v_0)
MPT_KERNEL_API hipError_t mpt_launch_denoise_prologue(const MptVec4 *f0, const MptVec4 *f1, const MptVec4 *f2, MptVec4 *e, MptVec4 *a,
                                                      MptVec4 *n, size_t npix, int demodulate, const MptVec4 *mark, float *v,
                                                      hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    if ((mark == nullptr) != (v == nullptr)) return hipErrorInvalidValue;
    const int grid = (int)((npix + 255) / 256);
    if (v) hipLaunchKernelGGL(dn_prologue_kernel<true>, dim3(grid), dim3(256), 0, stream, (const float4 *)f0, (const float4 *)f1, (const float4 *)f2,
                              (float4 *)e, (float4 *)a, (float4 *)n, npix, demodulate, (const float4 *)mark, v);
    else hipLaunchKernelGGL(dn_prologue_kernel<false>, dim3(grid), dim3(256), 0, stream, (const float4 *)f0, (const float4 *)f1, (const float4 *)f2,
                            (float4 *)e, (float4 *)a, (float4 *)n, npix, demodulate, (const float4 *)nullptr, (float *)nullptr);
    return hipGetLastError();
}

template <bool VAR>
static hipError_t dn_launch_atrous(const float4 *ei, float4 *eo, const float4 *ap, const float4 *np, int nx, int ny, int s, float kc, float ka,
                                   float kn, int use_lds, const float *vi, float *vo, hipStream_t stream) {
    const int by = (ny + DN_LANES - 1) / DN_LANES;
    const dim3 block(DN_LANES, DN_ROWS);
    if (use_lds && s <= 2) {
        const long long blocks = (long long)((nx + DN_TILE_X - 1) / DN_TILE_X) * by;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidConfiguration;
        if (s == 1) hipLaunchKernelGGL((dn_atrous_lds_kernel<1, VAR>), dim3((unsigned)blocks), block, 0, stream, ei, eo, ap, np, nx, ny, by, kc, ka, kn, vi, vo);
        else hipLaunchKernelGGL((dn_atrous_lds_kernel<2, VAR>), dim3((unsigned)blocks), block, 0, stream, ei, eo, ap, np, nx, ny, by, kc, ka, kn, vi, vo);
    } else {
        const long long blocks = (long long)((nx + DN_ROWS - 1) / DN_ROWS) * by;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidConfiguration;
        hipLaunchKernelGGL(dn_atrous_gather_kernel<VAR>, dim3((unsigned)blocks), block, 0, stream, ei, eo, ap, np, nx, ny, by, s, kc, ka, kn, vi, vo);
    }
    return hipGetLastError();
}

// one iteration at stride s; use_lds: the strides 1 and 2 run the LDS kernel (same bits either way).  v_in and v_out: both null
// (the fixed filter: kc is the colour term's factor) or both given (the guided one: kc is sigma_variance^2, v_out takes v')
MPT_KERNEL_API hipError_t mpt_launch_denoise_atrous(const MptVec4 *e_in, MptVec4 *e_out, const MptVec4 *a, const MptVec4 *n, int nx, int ny,
                                                    int s, float kc, float ka, float kn, int use_lds, const float *v_in, float *v_out,
                                                    hipStream_t stream) {
    if (nx <= 0 || ny <= 0) return hipSuccess;
    if ((v_in == nullptr) != (v_out == nullptr)) return hipErrorInvalidValue;
    const float4 *ei = (const float4 *)e_in, *ap = (const float4 *)a, *np = (const float4 *)n;
    if (v_in) return dn_launch_atrous<true>(ei, (float4 *)e_out, ap, np, nx, ny, s, kc, ka, kn, use_lds, v_in, v_out, stream);
    return dn_launch_atrous<false>(ei, (float4 *)e_out, ap, np, nx, ny, s, kc, ka, kn, use_lds, nullptr, nullptr, stream);
}

MPT_KERNEL_API hipError_t mpt_launch_denoise_epilogue(const MptVec4 *e, const MptVec4 *a, MptVec4 *out, size_t npix, int demodulate,
                                                      hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    const int grid = (int)((npix + 255) / 256);
    hipLaunchKernelGGL(dn_epilogue_kernel, dim3(grid), dim3(256), 0, stream, (const float4 *)e, (const float4 *)a, (float4 *)out, npix, demodulate);
    return hipGetLastError();
}

// display.hip -- the film as a screen, a PNG or a viewport wants it: metered, tone-mapped, transfer-encoded, dithered and packed to
// 8-bit RGBA on the device (mpt_get_display; the definition is in include/miptina.h; the numpy restatement
// tests/display_ref.py).  The reference sketched the operator (ptina/wip/tonemapping.py:15-18) and never wired it in; its scripts clip
// linear radiance on the host.
//
//   metering    two launches, no float atomics.  Workgroup b of display_meter_kernel takes the film elements [4096 b, 4096 (b + 1)):
//               lane t adds log(1e-4 + Y) of the valid ones among 4096 b + t + 256 k, k = 0 .. 15 ascending, and the workgroup
//               leaves (sum, count).  ONE workgroup of display_expose_kernel then folds the partials and lane 0 writes the exposure.
//               Both stages are film_fold.h's, which says why the exposure, and with it every byte, repeats bit for bit.
//               The luminances are f32; their logarithms are taken and summed in f64 (free in a pass
//               that waits for memory: an f32 log's rounding does not average out over the film, it moved the exposure by two to
//               three f32 ulps), and the exposure is rounded to f32 once: the order of the sum moves it by 1e-16, far below an ulp.
//   conversion  one pass: sanitise, expose, operator, transfer, dither, pack, one 32-bit store per pixel.  The FILM layout streams
//               (element x ny + y in, the same element out).  The DISPLAY layout reads the film along y (16 bytes a lane, 256
//               contiguous bytes per column of a tile) and writes rows top-down along x (4 bytes a lane, 256 contiguous bytes per
//               row of a tile), the 64 x 16 tile of packed pixels turned in LDS.
//
// The source is an array of accumulators (rgb sums, weight): a film pass, or -- for the denoised source and the test door -- any
// array of that form; a resolved image (alpha 1 / marker rows with alpha 0) is such an array, and rgb / 1 is exact.
// All f32 except the metering's logarithms and sum, compiled without contraction.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/miptina.h"
#include "mpt_types.h"
#include "film_ops.h"
#include "film_fold.h"

enum { DP_BLOCK = FILM_FOLD_BLOCK, DP_PER_LANE = 16, DP_RUN = DP_BLOCK * DP_PER_LANE };   // metering: 4096 consecutive film elements per workgroup
enum { DP_TILE_X = 64, DP_TILE_Y = 16, DP_PITCH = DP_TILE_Y + 1 };            // DISPLAY layout: tile of packed pixels, rows padded by one word
static_assert(DP_TILE_X * DP_TILE_Y % DP_BLOCK == 0 && DP_BLOCK % DP_TILE_Y == 0 && DP_BLOCK % DP_TILE_X == 0, "tile and block");

#define DP_MARKER 0x00E666E6u          // the bytes (230, 102, 230, 0): get_image's empty pixel (0.9, 0.4, 0.9, 0) at 8 bits
#define DP_VMAX 1.0e18f                // exposed radiance is capped here: every operator has saturated long before, and v * v stays finite

__device__ __forceinline__ float dp_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__device__ __forceinline__ float dp_operator(float v, int op, float white2) {
    float t = v;                                                                   // MPT_TONE_LINEAR
    if (op == MPT_TONE_PTINA) t = v / (v + 0.155f) * 1.019f;                       // ptina/wip/tonemapping.py:15-18
    else if (op == MPT_TONE_REINHARD) t = v * (1.0f + v / white2) / (1.0f + v);
    else if (op == MPT_TONE_ACES) t = v * (2.51f * v + 0.03f) / (v * (2.43f * v + 0.59f) + 0.14f);
    return fminf(fmaxf(t, 0.0f), 1.0f);
}

__device__ __forceinline__ float dp_transfer(float t, int transfer, float inv_gamma) {
    if (transfer == MPT_TRANSFER_SRGB) return t <= 0.0031308f ? 12.92f * t : 1.055f * powf(t, 1.0f / 2.4f) - 0.055f;
    return powf(t, inv_gamma);
}

// the 8 x 8 Bayer index of (x & 7, y & 7); its 2 x 2 corner is [[0, 2], [3, 1]]
__device__ __forceinline__ int dp_bayer(int x, int y) {
    int m = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)
        m |= ((((x ^ y) >> i) & 1) << (2 * (2 - i) + 1)) | (((y >> i) & 1) << (2 * (2 - i)));
    return m;
}

__device__ __forceinline__ unsigned dp_quantise(float s, float bias) {
    return (unsigned)fminf(fmaxf(floorf(255.0f * s + bias), 0.0f), 255.0f);
}

// one pixel: accumulator -> packed RGBA8 (R in the low byte)
__device__ __forceinline__ unsigned dp_pixel(const float4 f, int x, int y, float E, const MptDisplayArgs a) {
    if (f.w == 0.0f) return DP_MARKER;
    const float bias = a.dither ? ((float)dp_bayer(x, y) + 0.5f) / 64.0f : 0.5f;
    const float c[3] = { f.x / f.w, f.y / f.w, f.z / f.w };
    unsigned px = 0xff000000u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float v = fminf(E * film_sanitise(c[k]), DP_VMAX);
        const float s = dp_transfer(dp_operator(v, a.op, a.white2), a.transfer, a.inv_gamma);
        px |= dp_quantise(s, bias) << (8 * k);
    }
    return px;
}

// ---------------------------------------------------------------- metering
struct DpAcc {                                            // a partial: the sum of the logarithms and the count of the pixels in it
    double sum, n;
    static __device__ __forceinline__ DpAcc zero() { return { 0.0, 0.0 }; }
    __device__ __forceinline__ void add(const DpAcc &o) { sum += o.sum; n += o.n; }
    __device__ __forceinline__ DpAcc across(int h) const { return { film_lane_xor(sum, h), film_lane_xor(n, h) }; }
};
static_assert(sizeof(DpAcc) == 2 * sizeof(double), "mpt_launch_display_meter's `part` holds two doubles per partial");

__global__ __launch_bounds__(DP_BLOCK) void display_meter_kernel(const float4 *__restrict__ src, size_t npix, DpAcc *__restrict__ part) {
    __shared__ DpAcc s_wave[FILM_FOLD_WAVES];
    const size_t base = (size_t)blockIdx.x * DP_RUN + threadIdx.x;
    DpAcc acc = DpAcc::zero();
#pragma unroll 4
    for (int k = 0; k < DP_PER_LANE; k++) {
        const size_t p = base + (size_t)k * DP_BLOCK;
        if (p < npix) {
            const float4 f = src[p];
            if (f.w != 0.0f) {
                const float Y = dp_luma(film_sanitise(f.x / f.w), film_sanitise(f.y / f.w), film_sanitise(f.z / f.w));
                acc.sum += log((double)(1e-4f + Y));
                acc.n += 1.0;
            }
        }
    }
    const DpAcc tot = film_block_fold(acc, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// E = key / exp(sum / N), 1 for a film without a valid pixel; to the device word the conversion reads and to the host's mapped word
__global__ __launch_bounds__(DP_BLOCK) void display_expose_kernel(const DpAcc *__restrict__ part, int nparts, float key,
                                                                  float *__restrict__ e_dev, float *__restrict__ e_host) {
    __shared__ DpAcc s_wave[FILM_FOLD_WAVES];
    const DpAcc tot = film_fold_parts(part, nparts, s_wave);
    if (threadIdx.x == 0) {
        const float E = tot.n > 0.0 ? (float)((double)key / exp(tot.sum / tot.n)) : 1.0f;
        *e_dev = E;
        *e_host = E;
    }
}

// ---------------------------------------------------------------- conversion
__global__ __launch_bounds__(256) void display_film_kernel(const float4 *__restrict__ src, unsigned *__restrict__ out, int nx, int ny,
                                                           const float *__restrict__ e_dev, MptDisplayArgs a) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)nx * ny) return;
    const float E = e_dev ? *e_dev : a.exposure;
    out[t] = dp_pixel(src[t], (int)(t / (size_t)ny), (int)(t % (size_t)ny), E, a);
}

// Block b covers film columns [64 (b / by), +64) and rows [16 (b % by), +16), by = tiles along y (a one-dimensional grid).  In: lane l
// of the 256 converts element (column (l >> 4) + 16 k, row l & 15), k = 0 .. 3 -- per wave four columns of 16 consecutive float4 --
// and leaves the packed pixel at tile[column][row].  Out: lane l stores tile[l & 63][(l >> 6) + 4 k] to image row ny - 1 - y -- per
// wave one row of 64 consecutive pixels.  Pitch 17 words: the 32 lanes of a read group fall on 32 different banks; a write group
// (two columns) meets itself on one bank, which a 4-byte LDS store does not pay for.
__global__ __launch_bounds__(DP_BLOCK) void display_transpose_kernel(const float4 *__restrict__ src, unsigned *__restrict__ out, int nx,
                                                                     int ny, int by, const float *__restrict__ e_dev, MptDisplayArgs a) {
    __shared__ unsigned tile[DP_TILE_X * DP_PITCH];
    const int x0 = (int)(blockIdx.x / by) * DP_TILE_X, y0 = (int)(blockIdx.x % by) * DP_TILE_Y;
    const int l = (int)threadIdx.x;
    const float E = e_dev ? *e_dev : a.exposure;
#pragma unroll
    for (int k = 0; k < DP_TILE_X * DP_TILE_Y / DP_BLOCK; k++) {
        const int lx = (l / DP_TILE_Y) + (DP_BLOCK / DP_TILE_Y) * k, ly = l % DP_TILE_Y;
        const int x = x0 + lx, y = y0 + ly;
        if (x < nx && y < ny) tile[lx * DP_PITCH + ly] = dp_pixel(src[(size_t)x * ny + y], x, y, E, a);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DP_TILE_X * DP_TILE_Y / DP_BLOCK; k++) {
        const int lx = l % DP_TILE_X, ly = (l / DP_TILE_X) + (DP_BLOCK / DP_TILE_X) * k;
        const int x = x0 + lx, y = y0 + ly;
        if (x < nx && y < ny) out[(size_t)(ny - 1 - y) * nx + x] = tile[lx * DP_PITCH + ly];
    }
}

// ---------------------------------------------------------------- launchers
MPT_KERNEL_API size_t mpt_display_parts(size_t npix) { return film_fold_count(npix, DP_RUN); }

// part: 2 * mpt_display_parts(npix) doubles
MPT_KERNEL_API hipError_t mpt_launch_display_meter(const MptVec4 *src, size_t npix, double *part, float key, float *e_dev, float *e_host,
                                                   hipStream_t stream) {
    unsigned nparts;
    if (const hipError_t e = film_fold_grid(npix, DP_RUN, &nparts)) return e;
    if (nparts) hipLaunchKernelGGL(display_meter_kernel, dim3(nparts), dim3(DP_BLOCK), 0, stream, (const float4 *)src, npix, (DpAcc *)part);
    hipLaunchKernelGGL(display_expose_kernel, dim3(1), dim3(DP_BLOCK), 0, stream, (const DpAcc *)part, (int)nparts, key, e_dev, e_host);
    return hipGetLastError();
}

// e_dev: the metered exposure on the device, or NULL for a->exposure
MPT_KERNEL_API hipError_t mpt_launch_display_convert(const MptVec4 *src, uint32_t *out, int nx, int ny, const MptDisplayArgs *a,
                                                     const float *e_dev, hipStream_t stream) {
    if (nx <= 0 || ny <= 0) return hipSuccess;
    if (a->layout == MPT_LAYOUT_DISPLAY) {
        const int by = (ny + DP_TILE_Y - 1) / DP_TILE_Y;
        const long long blocks = (long long)((nx + DP_TILE_X - 1) / DP_TILE_X) * by;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidConfiguration;
        hipLaunchKernelGGL(display_transpose_kernel, dim3((unsigned)blocks), dim3(DP_BLOCK), 0, stream, (const float4 *)src, (unsigned *)out,
                           nx, ny, by, e_dev, *a);
    } else {
        const size_t blocks = ((size_t)nx * ny + 255) / 256;
        if (blocks > 0x7fffffffULL) return hipErrorInvalidConfiguration;
        hipLaunchKernelGGL(display_film_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const float4 *)src, (unsigned *)out, nx, ny,
                           e_dev, *a);
    }
    return hipGetLastError();
}

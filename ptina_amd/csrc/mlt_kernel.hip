// mlt_kernel.hip -- the Metropolis path engine (MLTPathEngine, engine/mltpath.py): one chain per lane, K iterations of
// mutate -> path_trace -> splat record -> accept/reject per launch, and the deterministic splat pass that adds the records
// to film pass 0.
//
// Built twice from this one source like render_kernel.hip: MPT_STRICT=1 (StrictTracer, IEEE, the reference's traversal)
// and MPT_STRICT=0 (the gather tracer over the production binary tree, as the preview kernel walks it).  The path itself is
// path_common.h's, the PathEngine's.
//
// Randomness (the one deliberate deviation from the reference, whose ti.random() is a stateful generator): every draw is
// a stateless hash of (seed, chain, iteration, slot), nested 32-bit PCG hashes (O'Neill's pcg_hash):
//     pcg(v):  s = v * 747796405 + 2891336453;  w = ((s >> ((s >> 28) + 4)) ^ s) * 277803737;  return (w >> 22) ^ w
//     h = pcg(pcg(pcg(pcg(seed) + chain) + iteration) + slot)            (all u32, wrapping)
//     u = ((h >> 9) + 0.5) * 2^-23                                        in (0, 1), exact in f32
// Slots: 0 the large-step coin, 1 + j the uniform of dim j (a large step's value, or a small step's normaldist input),
// 33 the accept coin.  reset() draws X[c][j] from iteration 0xffffffff, slot 1 + j (no render iteration reaches it).
// 23 bits, not 24: ((2^24 - 1) + 0.5) rounds to 2^24 in f32 and u would be 1.0; with 23 bits the largest value,
// 1 - 2^-24, is exact.  u is never 0, so normaldist(u) is finite (u = 0 would give -inf and a NaN chain).
//
// Chain state: X[2][nchains][32] (double-buffered: bit[c] names the current half, an accept flips it), L[nchains][3].
// Splat records: key[k][c] = film element, val[k][c] = (r, g, b, 0) for iteration t0 + k of chain c.  The splat pass
// stable-sorts them by key (rocPRIM radix sort), so a pixel's records stay in (iteration, chain) order, and one lane per
// pixel adds its run with film_add_sample: no float atomics, the film is the same for any split of the iterations.

#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>          // the splat pass's sort
#include "path_common.h"
#include "film_ops.h"

DEV unsigned mlt_pcg(unsigned v) {
    unsigned s = v * 747796405u + 2891336453u;
    unsigned w = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;
    return (w >> 22) ^ w;
}
DEV float mlt_uniform(unsigned seed, unsigned chain, unsigned iter, unsigned slot) {
    unsigned h = mlt_pcg(mlt_pcg(mlt_pcg(mlt_pcg(seed) + chain) + iter) + slot);
    return ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-7f;             // 2^-23
}

// erfinv / normaldist, common.py:338-357 (Winitzki's approximation; the constants are the reference's Python doubles
// rounded to f32, as Taichi does)
DEV float mlt_erfinv(float x) {
    float sgn = x < 0.0f ? -1.0f : 1.0f;
    x = (1.0f - x) * (1.0f + x);
    float lnx = logf(x);
    float tt1 = (float)(2.0 / (3.141592653589793 * 0.147)) + 0.5f * lnx;
    float tt2 = (float)(1.0 / 0.147) * lnx;
    return sgn * sqrtf(-tt1 + sqrtf(tt1 * tt1 - tt2));
}
DEV float mlt_normaldist(float u) { return 1.41421356f * mlt_erfinv(u * 2.0f - 1.0f); }             // ti.sqrt(2) in f32

// (X_old + dX) % 1, mltpath.py:63: Taichi's float mod is x - floor(x); a result that rounds to 1.0 (x just below an
// integer) wraps to 0.0 -- a coordinate of 1.0 would splat to pixel nx
DEV float mlt_wrap(float x) {
    float r = x - floorf(x);
    return r >= 1.0f ? 0.0f : r;
}

// ifloor(x * nx), mltpath.py:47, clamped to the film: for a width that is not a power of two (1 - 2^-24) * nx can round
// up to nx
DEV int mlt_cell(float x, int n) {
    int i = (int)floorf(x * (float)n);
    return i < 0 ? 0 : i >= n ? n - 1 : i;
}

// MLTPathEngine._render, mltpath.py:55-83: lane = chain, iterations t0 .. t0 + K - 1
template <int STACK>
__global__ __launch_bounds__(MPT_BLOCK) void MPT_SUFFIX(mlt_chain_kernel)(const MptRenderParams p, const MptMltArgs a) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    const int c = blockIdx.x * MPT_BLOCK + threadIdx.x;
    if (c >= a.nchains) return;
    const size_t half = (size_t)a.nchains * 32;
    int cur = a.bit[c];
    const float *Xo = a.X + cur * half + (size_t)c * 32;
    float *Xn = a.X + (cur ^ 1) * half + (size_t)c * 32;
    V3 Lo = v3(a.L[(size_t)c * 3], a.L[(size_t)c * 3 + 1], a.L[(size_t)c * 3 + 2]);
    Cnt cnt = {};
    for (int k = 0; k < a.K; k++) {
        const unsigned t = (unsigned)(a.t0 + k);
        // proposal, mltpath.py:58-64
        const bool large = mlt_uniform(a.seed, (unsigned)c, t, 0u) < a.lsp;
        float x0 = 0.0f, x1 = 0.0f;
        for (int j = 0; j < 32; j++) {
            const float u = mlt_uniform(a.seed, (unsigned)c, t, 1u + (unsigned)j);
            float x;
            if (large) x = u;
            else {
                const float dX = a.sigma * mlt_normaldist(u);
                x = mlt_wrap(Xo[j] + dX);
            }
            Xn[j] = x;
            if (j == 0) x0 = x;
            if (j == 1) x1 = x;
        }
        // trace, mltpath.py:66-69
        PathState s;
        path_begin_vec<false>(p, s, Xn, cnt);
        while (!path_step<false>(p, tr, s, cnt)) {}
        // splat record, mltpath.py:76 (accum is 1)
        const size_t r = (size_t)k * a.nchains + c;
        a.keys[r] = (unsigned)(mlt_cell(x0, p.nx) * p.ny + mlt_cell(x1, p.ny));
        MptVec4 v; v.x = s.result.x; v.y = s.result.y; v.z = s.result.z; v.w = 0.0f;
        a.vals[r] = v;
        // accept, mltpath.py:71-82.  min(1, ratio) written so that a NaN ratio stays NaN: the coin's compare is then false
        // and a NaN path is never accepted (it is splatted, as above)
        const float an = vavg(s.result) + 1e-10f, ao = vavg(Lo) + 1e-10f;
        const float ratio = m_div(an, ao);
        const float accept = ratio > 1.0f ? 1.0f : ratio;
        if (mlt_uniform(a.seed, (unsigned)c, t, 33u) < accept) {
            Lo = s.result;
            cur ^= 1;
            const float *tmp = Xo; Xo = Xn; Xn = (float *)tmp;
        }
    }
    a.bit[c] = cur;
    a.L[(size_t)c * 3] = Lo.x; a.L[(size_t)c * 3 + 1] = Lo.y; a.L[(size_t)c * 3 + 2] = Lo.z;
}

// test door mpt_mlt_trace: camera + path_trace of given 32-vectors (mltpath.py:66-69) with the build's tracer
template <int STACK>
__global__ __launch_bounds__(MPT_BLOCK) void MPT_SUFFIX(mlt_trace_kernel)(const MptRenderParams p, const float *X, float *rgb, int n) {
    __shared__ int s_stack[STACK * MPT_BLOCK];
    BlockTracer tr = make_block_tracer(p, s_stack + threadIdx.x);
    const int i = blockIdx.x * MPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    Cnt cnt = {};
    PathState s;
    path_begin_vec<false>(p, s, X + (size_t)i * 32, cnt);
    while (!path_step<false>(p, tr, s, cnt)) {}
    rgb[(size_t)i * 3] = s.result.x; rgb[(size_t)i * 3 + 1] = s.result.y; rgb[(size_t)i * 3 + 2] = s.result.z;
}

MPT_KERNEL_API hipError_t MPT_SUFFIX(mpt_launch_mlt_chain)(const MptRenderParams *p, const MptMltArgs *a, int stack, hipStream_t stream) {
    const int grid = (a->nchains + MPT_BLOCK - 1) / MPT_BLOCK;
    return launch_by_stack<MPT_SUFFIX(mlt_chain_kernel)<32>, MPT_SUFFIX(mlt_chain_kernel)<64>>(stack, grid, stream, *p, *a);
}

MPT_KERNEL_API hipError_t MPT_SUFFIX(mpt_launch_mlt_trace)(const MptRenderParams *p, const float *X, float *rgb, int n, int stack,
                                                        hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int grid = (n + MPT_BLOCK - 1) / MPT_BLOCK;
    return launch_by_stack<MPT_SUFFIX(mlt_trace_kernel)<32>, MPT_SUFFIX(mlt_trace_kernel)<64>>(stack, grid, stream, *p, X, rgb, n);
}

#if MPT_STRICT
// ---------------------------------------------------------------- build-independent passes (compiled once, in the strict object)
// MLTPathEngine.reset, mltpath.py:31-37: X_old = random(), L_old = 0; the current half is X[0]
__global__ void mlt_reset_kernel(float *X, float *L, int *bit, int nchains, unsigned seed) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchains) return;
    for (int j = 0; j < 32; j++) X[(size_t)c * 32 + j] = mlt_uniform(seed, (unsigned)c, 0xffffffffu, 1u + (unsigned)j);
    L[(size_t)c * 3] = 0.0f; L[(size_t)c * 3 + 1] = 0.0f; L[(size_t)c * 3 + 2] = 0.0f;
    bit[c] = 0;
}

MPT_KERNEL_API hipError_t mpt_launch_mlt_reset(float *X, float *L, int *bit, int nchains, unsigned seed, hipStream_t stream) {
    hipLaunchKernelGGL(mlt_reset_kernel, dim3((nchains + 255) / 256), dim3(256), 0, stream, X, L, bit, nchains, seed);
    return hipGetLastError();
}

// the run of each film element in the sorted keys: [start, end); elements without records keep the zeroed [0, 0)
__global__ void mlt_runs_kernel(const unsigned *keys, int n, unsigned *start, unsigned *end) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const unsigned key = keys[k];
    if (k == 0 || keys[k - 1] != key) start[key] = (unsigned)k;
    if (k == n - 1 || keys[k + 1] != key) end[key] = (unsigned)k + 1u;
}

// film[pix] += every record of the pixel, in sorted = (iteration, chain) order (path.py:93's film_add_sample, w += 1)
__global__ void mlt_add_kernel(MptVec4 *film, const MptVec4 *vals, const unsigned *start, const unsigned *end, int npix) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    const unsigned k0 = start[pix], k1 = end[pix];
    if (k0 >= k1) return;
    MptVec4 acc = film[pix];
    for (unsigned k = k0; k < k1; k++) {
        const MptVec4 v = vals[k];
        film_add_sample(acc, v.x, v.y, v.z);
    }
    film[pix] = acc;
}

static int mlt_key_bits(int npix) {
    int b = 1;
    while (b < 32 && (1u << b) < (unsigned)npix) b++;
    return b;
}

// scratch bytes of the sort of n records over npix film elements
MPT_KERNEL_API hipError_t mpt_mlt_sort_bytes(int n, int npix, size_t *bytes) {
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, (const unsigned *)nullptr, (unsigned *)nullptr, (const MptVec4 *)nullptr,
                                     (MptVec4 *)nullptr, (size_t)n, 0, mlt_key_bits(npix), (hipStream_t)0);
}

// the splat pass: sort (key, val) -> (keys2, vals2), find the runs, add them to the film.  runs: 2 * npix words
MPT_KERNEL_API hipError_t mpt_launch_mlt_splat(MptVec4 *film, const unsigned *keys, const MptVec4 *vals, unsigned *keys2, MptVec4 *vals2,
                                               void *tmp, size_t tmp_bytes, unsigned *runs, int n, int npix, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipError_t e;
    if ((e = rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys2, vals, vals2, (size_t)n, 0, mlt_key_bits(npix), stream)) != hipSuccess)
        return e;
    if ((e = hipMemsetAsync(runs, 0, (size_t)npix * 2 * sizeof(unsigned), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(mlt_runs_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, keys2, n, runs, runs + npix);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(mlt_add_kernel, dim3((npix + 255) / 256), dim3(256), 0, stream, film, vals2, runs, runs + npix, npix);
    return hipGetLastError();
}
#endif

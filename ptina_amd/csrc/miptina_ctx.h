// miptina_ctx.h -- what the translation units of the host runtime share: the context, the error
// plumbing and the launchers of the kernels.  Internal; the public surface is include/miptina.h.
#pragma once

#include "../../include/miptina.h"
#include "mpt_types.h"
#include "mpt_options.h"
#include "shade_feat.h"
#include "refit_rule.h"
#include "run_table.h"
#include "deform_rule.h"
#include "anim_rule.h"
#include "subdiv_rule.h"
#include "displace_rule.h"
#include "scatter_rule.h"
#include "history_rule.h"
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

// A launcher that both builds of a dual translation unit define (Makefile DUAL; path_common.h MPT_SUFFIX): one signature, the two
// names.  MPT_LAUNCHER(c, name) is the one of the build the context renders with.
#define MPT_DUAL_LAUNCHER(name, ...)                    \
    MPT_KERNEL_API hipError_t name##_fast(__VA_ARGS__); \
    MPT_KERNEL_API hipError_t name##_strict(__VA_ARGS__)
#define MPT_LAUNCHER(c, name) ((c)->opt.mode == MPT_MODE_STRICT ? name##_strict : name##_fast)

// kernel launchers (render_kernel.hip x2, aux_kernels.hip)
MPT_DUAL_LAUNCHER(mpt_launch_render, const MptRenderParams *, int grid, int stack, int count, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_derive_materials(MptMaterial *mats, int count, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_derive_tfast(const MptVec4 *tgeo, MptVec4 *tfast, int n, hipStream_t);
MPT_KERNEL_API hipError_t mpt_wide_blocks(int grid, int count, int quant, int *blocks);
MPT_KERNEL_API hipError_t mpt_launch_render_wide(const MptRenderParams *, int blocks, int count, int quant, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_render_lds(const MptRenderParams *, int grid, int block, size_t lds_bytes, int count, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_render_lds4(const MptRenderParams *, int grid, int block, size_t lds_bytes, int count, int feat, int lean, hipStream_t);
// mlt_kernel.hip: the Metropolis engine's chain kernel (both builds), its test door, and the build-independent passes
MPT_DUAL_LAUNCHER(mpt_launch_mlt_chain, const MptRenderParams *, const MptMltArgs *, int stack, hipStream_t);
MPT_DUAL_LAUNCHER(mpt_launch_mlt_trace, const MptRenderParams *, const float *X, float *rgb, int n, int stack, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_mlt_reset(float *X, float *L, int *bit, int nchains, unsigned seed, hipStream_t);
MPT_KERNEL_API hipError_t mpt_mlt_sort_bytes(int n, int npix, size_t *bytes);
MPT_KERNEL_API hipError_t mpt_launch_mlt_splat(MptVec4 *film, const unsigned *keys, const MptVec4 *vals, unsigned *keys2, MptVec4 *vals2,
                                               void *tmp, size_t tmp_bytes, unsigned *runs, int n, int npix, hipStream_t);
// brute_kernel.hip: the brute-force engine's kernel (both builds)
MPT_DUAL_LAUNCHER(mpt_launch_brute, const MptRenderParams *, int grid, int stack, hipStream_t);
// adapt_kernel.hip: adaptive sampling's list render kernel (both builds); samples holds count * nframes records
MPT_DUAL_LAUNCHER(mpt_launch_adapt_render, const MptRenderParams *, const int32_t *list, int count, MptVec4 *samples, int stack, hipStream_t);
MPT_DUAL_LAUNCHER(mpt_launch_preview, const MptRenderParams *, int grid, int stack, hipStream_t);
// query_kernel.hip: the batch ray queries (both builds), one lane per ray of MptQueryArgs
MPT_DUAL_LAUNCHER(mpt_launch_query_closest, const MptRenderParams *, const MptQueryArgs *, int stack, hipStream_t);
MPT_DUAL_LAUNCHER(mpt_launch_query_occluded, const MptRenderParams *, const MptQueryArgs *, int stack, hipStream_t);
// walk_eval.hip: the test door through the production walks (production build only); walk: MPT_WALK_* of include/miptina.h
MPT_KERNEL_API hipError_t mpt_launch_walk_eval(const MptRenderParams *, const MptQueryArgs *, int walk, int stack, size_t lds_bytes, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_sobol_update(const int *X, int *Xout, const int *V, float *P, int dim, int rows, int time0,
                                              int count, int keep, int write_x, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_launch_combine(MptVec4 *film, const MptVec4 *partial, int ny, int x0, int x1,
                                         int stripe_w, int stripe_pitch, int ccols, int nframes, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_resolve(const MptVec4 *film, MptVec4 *out, size_t npix, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_probe(double *out, int threads, size_t lds_bytes, hipStream_t);
MPT_DUAL_LAUNCHER(mpt_launch_unit_eval, const MptRenderParams *, int kind, const float *in, int in_cols, float *out, int out_cols, int n, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_copy_pieces(const MptVec4 *src, MptVec4 *dst, const MptPiece *tab, int npieces,
                                             long long max_count, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_export(const MptVec4 *film, float *out, int nx, int ny, hipStream_t);
// denoise.hip: the A-Trous filter of pass 0 guided by passes 1 and 2 (mpt_get_denoised)
// (guided by variance: mark and v, v_in and v_out given, kc = sigma_variance^2; the fixed filter: all four null)
MPT_KERNEL_API hipError_t mpt_launch_denoise_prologue(const MptVec4 *f0, const MptVec4 *f1, const MptVec4 *f2, MptVec4 *e, MptVec4 *a,
                                                      MptVec4 *n, size_t npix, int demodulate, const MptVec4 *mark, float *v, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_denoise_atrous(const MptVec4 *e_in, MptVec4 *e_out, const MptVec4 *a, const MptVec4 *n, int nx, int ny,
                                                    int s, float kc, float ka, float kn, int use_lds, const float *v_in, float *v_out, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_denoise_epilogue(const MptVec4 *e, const MptVec4 *a, MptVec4 *out, size_t npix, int demodulate, hipStream_t);
// display.hip: metering and the conversion to 8-bit RGBA (mpt_get_display); part holds 2 * mpt_display_parts(npix) doubles
MPT_KERNEL_API size_t mpt_display_parts(size_t npix);
MPT_KERNEL_API hipError_t mpt_launch_display_meter(const MptVec4 *src, size_t npix, double *part, float key, float *e_dev, float *e_host, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_display_convert(const MptVec4 *src, uint32_t *out, int nx, int ny, const MptDisplayArgs *a,
                                                     const float *e_dev /* NULL: a->exposure */, hipStream_t);
// noise.hip: the noise estimate of a film against its mark (mpt_get_noise); part holds max(mpt_noise_parts(npix), 1) records
MPT_KERNEL_API size_t mpt_noise_parts(size_t npix);
MPT_KERNEL_API hipError_t mpt_launch_noise(const MptVec4 *film, MptVec4 *mark, size_t npix, float threshold, int remark, float *map /* or NULL */,
                                           mpt_noise_stats *part, mpt_noise_stats *stats_host, hipStream_t);
// adapt_select.hip: the selection of the pixels that still need samples (mpt_adapt_select) and the fold of a list pass's samples
// into the film (mpt_render_selected); ballot holds 4 words and count one int per tile, list nx * ny indices
MPT_KERNEL_API size_t mpt_adapt_tiles(int nx, int ny);
MPT_KERNEL_API size_t mpt_adapt_tile_bound(size_t npix);
MPT_KERNEL_API hipError_t mpt_launch_adapt_select(const MptVec4 *film, const MptVec4 *mark, int nx, int ny, float threshold, int dilate,
                                                  unsigned long long *ballot, int *count, int32_t *list, long long *total_host, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_adapt_fold(MptVec4 *film, MptVec4 *mark /* or NULL */, const int32_t *list, int count, const MptVec4 *samples,
                                                int nframes, int remark, hipStream_t);
// history_kernel.hip: the G-buffer of the view as it is kept and the motion records of the new view (both builds); history.hip: the
// kept copy of the model's positions, and the resample launch with its fold; part holds max(mpt_history_parts(npix), 1) records
MPT_DUAL_LAUNCHER(mpt_launch_history_gbuffer, const MptRenderParams *, const MptHistoryArgs *, int stack, hipStream_t);
MPT_DUAL_LAUNCHER(mpt_launch_history_motion, const MptRenderParams *, const MptHistoryArgs *, int stack, hipStream_t);
MPT_KERNEL_API size_t mpt_history_parts(size_t npix);
MPT_KERNEL_API hipError_t mpt_launch_history_verts(const float *verts, float *kept, int n, hipStream_t);
MPT_KERNEL_API hipError_t mpt_launch_history_resample(const MptResampleArgs *, mpt_history_stats *part, mpt_history_stats *stats_host, hipStream_t);
// compose.hip: meshes of the pool placed by the object table, written as the model the tree builders read, and its bounding box
// (mpt_compose); part holds 6 floats per mpt_compose_groups(vertices) workgroups
MPT_KERNEL_API size_t mpt_compose_groups(size_t nverts);
MPT_KERNEL_API hipError_t mpt_launch_compose(const float *pool, const MptComposeObj *objs, const int *first, int nobj, int nverts,
                                             const MptRun *runs, int nruns, int blocks, int all, unsigned epoch, float *out,
                                             int *mtlids, float *part, float *bounds_host, hipStream_t);
// anim.hip: the poses of a launch's bound objects at scene time t, written where deform.hip reads them; the door of its acos and sin
MPT_KERNEL_API hipError_t mpt_launch_anim(const MptAnimObj *objs, int nobj, double t, const int32_t *parents, const int32_t *depths, const double *rest,
                                          const double *inverse_bind, const MptAnimTrack *tracks, const float *times, const float *values, double *pose,
                                          hipStream_t stream);
// ... and the world matrices of the objects that object clips move, written into their rows of the object table
MPT_KERNEL_API hipError_t mpt_launch_motion(const MptMotionObj *objs, int n, double t, const MptAnimTrack *tracks, const float *times, const float *values,
                                            MptComposeObj *rows, int nrows, unsigned epoch, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_launch_anim_trig(const double *x, int n, double *acos_out, double *sin_out, hipStream_t stream);
// hierarchy.hip
MPT_KERNEL_API hipError_t mpt_launch_hierarchy_walk(const MptHierObj *items, const MptHierLevels *lv, int nlevels, double t, const MptAnimTrack *tracks,
                                                    const float *times, const float *values, const double *pose, int64_t npose, MptComposeObj *rows,
                                                    int nrows, unsigned epoch, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_launch_hierarchy_level(const MptHierObj *items, int begin, int end, double t, const MptAnimTrack *tracks, const float *times,
                                                     const float *values, const double *pose, int64_t npose, MptComposeObj *rows, int nrows, unsigned epoch,
                                                     hipStream_t stream);
// deform.hip: the deformed copies of the objects of a launch's table, written into the pool the meshes lie in (mpt_compose)
MPT_KERNEL_API hipError_t mpt_launch_deform(float *pool, const MptDeformObj *objs, const MptRun *runs, int nruns, int blocks,
                                            const float *deltas, const uint16_t *joints, const float *weights, const double *pose,
                                            hipStream_t stream);
// subdiv.hip: the subdivided copies of a launch's jobs -- one refine launch per level, the last level's normals, the records (mpt_compose)
MPT_KERNEL_API hipError_t mpt_launch_subdiv_refine(const float *pool, const MptSubdivJob *jobs, const MptRun *runs, int nruns, int blocks,
                                                   int level, int cc, const int32_t *topo, double *work, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_launch_subdiv_normals(const MptSubdivJob *jobs, const MptRun *runs, int nruns, int blocks, const int32_t *topo,
                                                    double *work, hipStream_t stream);
// displace.hip: the displaced positions of a launch's displaced jobs, between the last refine launch and the normals (mpt_compose)
MPT_KERNEL_API hipError_t mpt_launch_displace(const float *pool, const MptSubdivJob *jobs, const MptDisplaceJob *djobs, const MptRun *runs, int nruns,
                                              int blocks, const int32_t *topo, const MptVec4 *texels, double *work, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_launch_subdiv_emit(float *pool, const MptSubdivJob *jobs, const MptRun *runs, int nruns, int blocks,
                                                 const int32_t *topo, const double *work, hipStream_t stream);
// scatter.hip: the weights of the selecting scatters' faces with their largest, the faces' integer shares scanned, the instances'
// sticky records, and the instances' world matrices written into the object table (mpt_compose)
MPT_KERNEL_API hipError_t mpt_launch_scatter_weights(const float *pool, const MptComposeObj *objs, const MptScatterJob *jobs, const MptRun *runs, int nruns,
                                                     int blocks, const MptVec4 *texels, double *w, double *part, double *wmax, double *wmax_host,
                                                     hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_launch_scatter_scan(const MptScatterJob *jobs, const MptRun *runs, int nruns, int blocks, const double *w, const double *wmax,
                                                  uint32_t *q, uint64_t *cdf, uint64_t *bsum, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_launch_scatter_select(const MptScatterJob *jobs, const MptRun *runs, int nruns, int blocks, const uint64_t *cdf,
                                                    MptScatterPoint *points, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_launch_scatter_place(const float *pool, MptComposeObj *objs, const MptScatterJob *jobs, const MptRun *runs, int nruns,
                                                   int blocks, const MptScatterPoint *points, unsigned epoch, hipStream_t stream);
// scatter_space.hip: the elimination of the spaced scatters' candidates -- their positions and the grid over them (five kernels),
// `n` rounds, and the first `count` kept records compacted into the sticky arena
MPT_KERNEL_API hipError_t mpt_launch_space_grid(const float *pool, const MptComposeObj *objs, const MptScatterJob *jobs, const MptSpaceJob *sjobs,
                                                const MptRun *runs, int nruns, int blocks, const MptScatterPoint *records, double *pos, double *part,
                                                MptSpaceGrid *grids, int32_t *state, uint32_t *cursor, uint32_t *start, int32_t *items, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_launch_space_rounds(const MptSpaceJob *sjobs, const MptSpaceGrid *grids, const MptRun *runs, int nruns, int blocks,
                                                  const double *pos, const uint32_t *start, const uint32_t *cursor, const int32_t *items, int32_t *state,
                                                  uint32_t *left_host, unsigned first, int n, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_launch_space_compact(const MptSpaceJob *sjobs, const MptRun *runs, int nruns, const int32_t *state,
                                                   const MptScatterPoint *records, MptScatterPoint *points, int32_t *index, uint32_t *kept_host,
                                                   hipStream_t stream);

// on-GPU LBVH build (lbvh_build.hip)
struct MptLbvhBuffers {
    const float *verts; const int *mtlids; int n;
    float *cen; int *bounds;
    unsigned long long *keys_in, *keys_out;
    void *sort_tmp; size_t sort_tmp_bytes;
    int *child, *parent, *leaf, *mc;
    float *bmin, *bmax;
    unsigned *arrive;
    int *depth;
    MptVec4 *snode, *fnode, *tgeo, *tshade;
};
MPT_KERNEL_API size_t mpt_sah_seg_capacity(int n);
MPT_KERNEL_API size_t mpt_sah_chunk_capacity(int n);
MPT_KERNEL_API size_t mpt_sah_task_capacity(int n);
MPT_KERNEL_API size_t mpt_sah_part_words(int n);
MPT_KERNEL_API size_t mpt_sah_segbin_words(int n);
MPT_KERNEL_API size_t mpt_sah_level_words(int n, size_t nseg, int *nb_out);
MPT_KERNEL_API int mpt_sah_task_max(void);
MPT_KERNEL_API hipError_t mpt_sah_build(const MptSahBuffers *B, int *depth, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_wide_scan_bytes(int ni, size_t *bytes);
MPT_KERNEL_API hipError_t mpt_wide_build(const MptVec4 *fnode, int n, MptVec4 *wnode, MptVec4 *qnode, int *bin_of, int *ncount,
                                     void *scan_tmp, size_t scan_bytes, double *d_area, int *nwide, int *depth,
                                     double area[2], hipStream_t stream, volatile int *mail_host, int *mail_dev);
MPT_KERNEL_API hipError_t mpt_lbvh_sort_bytes(int n, size_t *bytes);
MPT_KERNEL_API hipError_t mpt_lbvh_build(const MptLbvhBuffers *b, hipStream_t stream);
MPT_KERNEL_API hipError_t mpt_lbvh_refit(const MptLbvhBuffers *b, hipStream_t stream);     // boxes, snode, tgeo, tshade over the hierarchy as it stands
// refit.hip: the parent slots of the binary and the wide records, their boxes fitted bottom-up to the vertices, the cost figure
MPT_KERNEL_API hipError_t mpt_refit_link(const MptVec4 *fnode, int ni, const MptVec4 *wnode, int nw, int *bin_parent, int *wide_parent, hipStream_t);
MPT_KERNEL_API hipError_t mpt_refit_cost(const MptVec4 *fnode, int ni, unsigned long long *sum, hipStream_t);
MPT_KERNEL_API hipError_t mpt_refit_fit(const float *verts, const int *leaf, int n, MptVec4 *fnode, const int *bin_parent, MptVec4 *wnode,
                                        MptVec4 *qnode, int nw, const int *wide_parent, unsigned *arrive, hipStream_t);

// ------------------------------------------------------------------ errors (miptina.cpp)
#define MPT_INTERNAL __attribute__((visibility("hidden")))   // shared between the .cpp files, not exported
MPT_INTERNAL int fail(const char *fmt, ...);

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return fail("%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ------------------------------------------------------------------ owned memory
struct MptNoCopy { MptNoCopy() = default; MptNoCopy(const MptNoCopy &) = delete; MptNoCopy &operator=(const MptNoCopy &) = delete; };

// A device allocation and its capacity in elements.  reserve() grows only and does not synchronise: the caller orders the free
// behind whatever still uses the old buffer.  A failed allocation leaves {nullptr, 0}, so the next call tries again instead of
// trusting a stale capacity.  Converts to T*, so launches and parameter structs take it as they took the raw pointer.
template <class T>
struct DevBuf : MptNoCopy {
    T *p = nullptr; size_t cap = 0;
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    int reserve(size_t n, bool *replaced = nullptr) {
        if (n <= cap) return 0;
        release();
        const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return fail("hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e)); }
        cap = n;
        if (replaced) *replaced = true;
        return 0;
    }
};

// The same for page-locked host memory (flags: hipHostMallocDefault, or hipHostMallocMapped for what a kernel writes)
template <class T>
struct PinnedBuf : MptNoCopy {
    T *p = nullptr; size_t cap = 0;
    ~PinnedBuf() { release(); }
    operator T *() const { return p; }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    int reserve(size_t n, unsigned flags) {
        if (n <= cap) return 0;
        release();
        const hipError_t e = hipHostMalloc((void **)&p, n * sizeof(T), flags);
        if (e != hipSuccess) { p = nullptr; return fail("hipHostMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e)); }
        cap = n;
        return 0;
    }
};

// Page-locked words a kernel writes and the host reads without a copy: the memory and its device alias, zeroed when made
template <class T>
struct MPT_INTERNAL MappedBuf {
    PinnedBuf<T> host; T *dev = nullptr;
    int create(size_t n) {
        if (host.reserve(n, hipHostMallocMapped)) return 1;
        HIP_TRY(hipHostGetDevicePointer((void **)&dev, host, 0));
        memset(host, 0, n * sizeof(T));
        return 0;
    }
};

// A stream (non-blocking) and an event, made on demand and destroyed with their owner.  They convert to the raw handle.
struct MPT_INTERNAL MptStream : MptNoCopy {
    hipStream_t s = nullptr;
    ~MptStream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    int create() { if (!s) HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return 0; }
};

struct MPT_INTERNAL MptEvent : MptNoCopy {
    hipEvent_t e = nullptr;
    ~MptEvent() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    int create(unsigned flags = hipEventDisableTiming) { if (!e) HIP_TRY(hipEventCreateWithFlags(&e, flags)); return 0; }   // (default: ordering only)
};

// Buffers that are sized together share one capacity and one reserve(): everything is freed, then allocated in the order
// written; `cap` is set only when all of it is there.
struct MPT_INTERNAL MptDisplayBufs {       // what mpt_get_display's kernels write, for a film of up to `cap` pixels
    DevBuf<uint32_t> rgba8;              // the packed image
    DevBuf<double> part;                 // the metering's partial sums: (sum, count) per workgroup of the first stage
    DevBuf<float> exposure;              // the metered exposure, where the conversion reads it
    size_t cap = 0;
    void release() { rgba8.release(); part.release(); exposure.release(); cap = 0; }
    int reserve(size_t npix) {
        if (npix <= cap) return 0;
        release();
        if (rgba8.reserve(npix) || part.reserve(2 * std::max<size_t>(mpt_display_parts(npix), 1)) || exposure.reserve(1)) return 1;
        cap = npix;
        return 0;
    }
};

struct MPT_INTERNAL MptNoiseBufs {         // what mpt_get_noise's kernels write, for a film of up to `cap` pixels
    DevBuf<float> map;                   // the estimate per pixel
    DevBuf<mpt_noise_stats> part;        // the first stage's partial statistics, one record per workgroup
    size_t cap = 0;
    void release() { map.release(); part.release(); cap = 0; }
    int reserve(size_t npix) {
        if (npix <= cap) return 0;
        release();
        if (map.reserve(npix) || part.reserve(std::max<size_t>(mpt_noise_parts(npix), 1))) return 1;
        cap = npix;
        return 0;
    }
};

struct MPT_INTERNAL MptAdaptBufs {         // what mpt_adapt_select's kernels write, for a film of up to `cap` pixels of any shape
    DevBuf<int32_t> list;                // the selection: film indices
    DevBuf<unsigned long long> ballot;   // the waves' ballots of their active lanes, 4 per tile
    DevBuf<int> count;                   // per tile: its active pixels, then its offset into the list
    DevBuf<mpt_noise_stats> part;        // the statistics' first-stage partials (noise.hip)
    size_t cap = 0;
    void release() { list.release(); ballot.release(); count.release(); part.release(); cap = 0; }
    int reserve(size_t npix) {
        if (npix <= cap) return 0;
        release();
        const size_t tiles = mpt_adapt_tile_bound(npix);
        if (list.reserve(npix) || ballot.reserve(4 * tiles) || count.reserve(tiles) || part.reserve(std::max<size_t>(mpt_noise_parts(npix), 1))) return 1;
        cap = npix;
        return 0;
    }
};

struct MPT_INTERNAL MptDenoiseBufs {       // mpt_denoise_eval: the caller's guide passes and what the filter's kernels write, for a film of up to `cap` pixels
    DevBuf<MptVec4> f1, f2;              // the accumulators of passes 1 and 2 (pass 0 and the mark go through MptDoorInput)
    DevBuf<MptVec4> e[2], a, n;          // as MptFilmBufs' dn_e, dn_a, dn_n
    DevBuf<float> v[2];                  // ... and dn_v
    size_t cap = 0;
    void release() { for (DevBuf<MptVec4> *b : { &f1, &f2, &e[0], &e[1], &a, &n }) b->release(); v[0].release(); v[1].release(); cap = 0; }
    int reserve(size_t npix) {
        if (npix <= cap) return 0;
        release();
        for (DevBuf<MptVec4> *b : { &f1, &f2, &e[0], &e[1], &a, &n })
            if (b->reserve(npix)) return 1;
        if (v[0].reserve(npix) || v[1].reserve(npix)) return 1;
        cap = npix;
        return 0;
    }
};

struct MPT_INTERNAL MptDoorInput {         // the test doors' input: the caller's accumulators for a film of up to `cap` pixels
    DevBuf<MptVec4> acc[2];              // mpt_display_eval uses the first; mpt_noise_eval and mpt_denoise_eval both: the film, and the mark (which mpt_noise_eval may rewrite)
    size_t cap = 0;
    int reserve(size_t npix) {
        if (npix <= cap) return 0;
        cap = 0;
        acc[0].release(); acc[1].release();
        if (acc[0].reserve(npix) || acc[1].reserve(npix)) return 1;
        cap = npix;
        return 0;
    }
};

struct MPT_INTERNAL MptHistoryBufs {       // the reprojection's per-pixel buffers, for a film of up to `cap` pixels (film_history.cpp)
    DevBuf<int32_t> face, id;            // the kept G-buffer: the face and the object each pixel's centre ray hit
    DevBuf<float> depth;                 // ... and how far along the ray
    DevBuf<MptMotion> motion;            // the last reproject's motion records
    DevBuf<MptVec4> f_new;               // what the resample kernel writes: swapped with pass 0 (the film's), read back (the door's)
    DevBuf<mpt_history_stats> part;      // the counts' first-stage partials, one record per workgroup
    size_t cap = 0;
    void release() { face.release(); id.release(); depth.release(); motion.release(); f_new.release(); part.release(); cap = 0; }
    int reserve(size_t npix) {
        if (npix <= cap) return 0;
        release();
        if (face.reserve(npix) || id.reserve(npix) || depth.reserve(npix) || motion.reserve(npix) || f_new.reserve(npix) ||
            part.reserve(std::max<size_t>(mpt_history_parts(npix), 1))) return 1;
        cap = npix;
        return 0;
    }
};

struct MPT_INTERNAL MptFilmBufs {          // per pixel of the largest film set so far
    DevBuf<MptVec4> film[3];
    DevBuf<MptVec4> resolved;            // nx*ny float4 (get_image staging on device)
    DevBuf<float> exported;              // nx*ny*3
    // mpt_get_denoised's working buffers, nx*ny float4 each: the filtered colour e (rgb, valid flag) in two copies the
    // iterations alternate between (the one left over takes the image), and the guides a (albedo) and n (normal)
    DevBuf<MptVec4> dn_e[2], dn_a, dn_n;
    MptDisplayBufs disp;                 // mpt_get_display's 8-bit image and metering partials
    // mpt_film_mark's copy of pass 0 and what mpt_get_noise's kernels write: made by the first mark (reserve_mark), for `cap`
    // pixels, and released with the rest
    DevBuf<MptVec4> mark; MptNoiseBufs noise;
    // the variance-guided filter's plane v, nx*ny floats in two copies like dn_e: made by the first guided read-back
    // (reserve_variance), for `cap` pixels, and released with the rest
    DevBuf<float> dn_v[2];
    // adaptive sampling: the selection and its workspace, made by the first selection (reserve_adapt) for `cap` pixels, and the
    // list render kernel's samples, grown on demand (adapt_samples.cap records); released with the rest
    MptAdaptBufs adapt; DevBuf<MptVec4> adapt_samples;
    // reprojection: the kept G-buffer, the motion records and the buffer pass 0 is resampled into, made by the first
    // mpt_history_keep (reserve_history) for `cap` pixels; released with the rest, or by mpt_history_drop
    MptHistoryBufs hist;
    size_t cap = 0;
    int reserve_history() { return hist.reserve(cap); }
    int reserve_adapt() { return adapt.reserve(cap); }
    int reserve_mark() { return mark.reserve(cap) || noise.reserve(cap); }
    int reserve_variance() { return dn_v[0].reserve(cap) || dn_v[1].reserve(cap); }
    int reserve(size_t npix, hipStream_t stream) {     // the passes come back zeroed on `stream`
        if (npix <= cap) return 0;
        cap = 0;
        for (auto &b : film) b.release();
        resolved.release(); exported.release();
        for (DevBuf<MptVec4> *b : { &dn_e[0], &dn_e[1], &dn_a, &dn_n }) b->release();
        disp.release();
        mark.release(); noise.release();
        dn_v[0].release(); dn_v[1].release();
        adapt.release(); adapt_samples.release();
        hist.release();
        for (auto &b : film) {
            if (b.reserve(npix)) return 1;
            HIP_TRY(hipMemsetAsync(b, 0, npix * sizeof(MptVec4), stream));
        }
        if (resolved.reserve(npix) || exported.reserve(npix * 3)) return 1;
        for (DevBuf<MptVec4> *b : { &dn_e[0], &dn_e[1], &dn_a, &dn_n })
            if (b->reserve(npix)) return 1;
        if (disp.reserve(npix)) return 1;
        cap = npix;
        return 0;
    }
};

struct MPT_INTERNAL MptModelBufs {         // the device copy of the model
    DevBuf<float> d_verts; DevBuf<int> d_mtlids;
    size_t cap = 0;
    int reserve(size_t n, bool *replaced) {
        if (n <= cap) return 0;
        cap = 0;
        d_verts.release(); d_mtlids.release();
        if (d_verts.reserve(n * 24) || d_mtlids.reserve(n)) return 1;
        cap = n; *replaced = true;
        return 0;
    }
};

// A buffer that is appended to grows by copying into a larger one (at least twice the size): the first `used` elements are kept, the
// stream is idle when it returns.  The mesh pool and mesh deformation's arenas grow this way
template <class T>
inline int grow_keeping(DevBuf<T> &buf, size_t want, size_t used, hipStream_t stream) {
    if (want <= buf.cap) return 0;
    DevBuf<T> bigger;
    if (bigger.reserve(std::max(want, buf.cap * 2))) return 1;
    if (used) HIP_TRY(hipMemcpyAsync(bigger, buf, used * sizeof(T), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    buf.swap(bigger);
    return 0;
}

// Scene composition's device memory (scene_compose.cpp): the mesh pool grows by copying into a larger buffer (grow_pool), the table
// and the launch's workspace are sized by the objects and the output
struct MPT_INTERNAL MptComposeBufs {
    DevBuf<float> pool;                  // object-space records [vertex][8] of every mesh, back to back
    DevBuf<MptComposeObj> objs;          // the object table
    DevBuf<int> first;                   // the objects' first output faces, apart: what the lanes' binary search reads
    DevBuf<MptRun> runs;                 // a partial launch's runs of workgroups
    DevBuf<float> part;                  // 6 floats per workgroup of the output: min3, max3 of its positions
    int reserve_table(size_t nobj) { return objs.reserve(nobj) || first.reserve(nobj) || runs.reserve(nobj); }
    int grow_pool(size_t floats, size_t used, hipStream_t stream) { return grow_keeping(pool, floats, used, stream); }   // keeps the first `used` floats
};

// Mesh deformation's device memory (scene_deform.cpp): arenas that grow by copying into a larger buffer, as the mesh pool does --
// the meshes' deltas and skins, appended by mpt_mesh_set_morph / mpt_mesh_set_skin, and the objects' poses -- and a launch's tables
struct MPT_INTERNAL MptDeformBufs {
    DevBuf<float> deltas;                // [target][corner][6] f32 of every mesh with targets, back to back
    DevBuf<uint16_t> joints;             // [corner][4] joint indices of every mesh with a skin, back to back
    DevBuf<float> weights;               // [corner][4] their weights
    DevBuf<double> pose;                 // per deformable object: its morph weights, then its joints' 3x4 matrices
    DevBuf<MptDeformObj> objs;           // a launch's objects
    DevBuf<MptRun> runs;                 // ... and its runs of blocks
    int reserve_tables(size_t nobj) { return objs.reserve(nobj) || runs.reserve(nobj); }
};

// Keyframe animation's device memory (scene_anim.cpp): the arenas of the meshes' skeletons and clips, appended by mpt_mesh_set_skeleton /
// mpt_mesh_add_clip (they grow by copying, as the mesh pool does), and a launch's table
struct MPT_INTERNAL MptAnimBufs {
    DevBuf<int32_t> parents, depths;     // per joint of every skeleton, back to back: its parent within the skeleton (-1: a root), its depth
    DevBuf<double> rest;                 // [joint][10]: translation3 rotation4 scale3
    DevBuf<double> inverse_bind;         // [joint][12]
    DevBuf<MptAnimTrack> tracks;         // every clip's tracks, back to back (time_at / value_at count in the arenas below)
    DevBuf<float> times, values;         // the tracks' key times and values
    DevBuf<MptAnimObj> objs;             // a launch's objects
    DevBuf<MptMotionObj> moved;          // ... and the objects that object clips move (motion_kernel)
    DevBuf<MptHierObj> hier;             // ... and the bound children (hierarchy_kernel)
};

// Loop subdivision's device memory (scene_subdiv.cpp): the arena of the meshes' topology blocks, appended by mpt_mesh_set_subdivision
// (it grows by copying, as the mesh pool does), the jobs' f64 workspace and a launch's tables
struct MPT_INTERNAL MptSubdivBufs {
    DevBuf<int32_t> topo;                // every subdivided mesh's block of words (subdiv_rule.h), back to back; a displaced mesh's first-corner table (displace_rule.h) is a block of its own behind them
    DevBuf<double> work;                 // per job: the positions of levels 1..L, then the last level's vertex records, then a displaced copy's displaced positions
    DevBuf<MptSubdivJob> jobs;           // a compose's jobs
    DevBuf<MptDisplaceJob> djobs;        // ... the displacement of each (rows of copies without one are not read)
    DevBuf<MptRun> runs;                 // ... and the runs of its launches, (MPT_SUBDIV_MAX_LEVELS + 3) tables of up to a run per job
    int reserve_tables(size_t njobs) { return jobs.reserve(njobs) || djobs.reserve(njobs) || runs.reserve(njobs * (MPT_SUBDIV_MAX_LEVELS + 3)); }
};

struct MPT_INTERNAL MptLbvhBufs {          // workspace and result of the device LBVH build (lbvh_build.hip)
    DevBuf<float> d_cen; DevBuf<int> d_bounds, d_depth;
    DevBuf<unsigned long long> d_keys_in, d_keys_out;
    DevBuf<char> d_sort_tmp; size_t d_sort_bytes = 0;
    DevBuf<int> d_child, d_parent, d_leaf, d_mc;
    DevBuf<float> d_bmin, d_bmax;
    DevBuf<unsigned> d_arrive;
    size_t cap = 0;
    int reserve(size_t m) {
        if (m <= cap) return 0;
        cap = 0;
        d_cen.release(); d_bounds.release(); d_depth.release(); d_keys_in.release(); d_keys_out.release();
        d_sort_tmp.release(); d_child.release(); d_parent.release(); d_leaf.release(); d_mc.release();
        d_bmin.release(); d_bmax.release(); d_arrive.release();
        HIP_TRY(mpt_lbvh_sort_bytes((int)m, &d_sort_bytes));
        if (d_cen.reserve(m * 3) || d_bounds.reserve(6) || d_depth.reserve(1) || d_keys_in.reserve(m) || d_keys_out.reserve(m) ||
            d_sort_tmp.reserve(std::max<size_t>(d_sort_bytes, 16)) || d_child.reserve(m * 2) || d_parent.reserve(m * 2) ||
            d_leaf.reserve(m) || d_mc.reserve(m) || d_bmin.reserve(m * 3) || d_bmax.reserve(m * 3) || d_arrive.reserve(m)) return 1;
        cap = m;
        return 0;
    }
};

struct MPT_INTERNAL MptNodeBufs {          // per internal node: the reference tree's records and the fast build's
    DevBuf<MptVec4> snode, fnode;
    size_t cap = 0;
    int reserve(size_t ni) {
        if (ni <= cap) return 0;
        cap = 0;
        snode.release(); fnode.release();
        if (snode.reserve(ni * 2) || fnode.reserve(ni * 4)) return 1;
        cap = ni;
        return 0;
    }
};

struct MPT_INTERNAL MptTriBufs {           // per leaf slot: the reference-order triangle records
    DevBuf<MptVec4> tgeo, tshade;
    size_t cap = 0;
    int reserve(size_t n) {
        if (n <= cap) return 0;
        cap = 0;
        tgeo.release(); tshade.release();
        if (tgeo.reserve(n * 4) || tshade.reserve(n * 4)) return 1;
        cap = n;
        return 0;
    }
};

struct MPT_INTERNAL MptWideBufs {          // workspace of the device 4-wide collapse (wide_build.hip), per internal node
    DevBuf<int> bin_of, ncount;          // (the nodes' offsets within their workgroup live in ncount, the workgroups' in scan)
    DevBuf<char> scan; size_t scan_bytes = 0;
    DevBuf<double> area;
    size_t cap = 0;
    int reserve(size_t ni) {
        if (ni <= cap) return 0;
        cap = 0;
        bin_of.release(); ncount.release(); scan.release(); area.release();
        HIP_TRY(mpt_wide_scan_bytes((int)ni, &scan_bytes));
        if (bin_of.reserve(ni + 4) || ncount.reserve(ni) || scan.reserve(std::max<size_t>(scan_bytes, 16)) || area.reserve(2)) return 1;
        cap = ni;
        return 0;
    }
};

struct MPT_INTERNAL MptMltSlab {           // the Metropolis engine's splat records and the scratch of their sort
    DevBuf<uint32_t> keys, keys_sorted;
    DevBuf<MptVec4> vals, vals_sorted;
    DevBuf<char> tmp;                    // sort scratch: tmp.cap bytes
    DevBuf<uint32_t> runs;
    size_t cap = 0, runs_cap = 0;        // records the slab holds; film elements of the run table
    int reserve(size_t recs, size_t npix) {            // neither capacity shrinks when the other grows
        if (recs <= cap && npix <= runs_cap) return 0;
        const size_t ncap = std::max(recs, cap), nrcap = std::max(npix, runs_cap);
        size_t bytes = 0;
        HIP_TRY(mpt_mlt_sort_bytes((int)ncap, (int)nrcap, &bytes));
        cap = runs_cap = 0;
        keys.release(); keys_sorted.release(); vals.release(); vals_sorted.release(); tmp.release(); runs.release();
        if (keys.reserve(ncap) || keys_sorted.reserve(ncap) || vals.reserve(ncap) || vals_sorted.reserve(ncap) ||
            tmp.reserve(std::max(bytes, (size_t)16)) || runs.reserve(nrcap * 2)) return 1;
        cap = ncap; runs_cap = nrcap;
        return 0;
    }
};

// ------------------------------------------------------------------ launch timers
// The events recorded around the kernels of an engine's launches (per launch: `per_launch` events bounding per_launch - 1
// segments, in stream order), kept until somebody asks for the times.  Events come from and go back to the context's pool,
// which owns every timing event that no timer and no span holds.
struct MPT_INTERNAL MptEventPool : MptNoCopy {
    std::vector<hipEvent_t> idle;
    ~MptEventPool() { for (hipEvent_t e : idle) (void)hipEventDestroy(e); }
    hipEvent_t get() {
        hipEvent_t e = nullptr;
        if (idle.empty()) (void)hipEventCreate(&e);
        else { e = idle.back(); idle.pop_back(); }
        return e;
    }
    void put(hipEvent_t e) { if (e) idle.push_back(e); }
};

struct MPT_INTERNAL MptLaunchTimer {
    const int per_launch;
    MptEventPool &pool;
    std::vector<hipEvent_t> events;
    MptLaunchTimer(int n, MptEventPool &p) : per_launch(n), pool(p) {}
    ~MptLaunchTimer() { for (hipEvent_t e : events) pool.put(e); }      // (the pool is declared first, so it goes last)
    void record(const hipEvent_t *launch) {
        for (int q = 0; q < per_launch; q++) events.push_back(launch[q]);
        // nobody has asked for kernel times for a long while (an interactive session renders frame after
        // frame): keep the newest half.  The dropped events were recorded at least 2048 launches ago.
        const size_t half = (size_t)per_launch * 2048;
        if (events.size() <= 2 * half) return;
        for (size_t q = 0; q < half; q++) pool.put(events[q]);
        events.erase(events.begin(), events.begin() + half);
    }
    // seg_ms[per_launch - 1] += every launch's segments; the caller has synchronised the streams the events were recorded on
    int drain(double *seg_ms, int *launches) {
        for (size_t q = 0; q + per_launch <= events.size(); q += per_launch)
            for (int g = 0; g + 1 < per_launch; g++) {
                float t = 0;
                HIP_TRY(hipEventElapsedTime(&t, events[q + g], events[q + g + 1]));
                seg_ms[g] += t;
            }
        if (launches) *launches = (int)(events.size() / per_launch);
        for (hipEvent_t e : events) pool.put(e);
        events.clear();
        return 0;
    }
};

// One timed section of a stream.  Takes the timer's events from the pool and records the first (`begun`: how that went); mark()
// records the next, end() the last and files them all with the timer.  A span that goes out of scope before end() -- any error
// return in between -- gives its events back to the pool.
struct MPT_INTERNAL MptTimedSpan : MptNoCopy {
    MptLaunchTimer &timer;
    const hipStream_t stream;
    hipEvent_t ev[3] = {};                     // (no timer has more per launch)
    int next = 0;
    hipError_t begun;
    MptTimedSpan(MptLaunchTimer &t, hipStream_t s) : timer(t), stream(s) {
        for (int q = 0; q < timer.per_launch; q++) ev[q] = timer.pool.get();
        begun = mark();
    }
    ~MptTimedSpan() { for (hipEvent_t e : ev) timer.pool.put(e); }
    hipError_t mark() { return hipEventRecord(ev[next++], stream); }
    hipError_t end() {
        const hipError_t e = mark();
        if (e == hipSuccess) { timer.record(ev); for (hipEvent_t &q : ev) q = nullptr; }
        return e;
    }
};

// ------------------------------------------------------------------ the launch ring
// Launch pipelining (fast build): batch i renders in slot i mod cur_depth of the ring (2 to MPT_MAX_PIPE slots in use), on the slot's
// stream into its slab, while the main stream still combines / gathers / resolves batch i-1: one launch's tail overlaps the next one's head
struct MPT_INTERNAL MptRingSlot {
    MptStream stream;                             // the render
    MptEvent rendered;                            // ... of the batch in this slot has finished
    MptEvent consumed;                            // the combine pass has consumed the slab
    MptEvent ready;                               // Sobol points + zeroed queue heads of the batch are there
    DevBuf<MptVec4> slab;                         // one float4 per sample, [frame][pixel of the share]
    DevBuf<float> points;                         // [MPT_MAX_BATCH][sdim]
    DevBuf<unsigned int> heads;                   // 8 queue heads, a cache line each, and the finalisation's tile counter
    DevBuf<int> spill;                            // overflow strip of the wide kernel's per-lane stacks (launches of different slots are resident together and index theirs by block and lane only)
};

// ------------------------------------------------------------------ context
struct mpt_ctx {
    int device = 0;
    MptStream stream;
    mpt_caps caps{};

    MptOptions opt;                      // everything mpt_set_option sets (mpt_options.h)
    int max_mtlid = -1;                  // largest material id of the model (-1: only the default material)
    int num_cus = 256;
    int clock_khz = 0;                   // hipDeviceProp_t.clockRate: peak shader clock (roofline peaks in bench.py)
    int last_div = 1;                    // share of the chip the last launch took: 1/last_div of the CUs
    int last_kernel = 0;                 // what the last flush launched: MPT_KERNEL_* of lds_layout.h (0 binary gather, 1 LDS binary, 2 4-wide gather, 5 LDS 4-wide)
    int last_shade_feat = -1;            // the mask the last render launch was compiled for (MPT_FEAT_PLAIN / MPT_FEAT_GENERIC; -1: none yet)
    int last_shade_lean = -1;            // ... and whether it was the lean variant of the plain one (mpt_get_shade_variant)
    bool lean_on = true;                 // false: MIPTINA_SHADE_LEAN=0 was in the environment when the context was created (A/B timing)

    // film
    int nx = 0, ny = 0, x0 = 0, x1 = 0;
    int stripe_w = 0, stripe_idx = 0, stripe_mod = 1;   // stripe_w > 0: columns dealt out in stripes (mpt_set_stripes)
    MptFilmBufs fb;                      // the passes, the image staging and the denoiser's buffers; fb.cap: pixels allocated per pass

    // model (host copy kept for the tree build)
    int nfaces = 0;
    std::vector<float> verts;            // [3n][8]
    double scene_cen[3] = { 0, 0, 0 }, scene_rad = 0;   // bounding sphere of the model's box (mpt_load_model)
    std::vector<int32_t> mtlids;
    bool tree_valid = false;
    int tree_depth = 0;                  // reference LBVH (strict build)
    int fast_depth = 0;                  // tree the fast build walks (SAH or LBVH)
    bool host_tree_valid = false;        // h_child/h_leaf/... mirror the device tree (lazily downloaded)
    unsigned tree_seq = 0;               // counts the successful mpt_build_tree calls: a refit keeps the leaf order, a build makes a new one
    // device-side build workspace
    MptModelBufs dmodel;
    MptLbvhBufs lbvh;
    std::vector<int32_t> h_child, h_leaf, h_mc;
    std::vector<float> h_bmin, h_bmax;
    MptNodeBufs nodes;
    MptTriBufs tris;
    DevBuf<MptVec4> tfast;                            // production triangle records, 3 float4 each (derived from tgeo)
    DevBuf<MptVec4> qnode;                            // the same nodes, child boxes quantised to 8 bits, 4 float4 each
    DevBuf<MptVec4> wnode;                            // 4-wide nodes of the fast tree (gather kernel), 8 float4 each
    int wide_nodes = 0, wide_depth = 0;               // 0 nodes: not built (too deep)
    int wide_stack = 0;                               // stack levels a traversal of the 4-wide tree can ask for (exact from the host pass, 3 x depth + 2 from the device pass)
    float wide_ratio = 1.f;                           // expected fetches per ray, wide / binary (surface-area sums)
    MappedBuf<int> sah_mail;                          // [32]: the SAH pass's per-level hand-back (sah_build.hip plan kernel)
    MptSahStats sah_stats{};                          // what the last device SAH pass did
    bool h_model_stale = false;                       // the host copy (verts, mtlids) is behind the device's, which mpt_compose wrote: model_on_host fetches it
    bool d_model_stale = true;                        // the device copy of the model (d_verts, d_mtlids) is behind the host's: the next device build uploads
    double build_phase_us[6] = { 0, 0, 0, 0, 0, 0 };   // upload | LBVH | SAH pass | triangle records | 4-wide collapse | total (host clock)
    int sah_fallback = 0;                             // last build: the device SAH pass gave up (1: error, 2: depth) and the host pass ran
    DevBuf<char> sah_ws;                              // one allocation (sah_ws.cap bytes), carved up in build_sah_device
    MptWideBufs wb;

    // materials / images / lights / world / camera
    DevBuf<MptMaterial> mats;
    std::vector<unsigned char> mat_feat; // shade_feat_material of every record mpt_load_materials last loaded
    int default_feat = 0;                // ... and of the default material (mpt_create)
    std::vector<unsigned char> mat_lean; // shade_lean_material of the same records ...
    int default_lean = 1;                // ... and of the default material
    int nmats = 0;                       // material records mpt_load_materials last loaded (mpt_unit_eval refuses ids beyond them)
    int max_mat_tex = -1;                // largest texture id a loaded material names (-1: none): mpt_unit_eval checks it against the loaded images
    DevBuf<MptImage> images;
    std::vector<MptImage> h_images;
    DevBuf<MptVec4> texels;
    size_t texels_used = 0;
    unsigned long long image_gen = 1;    // counts mpt_load_image and mpt_reset_images: a displaced copy is displaced again when it moved (scene_subdiv.cpp)
    DevBuf<MptLight> lights;
    std::vector<MptLight> h_lights;
    float world_fac[4] = { 0.1f, 0.1f, 0.1f, 0.1f };   // light/world.py:14-16
    int world_tex = -1;                                 // documented deviation Q6 (reference default 0)
    float v2w[16], w2v[16];

    // sobol
    int sdim = 0, srows = 0;
    int32_t stime = 0;
    DevBuf<int> sV, sX;
    DevBuf<float> sP;                    // [MPT_MAX_BATCH][sdim]

    MptEventPool events;                 // the timing events at rest (declared before the timers, which hand theirs back to it)
    // Metropolis engine (mlt_kernel.hip, mpt_mlt_*): chain state, parameters, the iterations enqueued but not launched, splat slab
    struct MPT_INTERNAL Mlt {
        int n = 0, iter = 0, pending = 0; uint32_t seed = 0; float lsp = 0.25f, sigma = 0.01f;
        DevBuf<float> X, L; DevBuf<int32_t> bit;         // [2][n][32], [n][3], [n]
        MptMltSlab slab;
        MptLaunchTimer timer;                            // {chain start, chain end = splat start, splat end} per launch
        explicit Mlt(MptEventPool &ev) : timer(3, ev) {}
    } mlt{events};
    struct MPT_INTERNAL Display {                        // the display door (mpt_get_display, mpt_display_eval)
        MappedBuf<float> exposure;                       // the metered exposure of the last call
        MptDisplayBufs bufs;                             // mpt_display_eval: what the kernels write for the caller's accumulators (grown on demand)
        MptLaunchTimer timer;                            // mpt_get_display: {before the first kernel, after the conversion} per call
        explicit Display(MptEventPool &ev) : timer(2, ev) {}
    } display{events};
    struct MPT_INTERNAL Noise {                          // the noise estimate (mpt_film_mark, mpt_get_noise, mpt_noise_eval)
        bool marked = false;                             // fb.mark holds a mark of the film as it is sized now (mpt_clear and mpt_set_size drop it)
        MappedBuf<mpt_noise_stats> stats;                // the statistics of the last call
        MptNoiseBufs bufs;                               // mpt_noise_eval: what the kernels write for the caller's film and mark (grown on demand)
        MptLaunchTimer timer;                            // mpt_get_noise: {before the estimate, after the fold} per call
        explicit Noise(MptEventPool &ev) : timer(2, ev) {}
    } noise{events};
    struct MptAdaptRecord { mpt_noise_stats stats; long long count; };   // what a selection leaves in the host's mapped memory
    struct MPT_INTERNAL Adapt {                          // adaptive sampling (mpt_adapt_*, mpt_render_selected)
        bool selected = false; int count = 0;            // fb.adapt.list[0 .. count) is the selection (mpt_clear and mpt_set_size drop it)
        MappedBuf<MptAdaptRecord> rec;                   // the statistics and the count of the last selection
        MptAdaptBufs bufs;                               // mpt_adapt_eval: what the kernels write for the caller's film and mark (grown on demand)
        MptLaunchTimer select_timer, render_timer;       // mpt_adapt_select: {before the kernels, after them} per call; mpt_render_selected: the same around a call's launches
        explicit Adapt(MptEventPool &ev) : select_timer(2, ev), render_timer(2, ev) {}
    } adapt{events};
    // The scene side's two host tables, both Compose's (below): a row per mesh of the pool, which mpt_mesh_add alone adds, and a row per
    // object beside the device's record of it, which add_object (scene_compose.cpp) alone adds.  mpt_scene_clear clears both
    struct MptDeformMesh {                               // what mesh deformation keeps for a mesh (arena offsets)
        int ntargets = 0, njoints = 0; size_t delta_at = 0, skin_at = 0;
        bool skeleton = false; size_t joint_at = 0; int levels = 0;   // its skeleton (scene_anim.cpp): first joint in the arenas, the greatest depth of a joint
    };
    struct MptSubdivMesh {                               // what Loop subdivision keeps for a mesh: its level and where its topology lies
        MptSubdivHead head;                              // its block's header (subdiv_rule.h; levels 0: no subdivision), with srule_at = nrule_at where the mesh is uncreased: the records' rules are then the rings'
        size_t topo_at = 0;                              // the block's first word in bufs.topo
        int64_t out_faces = 0;                           // the triangles an object of the mesh has
        int job = -1;                                    // the shared copy of a mesh that is not deformable (-1: no object yet)
        // its texture displacement (mpt_mesh_set_displacement)
        bool displaced = false;
        int image = -1, mode = 0, channel = 0;           // the image of the image pool, MPT_DISPLACE_NORMAL / _VECTOR, MPT_DISPLACE_R .. _MEAN
        double strength = 0.0, midlevel = 0.0;
        size_t corner_at = 0;                            // the first-corner table of its last level: first word in bufs.topo
    };
    struct MptMeshRow { size_t vert = 0; int nfaces = 0; MptDeformMesh deform; MptSubdivMesh subdiv; };   // a mesh: its first pool vertex, its faces, what the features keep
    enum MptObjDirty : unsigned char {                   // why the next mpt_compose composes an object again
        MPT_OBJ_CLEAN = 0,
        MPT_OBJ_UPLOAD = 1,                              // its record changed on the host: it goes up
        MPT_OBJ_PLACED = 2,                              // an instance whose scatter places: scatter.hip writes its record on the device
        MPT_OBJ_MOVED = 4,                               // an object bound to an object clip (scene_anim.cpp): anim.hip's motion_kernel writes its matrix on the device; or a bound child (hierarchy.hip's kernel does)
        MPT_OBJ_COMPOSE = MPT_OBJ_UPLOAD | MPT_OBJ_PLACED | MPT_OBJ_MOVED,   // any of them
    };
    struct MptObjRow {                                   // an object: what the host alone keeps of it
        int mesh = 0;
        int pose = -1, copy = -1, scatter = -1;          // its rows of deform.poses and subdiv.copies, the scatter it is an instance of (-1: none)
        unsigned char dirty = MPT_OBJ_UPLOAD;            // MptObjDirty flags, cleared by mpt_compose
        int motion = -1;                                 // its row of anim.motions (-1: no object clip has ever moved it)
        int parent = -1, joint = -1;                     // its parent binding (scene_anim.cpp): the object it follows (-1: a root), the joint of that object's pose (-1: the object itself)
        int children = 0;                                // the objects bound to it
    };
    struct MPT_INTERNAL Compose {                        // scene composition on the device (mpt_mesh_add, mpt_object_*, mpt_compose)
        std::vector<MptMeshRow> meshes; size_t pool_verts = 0;
        std::vector<MptComposeObj> objs;                 // the table as the host keeps it (first_face as of the last layout)
        std::vector<MptObjRow> rows;                     // ... and the host's row of each of its objects
        bool relayout = true;                            // objects were added or dropped: the next mpt_compose writes everything
        bool out_valid = false;                          // dmodel holds the last mpt_compose's output (mpt_load_model takes the buffers back)
        int out_objs = 0;                                // ... of this many objects: the rows of bufs.first (objects added since are not in it)
        unsigned epoch = 0;                              // counts the mpt_compose calls (MptComposeObj::epoch)
        MptComposeBufs bufs;
        MappedBuf<float> bounds;                         // {min3, max3} of the composed positions
        mpt_compose_info stats{};
        MptLaunchTimer timer;                            // mpt_compose: {before the compose kernel, after the fold} per call
        explicit Compose(MptEventPool &ev) : timer(2, ev) {}
    } compose{events};
    // The room of derived copies behind the meshes in the pool, as mesh deformation and Loop subdivision each keep it for theirs (a
    // copy is a row with a copy_vert: its first pool vertex, -1 while it has no room).  lay_copies (below) assigns the room
    struct MptCopyRoom {
        size_t copy_verts = 0;                           // pool vertices the copies hold
        bool stale = true;                               // the room is not assigned, or the pool it lay in has gone
        template <class Copies>
        void lose(Copies &copies, bool &relayout) {      // a mesh joined the pool: it lies where the copies lay
            if (copy_verts == 0) return;
            copy_verts = 0; stale = relayout = true;
            for (auto &p : copies) p.copy_vert = -1;
        }
    };
    struct MptDeformPose {                               // a deformable object: its pose as the host keeps it, and its deformed copy
        int obj = 0, mesh = 0;
        std::vector<double> pose;                        // ntargets weights, then njoints x 12: the layout of bufs.pose
        size_t pose_at = 0; long long copy_vert = -1;    // where they lie on the device (copy_vert -1: no room assigned yet)
        bool dirty = true;                               // the pose changed since the copy was written
        int clip = -1;                                   // the clip it is bound to (scene_anim.cpp; -1: none, the pose above goes up): the device evaluates its pose
        double offset = 0.0, speed = 1.0; int loop = 1;  // ... and the binding
        // its second binding: the clip blended in (-1: none), its own offset, speed and loop, the weight's fade
        int clip_b = -1;
        double offset_b = 0.0, speed_b = 1.0; int loop_b = 1;
        double w0 = 1.0, w1 = 1.0, fade_start = 0.0, fade_duration = 0.0;
    };
    struct MPT_INTERNAL Deform {                         // mesh deformation (scene_deform.cpp: mpt_mesh_set_*, mpt_object_set_*, deform_step)
        std::vector<MptDeformPose> poses;
        size_t deltas_used = 0, skin_used = 0;           // floats of bufs.deltas, corners of bufs.joints / weights
        MptCopyRoom room;                                // the deformed copies' room, behind the meshes
        std::vector<MptDeformObj> h_objs;                // the last launch's tables as uploaded: they outlive the copies that read them
        std::vector<MptRun> h_runs;
        MptDeformBufs bufs;
        mpt_deform_info stats{};
        MptLaunchTimer timer;                            // mpt_compose: {before the deform kernel, after it} per launch
        explicit Deform(MptEventPool &ev) : timer(2, ev) {}
    } deform{events};
    struct MptAnimClip { int mesh = 0, ntracks = 0; size_t track_at = 0; double t0 = 0.0, t1 = 0.0; };   // a clip: its mesh (-1: an object clip), its tracks in the arena, its span
    struct MptMotion {                                   // a motion binding: the object, its object clip (-1: unbound, the row is kept for the next binding), the binding
        int obj = 0, clip = -1;
        double offset = 0.0, speed = 1.0; int loop = 1;
        double rest[MPT_ANIM_REST] = { 0, 0, 0, 0, 0, 0, 1, 1, 1, 1 };
        double base[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    };
    struct MPT_INTERNAL Anim {                           // keyframe animation (scene_anim.cpp: mpt_mesh_set_skeleton, mpt_mesh_add_clip, mpt_object_set_animation, mpt_scene_set_time, anim_step)
        std::vector<MptAnimClip> clips;
        size_t joints_used = 0, tracks_used = 0, times_used = 0, values_used = 0;   // elements of the arenas
        int skeletons = 0;
        double time = 0.0;                               // the scene's time
        std::vector<MptAnimObj> h_objs;                  // the last launch's table as uploaded: it outlives the copy that reads it
        std::vector<MptMotion> motions;                  // the motion bindings (an object's row names its own); cleared by mpt_scene_clear
        int moved = 0;                                   // ... of which bound
        std::vector<MptMotionObj> h_moved;               // the last motion launch's table as uploaded
        MptAnimBufs bufs;
        mpt_anim_info stats{};
        int64_t evaluated_blended = 0, evaluated_moved = 0;   // of the last mpt_compose (mpt_anim_blend_stats)
        MptLaunchTimer timer;                            // mpt_compose: {before the anim kernel, after it} per launch
        MptLaunchTimer motion_timer;                     // ... {before the motion kernel, after it}
        // parent bindings (the bindings themselves stand in the objects' rows)
        int bound_children = 0;
        bool order_stale = true;                         // a binding changed since `order` was made
        std::vector<int> order, depth;                   // the bound children by depth, then id; every object's depth (a root: 0)
        int deepest = 0;
        std::vector<MptHierObj> h_hier;                  // the last hierarchy launch's table as uploaded
        mpt_hierarchy_info hier_stats{};                 // of the last mpt_compose
        MptLaunchTimer hier_timer;                       // ... {before the hierarchy kernel's launches, after them}
        explicit Anim(MptEventPool &ev) : timer(2, ev), motion_timer(2, ev), hier_timer(2, ev) {}
    } anim{events};
    struct MptSubdivCopy {                               // a subdivided copy: of a mesh that is not deformable, or of one object of a mesh that is
        int mesh = 0, obj = -1;                          // obj -1: shared by the mesh's objects
        long long copy_vert = -1; size_t work_at = 0;    // where the copy and its workspace lie (copy_vert -1: no room assigned yet)
        bool dirty = true;                               // the control records or the displacement's parameters changed since the copy was written
        unsigned long long image_gen = 0;                // a displaced copy: the image generation it was last displaced at (0: never)
    };
    struct MPT_INTERNAL Subdiv {                         // Loop subdivision (scene_subdiv.cpp: mpt_mesh_set_subdivision, subdiv_step)
        std::vector<MptSubdivCopy> copies;
        size_t topo_used = 0;                            // words of bufs.topo
        MptCopyRoom room;                                // the subdivided copies' room, behind the meshes and the deformed copies
        std::vector<MptSubdivJob> h_jobs;                // the last compose's tables as uploaded: they outlive the copies that read them
        std::vector<MptRun> h_runs;
        MptSubdivBufs bufs;
        mpt_subdiv_info stats{};
        int launches = 0;                                // kernels launched since mpt_subdiv_kernel_time last asked
        MptLaunchTimer refine_timer, normal_timer, emit_timer;   // mpt_compose: {before, after} the refine launches, the normals, the records
        // texture displacement of the copies
        std::vector<MptDisplaceJob> h_djobs;             // as h_jobs
        int64_t displaced_copies = 0, displaced_verts = 0;   // what the last mpt_compose displaced
        int displace_launches = 0;                       // displacement launches since mpt_displace_kernel_time last asked
        MptLaunchTimer displace_timer;                   // mpt_compose: {before, after} the displacement launch
        explicit Subdiv(MptEventPool &ev) : refine_timer(2, ev), normal_timer(2, ev), emit_timer(2, ev), displace_timer(2, ev) {}
    } subdiv{events};
    struct MptScatterRow {                               // a scatter: `count` instances of `mesh` over the surface object `surf`
        int surf = 0, mesh = 0, first_obj = 0, count = 0;
        uint64_t seed = 0;
        mpt_scatter_params par{};                        // as given, `up` at unit length
        int faces = 0;                                   // the surface's faces (an object keeps its count): weights, shares and cdf have faces + 1 entries
        size_t face_at = 0, point_at = 0;                // where they and the sticky records lie in the arenas
        bool select = true;                              // weights, scan and selection are due: a new scatter, mpt_scatter_rescatter, mpt_scatter_set_params
        bool placed = false;                             // the rows of the device's table hold the instances' matrices (mpt_scatter_get)
        // spacing (mpt_scatter_set_spacing): the minimum distance (0: a plain scatter), the candidates, where
        // their states lie in their arena, and what the scatter's last elimination came to (mpt_scatter_get_spacing)
        double min_distance = 0; int64_t candidates = 0; size_t state_at = 0;
        int64_t kept = 0; int32_t rounds = 0;
    };
    struct MPT_INTERNAL Scatter {                        // scatters (scene_scatter.cpp: mpt_scatter_*, scatter_mark, scatter_step)
        std::vector<MptScatterRow> rows;
        size_t faces_used = 0, points_used = 0;          // entries of the arenas
        DevBuf<double> w; DevBuf<uint32_t> q; DevBuf<uint64_t> cdf;   // per face of every scatter's surface (and one entry behind them): weight, share, exclusive scan
        DevBuf<MptScatterPoint> points;                  // the sticky records of every scatter, back to back
        DevBuf<MptScatterJob> jobs; DevBuf<MptRun> runs; // a compose's table of scatters and its three run tables: faces and instances of the selecting ones, instances of the placing ones
        DevBuf<double> part; DevBuf<uint64_t> bsum;      // per workgroup of the weight launch: its largest weight, the sum of its shares
        DevBuf<double> wmax; MappedBuf<double> wmax_host; size_t wmax_cap = 0;   // per scatter: the largest weight, on the device and where the host reads it
        std::vector<MptScatterJob> h_jobs;               // the last compose's tables as uploaded: they outlive the rows that made them
        std::vector<MptRun> h_runs;
        std::vector<unsigned char> selects, places;      // per scatter: what the compose under way does (scatter_mark decides, scatter_step launches)
        mpt_scatter_info stats{};
        int launches = 0;                                // kernels launched since mpt_scatter_kernel_time last asked
        MptLaunchTimer select_timer, place_timer;        // mpt_compose: {before, after} weights + scan + selection, and the placement
        MptLaunchTimer space_timer;                      // ... and, inside the selection's, {before, after} the elimination of the spaced scatters
        struct MPT_INTERNAL Space {                      // the spaced scatters' elimination (scatter_space.hip; space_eliminate)
            size_t states_used = 0;                      // entries of the arena of states that scatters own
            DevBuf<int32_t> state;                       // per candidate of every spaced scatter: undecided, kept or rejected; behind them a door call's
            DevBuf<int32_t> index;                       // beside the sticky records: the candidate each instance came from
            // an elimination's workspace: positions [3] and bucket-sorted items per candidate, cursor and start per bucket, the box
            // partials per workgroup, and its tables
            DevBuf<double> pos, part; DevBuf<int32_t> items; DevBuf<uint32_t> cursor, start;
            DevBuf<MptSpaceJob> jobs; DevBuf<MptSpaceGrid> grids; DevBuf<MptRun> runs;
            MappedBuf<uint32_t> words; size_t words_cap = 0;   // per scatter of an elimination: the last round a lane waited in, then the number kept
            mpt_scatter_spacing_info stats{};            // the last mpt_compose's
        } space;
        explicit Scatter(MptEventPool &ev) : select_timer(2, ev), place_timer(2, ev), space_timer(2, ev) {}
    } scatter{events};
    struct MPT_INTERNAL Refit {                          // mpt_refit_tree (tree_refit.cpp, refit_rule.h)
        int topo = MPT_TOPO_NONE;                        // MptTopoState: do the node records hold a topology, and if not, why not
        int faces = 0; bool on_device = false;           // ... for this many faces, from the device build
        bool linked = false;                             // bin_parent / wide_parent are this build's (made by its first refit)
        DevBuf<int> bin_parent, wide_parent;             // per binary / wide node: the slot of its parent's record its box lives in
        DevBuf<unsigned long long> cost;                 // [2]: the cost kernel's sums, before and after
        uint64_t cost_built = 0, cost_now = 0;           // in units of 2^-40; cost_built is taken by the first refit after a build
        int64_t refits = 0, host_fetches = 0;            // since the build | fetches of the model's host copy refits caused, ever
        MptLaunchTimer timer;                            // {before the refit's kernels, after them} per call
        explicit Refit(MptEventPool &ev) : timer(2, ev) {}
        void lose(int why) { if (topo != MPT_TOPO_NONE) topo = why; }
    } refit{events};
    struct MPT_INTERNAL Query {                          // batch ray queries (tree_query.cpp, query_kernel.hip)
        DevBuf<float> o, d, dis;                         // a chunk's rays on the device: [cap][3], [cap][3], [cap]
        DevBuf<int32_t> avoid;                           // [cap]
        DevBuf<int32_t> out_i; DevBuf<float> out_f;      // its answers: hit | index | object (or occ), depth | u | v, [3][cap] each
        size_t cap = 0;                                  // rays the chunk buffers hold
        DevBuf<int32_t> leaf, slot_of;                   // slot -> face and face -> slot of the tree of build tables_seq
        DevBuf<int> walk_spill;                          // mpt_walk_trace: the spill strip of the 4-wide gather walks, 128 entries per lane of a chunk
        unsigned tables_seq = 0;
        MptLaunchTimer timer;                            // {before a chunk's kernel, after it} per launch
        explicit Query(MptEventPool &ev) : timer(2, ev) {}
        int reserve(size_t rays) {
            if (rays <= cap) return 0;
            cap = 0;
            for (DevBuf<float> *b : { &o, &d, &dis, &out_f }) b->release();
            avoid.release(); out_i.release();
            if (o.reserve(rays * 3) || d.reserve(rays * 3) || dis.reserve(rays) || avoid.reserve(rays) || out_i.reserve(rays * 3) ||
                out_f.reserve(rays * 3)) return 1;
            cap = rays;
            return 0;
        }
    } query{events};
    struct MPT_INTERNAL History {                        // reprojection (film_history.cpp: mpt_history_*); the per-pixel buffers are fb.hist
        bool have = false;                               // a view is kept and not spent: mpt_history_reproject may run
        bool gbuffer = false, motion = false;            // fb.hist holds a kept G-buffer / the motion records of a reproject, of a film of nx x ny
        int nx = 0, ny = 0, faces = 0;                   // the film size and the face count of the kept view
        float v2w[16] = {}, w2v[16] = {};                // its camera, as uploaded
        DevBuf<float> verts;                             // [faces][3][3] the positions it saw
        MappedBuf<mpt_history_stats> stats;              // the counts of the last resample launch
        MptHistoryBufs bufs;                             // mpt_history_eval: the caller's G-buffer and motion records, and what the kernels write (grown on demand)
        MptLaunchTimer keep_timer, reproject_timer;      // {before the call's kernels, after them} per call
        explicit History(MptEventPool &ev) : keep_timer(2, ev), reproject_timer(2, ev) {}
        void forget() { have = gbuffer = motion = false; }
    } history{events};
    MptDoorInput door;                                  // mpt_display_eval, mpt_noise_eval, mpt_denoise_eval: the caller's accumulators on the device (grown on demand)
    MptLaunchTimer render_timer{2, events};              // PathEngine launches: {kernel start, kernel end}
    MptLaunchTimer denoise_timer{2, events};             // mpt_get_denoised: {before the prologue, after the epilogue} per call
    float denoise_variance = 0.0f;                       // mpt_denoise_set_variance: sigma_variance of the denoised read-backs (0: the fixed filter)
    MptDenoiseBufs denoise_bufs;                         // mpt_denoise_eval: the filter's buffers for the caller's accumulators (grown on demand)
    MptLaunchTimer brute_timer{2, events};               // brute-force engine: {kernel start, kernel end} per launch
    int pending = 0;                                     // command batching: frames enqueued and not launched yet

    MptRingSlot ring[MPT_MAX_PIPE];
    MptStream probe_stream;                           // mpt_probe_kernel
    MptStream stress_stream;                          // mpt_stress_copies: a stream of device-to-device copies beside the render
    DevBuf<char> stress_buf; size_t stress_bytes = 0;   // 2 x stress_bytes
    MptStream aux;                                    // Sobol advances + queue resets of the pipelined batches
    int cur_depth = 2, cur_div = 1;                   // what the last launch used
    MptEvent ev_film;                                 // main-stream work on the film (combine, clear, gather) a finalising launch must see
    // tail finalisation (render_kernel.hip finalise_tiles, option "finalise"): launch_seq numbers the launches (slab tags);
    // film_version counts the changes of pass 0
    unsigned launch_seq = 0;
    unsigned tag_epoch = 0;                           // launch_seq / MPT_TAG_PERIOD when the slabs were last zeroed
    unsigned tag_wraps = 0;                           // times the slab tags came round (every slab zeroed): a test reads it
    unsigned long long film_version = 0;
    // the early image: hint = where the next mpt_get_image(0) wants the image (mpt_hint_image); ptr = the image a finalising
    // launch has written (or is writing), with the stream of that launch and the film version it shows
    struct { float *hint = nullptr, *ptr = nullptr; hipStream_t stream = nullptr; unsigned long long version = 0; } early;
    int last_finalised = 0;                           // the last launch finalised its tiles itself (diagnostics, option "last_finalised")
    MptEvent ev_main;                                 // main-stream work a render must see (uploads, resets, ...)
    bool main_dirty = true;
    int flip = 0;
    // Sobol points of the NEXT batch, computed ahead of time into the ring slot it will use (the sequence is
    // deterministic): valid while nothing has touched the sampler or the ring since; X = the sampler state that batch will leave
    // behind (swapped with sX when it is launched)
    struct { bool valid = false; int slot = -1, B = 0; int32_t time = 0; DevBuf<int> X; } spec;

    // measurement
    DevBuf<unsigned long long> d_timeline;
    int timeline_waves = 0;
    DevBuf<unsigned long long> d_counters;
    MappedBuf<unsigned int> watchdog;                            // raised by a render kernel's watchdog
    PinnedBuf<char> h_stage;                                     // page-locked staging (h_stage.cap bytes) for read-backs into pageable buffers

    // comm
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    DevBuf<double> d_scratch;
    // film gather of a striped split (comm.cpp): the share packed into one message per peer
    DevBuf<MptVec4> gather_buf;                              // sender: its packed share; root: every peer's, back to back
    DevBuf<MptPiece> d_pieces;                               // the plan's piece table on the device
    int plan_key[6] = { -1, -1, -1, -1, -1, -1 };            // (nx, ny, stripe_w, R, rank, root) the table was made for
    int plan_npieces = 0; long long plan_max_count = 0;
};

// entry checks of the API calls (miptina.cpp)
MPT_INTERNAL int use_ro(mpt_ctx *c);   // calls that only read results
MPT_INTERNAL int use(mpt_ctx *c);      // calls that may change what the next render launch reads
MPT_INTERNAL int check_watchdog(mpt_ctx *c);   // after a synchronise: did a persistent kernel give up?
// what the read-backs (film_read.cpp) take from miptina.cpp, beside mpt_flush
MPT_INTERNAL int read_back(mpt_ctx *c, void *out, const void *dev, size_t bytes);   // device -> caller buffer on the main stream, blocking
MPT_INTERNAL void *caller_alias(const mpt_ctx *c, void *p, size_t bytes);           // the device alias of a page-locked caller array of ours, or null
MPT_INTERNAL int timer_readout(mpt_ctx *c, MptLaunchTimer &timer, double *ms0, double *ms1, int *launches, bool render_streams = false);
// what the engines that launch at the call (engines.cpp) and the test door of the device functions (measure.cpp) take from it
MPT_INTERNAL int render_entry(mpt_ctx *c, int nframes);                          // null context, nframes < 0, "not set up yet": fails at the call
MPT_INTERNAL int fill_params(mpt_ctx *c, MptRenderParams &p, int nframes);       // the launch parameters of a batch of nframes frames
MPT_INTERNAL void fill_t_scale(const mpt_ctx *c, MptRenderParams &p, const float *o, int n);   // ... p.t_scale / t_unscale: for the camera, surfaces and n more origins
MPT_INTERNAL int fill_scene_params(mpt_ctx *c, MptRenderParams &p);              // ... the part that describes lights, world light, camera, materials and images
// the sampler moves by `count` frames; the points of the last `keep` go to P[0 .. keep) (default: the main stream, c->sP)
MPT_INTERNAL int sobol_advance(mpt_ctx *c, int count, int keep, hipStream_t stream = nullptr, float *P = nullptr);
// levels of the per-lane traversal stack of the kernels that gather the binary tree, by the tree the context's build walks
inline int gather_stack_levels(const mpt_ctx *c) { return mpt_gather_stack_levels(c->opt.mode == MPT_MODE_FAST ? c->fast_depth : c->tree_depth); }

// engines.cpp
MPT_INTERNAL int mlt_flush(mpt_ctx *c);       // mpt_flush, mpt_render: launch the Metropolis iterations enqueued so far

// tree_build.cpp
MPT_INTERNAL int download_tree(mpt_ctx *c);   // before anything reads c->h_leaf / h_child / ...: fetch the reference-layout arrays once per build

// tree_query.cpp
MPT_INTERNAL int query_tables(mpt_ctx *c);    // before a launch reads c->query.leaf / slot_of: slot -> face and face -> slot of the tree as built

// scene_compose.cpp
MPT_INTERNAL int model_on_host(mpt_ctx *c);  // before anything reads c->verts / c->mtlids: fetch them once if mpt_compose made the model
// ... and what the other scene files take from it.  The checks of a mesh or an object argument word their refusal with "who: " in
// front, or bare where who is null
MPT_INTERNAL int check_mesh(const mpt_ctx *c, int mesh_id, const char *who);
MPT_INTERNAL int check_object(const mpt_ctx *c, int obj_id, const char *who);
MPT_INTERNAL int check_fresh_mesh(const mpt_ctx *c, int mesh_id, const char *who);   // the mesh argument of the mpt_mesh_set_* calls: a mesh of the pool, without an object yet
MPT_INTERNAL int fetch_mesh(mpt_ctx *c, int mesh_id, std::vector<float> &rec);       // the mesh's records [face][3][8] as the pool holds them; the stream is idle behind it
// The one place an object is added: its record of the table (world null: the identity, an instance's placeholder), its host row, and
// through deform_object_added and subdiv_object_added its pose and its copy.  Returns its id
MPT_INTERNAL int add_object(mpt_ctx *c, int mesh_id, const double *world, int mtlid, int scatter);
// the read-back of a copy of `k` faces that lies at copy_vert: `noun` names the copies, `mesh` what has the k faces
MPT_INTERNAL int read_copy(mpt_ctx *c, long long copy_vert, bool stale, int k, int obj_id, float *verts, int cap_faces, const char *who,
                           const char *noun, const char *mesh);

// The room of a list of copies (rows with a copy_vert), laid out back to back from pool vertex `base`; verts_of(copy) is a copy's
// vertices.  Refuses a pool past 2^31 - 1 vertices (MptComposeObj::mesh_vert) and grows the pool, keeping what lies below `base` --
// for the subdivided copies that includes the deformed ones, and it is this grow_pool that waits for the queued deform launch.
// The caller points the objects' mesh_vert at the copies (the table changes: all of it goes up, relayout) and clears room.stale
// once the copies' side arenas have their room too
template <class Copies, class VertsOf>
inline int lay_copies(mpt_ctx *c, mpt_ctx::MptCopyRoom &room, Copies &copies, size_t base, VertsOf verts_of, const char *noun) {
    size_t at = base;
    for (auto &p : copies) at += verts_of(p);
    if (at > 0x7fffffffu) return fail("mesh pool full: %zu vertices with the %s copies", at, noun);
    if (c->compose.bufs.grow_pool(at * 8, base * 8, c->stream)) return 1;
    at = base;
    for (auto &p : copies) { p.copy_vert = (long long)at; at += verts_of(p); }
    room.copy_verts = at - base;
    c->compose.relayout = true;
    return 0;
}

// scene_deform.cpp: what add_object and mpt_scene_clear tell the deform table, and the step of mpt_compose that writes the deformed copies
MPT_INTERNAL void deform_object_added(mpt_ctx *c, int obj_id);   // (called by add_object alone, as subdiv_object_added behind it)
MPT_INTERNAL void deform_scene_cleared(mpt_ctx *c, int meshes);
MPT_INTERNAL int deform_step(mpt_ctx *c);                        // before compose_kernel: room, poses, the deform launch; rewrites objs' mesh_vert at a relayout

// scene_anim.cpp: what mpt_scene_clear tells keyframe animation, and what deform_step asks of it
MPT_INTERNAL void anim_scene_cleared(mpt_ctx *c, int meshes);    // the bindings go with the poses (scene_deform.cpp); skeletons and clips go with the meshes
MPT_INTERNAL void hierarchy_mark(mpt_ctx *c);                    // at the head of mpt_compose: a dirty parent, or a dirty pose under a joint binding, marks its children MPT_OBJ_MOVED, level by level
MPT_INTERNAL int hierarchy_step(mpt_ctx *c);                     // inside mpt_compose, behind motion_step and in front of scatter_step: the bound children's matrices
MPT_INTERNAL int motion_step(mpt_ctx *c);                        // inside mpt_compose, behind the table's upload and in front of scatter_step: the moved objects' matrices
MPT_INTERNAL int anim_step(mpt_ctx *c, const std::vector<int> &poses);   // inside deform_step, before the deform launch: evaluates these rows of deform.poses (bound objects) on the device

// scene_subdiv.cpp: what scene_compose.cpp and scene_deform.cpp tell the subdivision table, and the step of mpt_compose behind deform_step
MPT_INTERNAL int subdiv_object_faces(const mpt_ctx *c, int mesh_id);   // the faces an object of this mesh has: k * 4^L (Catmull-Clark: 2 quads' worth per quad of level L)
MPT_INTERNAL void subdiv_object_added(mpt_ctx *c, int obj_id);
MPT_INTERNAL void subdiv_pose_changed(mpt_ctx *c, int obj_id);   // mpt_object_set_morph_weights / mpt_object_set_joints
MPT_INTERNAL void subdiv_scene_cleared(mpt_ctx *c, int meshes);
MPT_INTERNAL int subdiv_images_ready(mpt_ctx *c);                // before deform_step: a displaced copy that will be displaced has its image loaded, else mpt_compose refuses and changes nothing
MPT_INTERNAL int subdiv_step(mpt_ctx *c);                        // behind deform_step: room, the launches; rewrites objs' mesh_vert at a relayout

// scene_scatter.cpp: what scene_compose.cpp tells the scatters, and their steps of mpt_compose
MPT_INTERNAL void scatter_scene_cleared(mpt_ctx *c);             // the scatters go with the objects
MPT_INTERNAL int scatter_ready(mpt_ctx *c);                      // before deform_step: a surface has faces, a density image that will be sampled is loaded, else mpt_compose refuses and changes nothing
MPT_INTERNAL bool scatter_selection_due(const mpt_ctx *c);       // ... and will the compose under way select (and so may refuse a surface without weight)?
MPT_INTERNAL void scatter_mark(mpt_ctx *c);                      // behind subdiv_step: which scatters select and place; flags their instances MPT_OBJ_PLACED
MPT_INTERNAL int scatter_step(mpt_ctx *c);                       // behind the table's upload, before compose_kernel: the launches

// film_read.cpp
MPT_INTERNAL int check_pass(mpt_ctx *c, int pass);

// comm.cpp
MPT_INTERNAL void mpt_comm_release(mpt_ctx *c);   // mpt_destroy: drop the communicator, if any


/*
 * miptina.h -- C ABI of libmiptina.so, the MI355X (gfx950) path-trace hot path that sits
 * underneath PTina's Python object API.
 *
 * The reference (archibate/ptina) has no FFI of its own: the path is reached through Python
 * singletons whose flattest statement is ptina/worker.py:11-87.  Each entry point below names
 * the reference call it replaces (file:line relative to the reference tree); the Python
 * package ptina_amd binds them with ctypes and keeps the reference's class and method names.
 *
 * Conventions
 *   - plain C types only; every pointer is a host pointer borrowed for the duration of the
 *     call (inputs are copied to the device, outputs are written into caller buffers);
 *   - functions return 0 on success, non-zero on error; mpt_last_error() gives the message
 *     (the Python layer raises RuntimeError with it, as the reference raises);
 *   - a context is NOT re-entrant: one caller thread per context (the reference funnels
 *     every call through one thread, ptina/tools/mtworker.py:22-42);
 *   - mpt_render* only ENQUEUE work (the reference's kernel launches are asynchronous too);
 *     the read-backs and mpt_synchronize block.  Consecutive mpt_render calls are batched
 *     into one launch at the next flush point.
 */
#ifndef MIPTINA_H
#define MIPTINA_H

#include <stddef.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpt_ctx mpt_ctx;

/* capacities, ptina/things.py:12-19 (init_things keyword arguments) */
typedef struct {
    int32_t max_faces;       /* 2^21 */
    int32_t max_texels;      /* 2^22 */
    int32_t max_materials;   /* 2^6  */
    int32_t max_textures;    /* 2^6  */
    int32_t max_lights;      /* 2^6  */
    int32_t max_filmsize;    /* 2^21 */
    int32_t max_filmpasses;  /* 3    */
} mpt_caps;

/* work counters of the traversal actually run (for the roofline's algorithmic bytes) */
typedef struct {
    uint64_t samples;        /* camera samples traced                    */
    uint64_t rays;           /* BVH traversals (closest-hit + shadow)    */
    uint64_t n_box;          /* box tests                                */
    uint64_t n_tri;          /* triangle tests                           */
    uint64_t n_shade;        /* shaded hits                              */
    uint64_t n_draws;        /* Sobol draws                              */
    uint64_t bounces;        /* path-loop iterations                     */
    uint64_t n_node;         /* internal-node records fetched            */
    uint64_t it_node;        /* wave-level NODE steps issued (n_node / (64 it_node) = lane utilisation) */
    uint64_t it_leaf;        /* wave-level LEAF steps issued             */
    uint64_t it_shade;       /* wave-level SHADE stages issued           */
    uint64_t it_new;         /* wave-level NEW stages issued             */
    /* spare counters: zero in the product library; the diagnostic build -DMPT_X_STAMPS=2 fills them with the cycles of the
     * segments of SHADE (render_shade.h; read by tools/gpu_diag.py stamps) */
    uint64_t pl_local;
    uint64_t pl_batches;
    uint64_t pl_batch_lanes;
    uint64_t pl_prim;
    uint64_t pl_tidle;
    uint64_t pl_sidle;
    uint64_t pl_trips;
    uint64_t pl_taken;
} mpt_counters;

#define MPT_LIGHT_POINT 1    /* LightPool.TYPES, ptina/light/__init__.py:11 */
#define MPT_LIGHT_AREA  2

/* render modes (mpt_set_option "mode") */
#define MPT_MODE_FAST   0    /* ordered, depth-culled traversal; any-hit shadow rays; FMA + native rcp/sin/cos */
#define MPT_MODE_STRICT 1    /* the reference's traversal order and IEEE arithmetic without contraction        */

const char *mpt_last_error(void);
int  mpt_device_count(void);
int  mpt_version(void);

/* init_things(), ptina/things.py:12-28 */
mpt_ctx *mpt_create(const mpt_caps *caps, int device);
void mpt_destroy(mpt_ctx *ctx);

/* Options of a context.  mpt_set_option first launches the frames enqueued so far, which render with the options they were enqueued
 * under; it refuses a value outside the domain ("<key> must be <domain>") and a key it does not know ("unknown option '<key>'") and
 * then leaves the context as it was.  mpt_get_option reads every key below; it launches and waits for nothing.
 * One entry per key -- default; domain; meaning.  "flag": any int is taken, non-zero is stored (and read back) as 1.
 * Settable -- what a render launch reads:
 *   "mode"            0; 0, 1; MPT_MODE_FAST / MPT_MODE_STRICT: which build of the kernels renders
 *   "batch"           32; 1..64; most frames per launch
 *   "chunk"           0; >= 0; frames per work item, 0 = auto
 *   "count"           0; flag; 1 = accumulate mpt_counters (slower)
 *   "lds"             1; flag; 1 = use the LDS-resident persistent kernel when the scene fits a CU's 160 KiB LDS, 0 = always gather from
 *                     HBM/L2
 *   "lds_wide"        1; 0, 1; what that kernel walks: 1 = the 4-wide nodes with exact boxes, 112 bytes apart in LDS -- needs "wide" = 1;
 *                     0 = the binary nodes; the same film up to ties between equally distant hits
 *   "lds_block"       0; 0, 256, 512, 768, 1024; lanes per persistent workgroup of the LDS kernel, 0 = auto (diagnostics)
 *   "wide"            1; flag; scenes that do not fit LDS: 1 = walk the fast tree collapsed into 4-wide nodes, 0 = the binary tree
 *   "wide_quant"      1; flag; 1 = the 4-wide nodes as 64-byte records with 8-bit child boxes rounded outwards: four gathers per step;
 *                     0 = 128-byte records with the exact boxes: seven
 *   "shade_spec"      1; 0, 1; 1 = a scene whose feature mask is empty (no clearcoat, no transmission, no texture) runs the plain
 *                     instantiation of the LDS 4-wide kernel's SHADE, 0 = always the generic one (A/B, tests); same film bit for bit
 *   "skip_dark"       -1; -1..1; 1 = a shadow ray whose candidate direct light is exactly zero -- the light behind the surface -- is not
 *                     traced: adding zero or not is the same sum; 0 = traced like the reference does; -1 = on in the production build,
 *                     off in the strict build
 *   "tile_w_shift"    3; 0..3; a work item's tile is 2^w pixels wide ...
 *   "tile_h_shift"    3; 0..3; ... and 2^h high
 *   "pipe_depth"      0; 0, 2..6; batches in flight, 0 = auto
 *   "grid_div"        0; 0..8; each launch takes 1/G of the CUs so that G launches are resident in different phases; 0 = choose by
 *                     samples per lane, and the whole chip for a launch that finds nothing else in flight
 *   "reserve_cus"     0; 0..num_cus - 1; CUs every persistent render launch leaves unclaimed; measured to be of no use to foreign
 *                     kernels while launches overlap, kept for experiments
 *   "finalise"        1; 0..2; 1 = a render launch that finds no other launch in flight adds its frames to the film, resolves and writes
 *                     out finished tiles itself while its last paths drain; 2 = the same without the early image (A/B); 0 = always the
 *                     combine pass after the launch; same film bit for bit
 * -- read-backs:
 *   "zero_copy"       1; flag; 1 = mpt_get_image into an mpt_host_alloc array has the resolve pass write the image straight into it
 *                     over PCIe; 0 = device buffer + DMA -- same image, 20 us more per call
 *   "spin_us"         20000; >= 0; how long mpt_get_image polls a finalising launch before it blocks, 0 = block at once
 *   "denoise_lds"     1; flag; 1 = mpt_get_denoised's iterations of stride 1 and 2 filter from a tile held in LDS; 0 = every stride
 *                     gathers from memory -- same image bit for bit
 * -- what mpt_build_tree reads.  These leave a built tree invalid (rendering fails with "BVH not built" until the next
 *    mpt_build_tree): the first four when the stored value changes, the last three at every set, even of the same value:
 *   "tree"            1; 0, 1; fast build: 1 = SAH re-partition of the LBVH's leaves, 0 = walk the LBVH itself
 *   "gpu_build"       1; flag; 1 = LBVH built on the device, 0 = on the host
 *   "sah_build"       -1; -1..1; where the SAH re-partition runs: 1 = on the device, binned above 32 triangles and exact below; 0 = host
 *                     pass, exact up to "sah_exact_max"; -1 = auto: the device above 8192 faces, the host pass up to there
 *   "wide_build"      1; flag; 1 = the 4-wide collapse runs on the device, 0 = host pass over downloaded records: same bytes
 *   "sah_max"         4194304 (2^22); any int; faces above which the fast build walks the LBVH itself
 *   "sah_exact_max"   8192; >= 2; host SAH pass: ranges up to this many leaves are swept exactly, larger ones binned (diagnostics)
 *   "sah_inject_fail" 0; flag; test door: 1 = treat the device SAH pass as failed after it ran, so that the host pass takes over
 * -- diagnostics:
 *   "timeline"        0; flag; 1 = record mpt_get_timeline data
 *   "lane_hist"       0; flag; 1 = counting kernels ("count" = 1) fill the lane histogram (mpt_get_lane_hist)
 *   "build_phases"    0; flag; 1 = mpt_build_tree synchronises at the end of every phase and times it (read-only keys below)
 *   "launch_seq"      0; >= 0; test door, state rather than an option: the number of the next render launch minus one (its slab tag
 *                     is 2 + number mod 65534), so that a test can walk the launches across the point where the tags come round;
 *                     reads back masked to 31 bits
 * Read-only -- the last build:
 *   "tree_depth"      depth of the reference LBVH (strict build)
 *   "fast_depth"      depth of the tree the fast build walks (SAH or LBVH)
 *   "wide_nodes"      nodes of the 4-wide tree, 0 = not built (too deep)
 *   "wide_depth"      its depth
 *   "wide_stack"      stack levels a traversal of the 4-wide tree can ask for
 *   "wide_ratio_permille"  expected fetches per ray, 4-wide / binary, in thousandths (surface-area sums)
 *   "sah_fallback"    the device SAH pass gave up (1 = error, 2 = depth) and the host pass ran; 0 = not
 *   "build_phase_us_N"  N = 0..5, with "build_phases" = 1: microseconds (host clock) of upload | LBVH | SAH pass | triangle records |
 *                     4-wide collapse | total
 *   "sah_levels"      what the last device SAH pass did (diagnostics): binned levels
 *   "sah_kelems"      positions streamed, summed over the binned levels, in thousands
 *   "sah_chunks"      chunks, summed over the binned levels
 *   "sah_segments"    segments, summed over the binned levels
 *   "sah_part_kwords" words of chunk bins written, summed over the levels, in thousands
 *   "sah_tasks_small" ranges finished in LDS of up to 512 triangles
 *   "sah_tasks_big"   ... and of 513 to 1024
 *   "sah_t_sort_k"    the finish kernels' time in units of 1024 clock ticks: summed over the tasks in the sort,
 *   "sah_t_loop_k"    ... in the level loop,
 *   "sah_t_max_k"     ... and the longest task
 *   "sah_task_levels" levels the tasks ran, summed
 *   "sah_task_levels_max"  ... and the most of one task
 * -- the last launch:
 *   "pending"         frames enqueued and not yet launched
 *   "last_kernel"     0 = gather over the binary tree, 1 = LDS-resident over the binary nodes, 2 = gather over 4-wide nodes, 5 = LDS-
 *                     resident over the 4-wide nodes; 3 and 4 are retired numbers of kernels since removed and never returned
 *   "cur_div"         the ring the last launch belonged to: G launches of 1/G of the CUs,
 *   "cur_depth"       that many batches in flight
 *   "last_div"        what the last launch really took: 1 when it found the ring idle, else cur_div
 *   "last_finalised"  1 = the last launch finalised its tiles itself ("finalise")
 *   "tag_wraps"       times the slab tags came round and every slab was zeroed ("launch_seq")
 *   "scene_feat"      the scene's feature mask as loaded
 *   "shade_inst"      the mask the last render launch was compiled for (0 plain, 31 generic; -1: none yet)
 * -- the device and the process:
 *   "num_cus"         compute units of the device
 *   "clock_khz"       its peak shader clock
 *   "device"          the device the context was created on
 *   "nranks"          size of the communicator, 1 without one,
 *   "rank"            and this context's rank in it
 *   "hw_queues"       GPU_MAX_HW_QUEUES as the HIP runtime was asked for it -- the library requests 12 at load time unless the variable
 *                     is set; NEGATIVE when that request came after a preloaded profiler tool may already have initialised HIP */
int mpt_set_option(mpt_ctx *ctx, const char *key, int value);
int mpt_get_option(mpt_ctx *ctx, const char *key, int *value);

/* FilmTable.set_size / nx,ny, ptina/filmtable.py:41-42,16-24; worker.set_size/get_size, worker.py:29-34 */
int mpt_set_size(mpt_ctx *ctx, int nx, int ny);
int mpt_get_size(mpt_ctx *ctx, int *nx, int *ny);
/* multi-GPU: this context renders film columns x in [x0, x1) only (no reference counterpart) */
int mpt_set_slab(mpt_ctx *ctx, int x0, int x1);
/* Deal the film out in stripes of `width` columns (a multiple of 16): this context renders stripes index,
 * index + modulo, ...  The multi-GPU split with even load; mpt_comm_gather_film follows it when every
 * rank r of R called mpt_set_stripes(width, r, R).  mpt_set_slab / mpt_set_size return to one slab. */
int mpt_set_stripes(mpt_ctx *ctx, int width, int index, int modulo);

/* ModelPool.from_numpy, ptina/model.py:54-60: verts [3n][8] = pos3 nrm3 uv2, mtlids [n] or NULL (= -1) */
int mpt_load_model(mpt_ctx *ctx, const float *verts, const int32_t *mtlids, int n);
/* MaterialPool.load, ptina/mtllib.py:58-77: fac [m][12][4], tex [m][12] (-1 = none) */
int mpt_load_materials(mpt_ctx *ctx, const float *fac, const int32_t *tex, int m);
/* ImagePool.load / load_one, ptina/image.py:69-96: rgba [nx][ny][4] f32; returns image id via *id */
int mpt_reset_images(mpt_ctx *ctx);
int mpt_load_image(mpt_ctx *ctx, const float *rgba, int nx, int ny, int *id);
/* BVHTree.build, ptina/tree/lbvh.py:297-305 */
int mpt_build_tree(mpt_ctx *ctx);
/* test/inspection: reference-layout tree arrays (tree/lbvh.py:48-56); any pointer may be NULL */
int mpt_get_tree(mpt_ctx *ctx, int32_t *child /*[n-1][2]*/, int32_t *leaf /*[n]*/,
                 float *bmin /*[n-1][3]*/, float *bmax /*[n-1][3]*/, int32_t *mc /*[n]*/, int32_t *depth);

/* test/inspection: the 4-wide records the gather kernels walk (no reference counterpart): wnode [nw][8][4] f32 with the exact
 * child boxes, qnode [nw][4][4] with 8-bit boxes; any pointer may be NULL; *nw = wide nodes built (0: none) */
int mpt_get_wide(mpt_ctx *ctx, float *wnode, float *qnode, int cap_nodes, int *nw);

/* test/inspection: the node and triangle records the kernels of both builds fetch, as they lie on the device (no reference
 * counterpart), for a model of n faces: snode [n-1][2][4] f32 {bmin, child0} {bmax, child1}; fnode [n-1][4][4], three rows
 * {lo0, lo1, hi0, hi1} and an id row {id0, id1, -, -} (id >= 0: a node, id < 0: leaf slot ~id); tgeo, tshade [n][4][4] and tfast
 * [n+1][3][4] by leaf slot (record n of tfast: every word 0xffffffff).  Any pointer may be NULL; *nfaces = n, always.  A
 * non-NULL array with cap_faces < n fails before anything is copied; so does a tree that is not built for the model as it
 * stands, or an array the context does not hold.  n = 0 and n = 1 have no node records.  Changes nothing a render, a refit or
 * a query reads. */
int mpt_get_records(mpt_ctx *ctx, float *snode, float *fnode, float *tgeo, float *tshade, float *tfast, int cap_faces, int *nfaces);

/* Pure sizing rule of the on-device SAH re-partition's workspace (no context, no GPU; the reference has no counterpart: its
 * tree is the LBVH of ptina/tree/lbvh.py:297-305).  For a model of n faces: out[0] = segments a level can hold, out[1] = words
 * of per-segment workspace the build allocates, out[2] = words a level of `nseg` segments writes, out[3] = bins per axis at
 * that level.  The build is sound iff out[2] <= out[1] for every nseg <= out[0]; returns 0, or 1 for n < 1 / nseg < 0. */
int mpt_sah_workspace(int n, int64_t nseg, int64_t out[4]);

/* Camera.set_perspective, ptina/camera.py:19-22: the two f32 matrices the reference stores
 * (V2W = inv(pers) computed by the caller in f64 exactly as the reference does) */
int mpt_set_camera(mpt_ctx *ctx, const float v2w[16], const float w2v[16]);

/* LightPool.clear / add, ptina/light/__init__.py:31-49 (pos/axes already extracted from the world matrix) */
int mpt_clear_lights(mpt_ctx *ctx);
int mpt_add_light(mpt_ctx *ctx, int type, const float color[3], const float pos[3],
                  const float axes[9], float size, int *index);
/* WorldLight.set, ptina/light/world.py:18-20 */
int mpt_set_world_light(mpt_ctx *ctx, const float fac[4], int tex);

/* SobolSampler.__init__ / reset / update, ptina/sampling/sobol.py:75-105.
 * V = direction-number grid [rows][dim] (bit pattern, i32) from calc_sobol_vgrid */
int mpt_sobol_init(mpt_ctx *ctx, const int32_t *V, int rows, int dim);
int mpt_sobol_reset(mpt_ctx *ctx, int skip);
int mpt_sobol_update(mpt_ctx *ctx, int count);
int mpt_sobol_get(mpt_ctx *ctx, int32_t *X, float *P, int32_t *time);

/* PathEngine.render, ptina/engine/path.py:75-77 : nframes x (Sobol update + one sample per pixel) */
int mpt_render(mpt_ctx *ctx, int nframes);
/* PreviewEngine.render, ptina/engine/preview.py:18-41 : albedo -> pass 1, normal -> pass 2 */
int mpt_render_preview(mpt_ctx *ctx, int nframes);
/* MLTPathEngine, ptina/engine/mltpath.py (Metropolis light transport over the path integrator; single GPU: a slab / stripe
 * split or a communicator makes mpt_mlt_render fail).  Its ti.random() is a stateless hash of (seed, chain, iteration, slot)
 * here (ptina_amd/csrc/mlt_kernel.hip), so runs repeat bit for bit.
 * reset, mltpath.py:31-37: nchains chains of 32 dims, X_old = random(), L_old = 0, iteration counter 0 */
int mpt_mlt_reset(mpt_ctx *ctx, int nchains, uint32_t seed);
/* LSP[None] / Sigma[None], mltpath.py:18-27 (defaults 0.25 / 0.01) */
int mpt_mlt_set_param(mpt_ctx *ctx, float lsp, float sigma);
/* render, mltpath.py:85-87 x iterations: each chain proposes, traces, splats (w += 1) into film pass 0 and accepts or rejects.
 * Enqueued; consecutive calls are fused into one launch at the next read-back, like mpt_render's frames */
int mpt_mlt_render(mpt_ctx *ctx, int iterations);
/* Test doors: the chain state (X [nchains][32] = X_old, L [nchains][3] = L_old, the number of iterations done); set_state
 * makes the given vectors current */
int mpt_mlt_get_state(mpt_ctx *ctx, float *X, float *L, int *iteration);
int mpt_mlt_set_state(mpt_ctx *ctx, const float *X, const float *L, int iteration);
/* Test door: camera + path_trace (mltpath.py:66-69) of n given 32-vectors by the context's build; rgb [n][3] */
int mpt_mlt_trace(mpt_ctx *ctx, const float *X, float *rgb, int n);
/* HIP-event times (ms) of the chain kernels and of the splat passes launched since the last call, and their launch count */
int mpt_mlt_kernel_time(mpt_ctx *ctx, double *chain_ms, double *splat_ms, int *launches);
/* BruteEngine.render, ptina/engine/brute.py:24-26 x nframes : the walk of path_trace with no light sampling and no MIS (a light
 * counts only when a bounce ray hits it; one random3 per bounce; loop head throughput > 1e-6), one sample per pixel and frame
 * into film pass 0 with weight 1, on the Sobol sampler mpt_render and mpt_render_preview advance.  Launched at the call (not
 * deferred), behind every frame and Metropolis iteration enqueued before it: all three add to the film in call order.  Honours
 * mpt_set_slab / mpt_set_stripes as mpt_render_preview does.  For testing: see DESIGN.md section 3.8 */
int mpt_render_brute(mpt_ctx *ctx, int nframes);
/* HIP-event time (ms) of the brute-force kernels launched since the last call, and their launch count */
int mpt_brute_kernel_time(mpt_ctx *ctx, double *ms, int *launches);
/* launch everything enqueued so far (does not wait) */
int mpt_flush(mpt_ctx *ctx);
/* worker.synchronize, ptina/worker.py:17-18 */
int mpt_synchronize(mpt_ctx *ctx);

/* FilmTable.clear, ptina/filmtable.py:44-45 (zeroes every pass, whatever `pass` says, as the reference does) */
int mpt_clear(mpt_ctx *ctx, int pass);
/* FilmTable.get_image, ptina/filmtable.py:47-63 : out [nx][ny][4] */
int mpt_get_image(mpt_ctx *ctx, int pass, float *out);
/* Advice, optional (the reference's get_image allocates its array inside the call, filmtable.py:48; this says beforehand where
 * that array will be): the next mpt_get_image(pass, out) will be given THIS `out` (a buffer of mpt_host_alloc, [nx][ny][4]).
 * A render launch that finalises its own tiles (option "finalise") then also writes the resolved image there while it drains,
 * and that mpt_get_image only waits for the launch.  Results never depend on it: a different pointer, a film that has changed
 * since, or no hint at all take the resolve pass.  `out` must stay allocated until mpt_get_image(pass, out) has returned or
 * another hint (NULL = none) has replaced it; only pass 0 is used. */
int mpt_hint_image(mpt_ctx *ctx, int pass, float *out);
/* FilmTable.fast_export_image, ptina/filmtable.py:66-79 : out [ny*nx*3] */
int mpt_fast_export_image(mpt_ctx *ctx, int pass, float *out);
/* raw accumulators [nx*ny][4] (rgb sums, sample count) */
int mpt_get_film_raw(mpt_ctx *ctx, int pass, float *out);
/* device-side resolve only (no read-back): what get_image does before the copy */
int mpt_resolve(mpt_ctx *ctx, int pass);

/* Film pass 0 denoised on the device by an edge-avoiding A-Trous wavelet filter (Dammertz et al. 2010), guided by the albedo and
 * normal passes (1 and 2) that PreviewEngine renders (ptina/engine/preview.py:18-41; the reference exports them as denoiser AOVs and
 * leaves the filter to Blender's compositor, so the call has no counterpart there).  With F0, F1, F2 the raw accumulators of the
 * passes (film index x*ny + y):
 *   valid(p) = F0.w != 0;  c = F0.rgb / F0.w;  a = F1.rgb / F1.w, n = F2.rgb / F2.w (0 where that pass is empty);
 *   m = max(a, 1e-2) per channel when `demodulate`, else 1;  e_0 = c / m;  h = [1/16, 1/4, 3/8, 1/4, 1/16];
 *   for i = 0 .. iterations-1, s = 2^i, every valid p, over dx, dy in -2..2 with q = p + s (dx, dy) inside the film and valid:
 *       w(q) = h[dx] h[dy] exp(-(|e_i(p)-e_i(q)|^2 / (sigma_color 2^-i)^2 + |a(p)-a(q)|^2 / sigma_albedo^2 + |n(p)-n(q)|^2 / sigma_normal^2))
 *       e_{i+1}(p) = sum w e_i(q) / sum w
 *   out = (e_final m, 1) for valid pixels and (0.9, 0.4, 0.9, 0) for the others, as mpt_get_image gives them.
 * f32 arithmetic, a gather without atomics: repeats bit for bit.  iterations = 0 is exactly mpt_get_image(ctx, 0, out).  With passes
 * 1 and 2 empty the filter is guided by colour alone.  Columns a slab or stripe split did not render are not valid.  Flushes what is
 * enqueued, reads whatever film the context holds, writes no film pass and neither uses nor disturbs an mpt_hint_image hint.
 * Fails for iterations outside 0..8 and for a sigma that is not finite and positive. */
typedef struct {
    int32_t iterations;      /* 5   */
    float sigma_color;       /* 1.0 */
    float sigma_albedo;      /* 0.1 */
    float sigma_normal;      /* 0.3 */
    int32_t demodulate;      /* 1   */
} mpt_denoise_params;
int mpt_get_denoised(mpt_ctx *ctx, const mpt_denoise_params *params /* NULL = the defaults above */, float *out /* [nx][ny][4] */);
/* HIP-event time (ms) of the filter's kernels (prologue to epilogue) of the mpt_get_denoised calls since the last call, and their count */
int mpt_denoise_kernel_time(mpt_ctx *ctx, double *ms, int *launches);
/* Variance guidance, an opt-in mode of the denoised read-backs (the spatial half of spatiotemporal variance-guided filtering,
 * Schied et al. 2017): the colour tolerance of every pixel follows that pixel's own standard error, which the film's mark
 * (mpt_film_mark, below) measures, instead of one global sigma_color -- converged detail the guides cannot see (shadow edges,
 * caustics, reflections) is kept, and noise is still filtered where there is noise.  With M the mark, F0 and m as above, all
 * arithmetic f32 without contraction, IEEE division, expf:
 *   nA = M.w;  n = F0.w;  nB = n - nA;  has(p) = valid(p) and nA > 0 and nB > 0
 *   d = (F0.rgb / n - M.rgb / nA) / m  per channel
 *   v_0(p) = fminf(fmaxf(((d.r d.r + d.g d.g) + d.b d.b) (nA / nB), 0), 3.0e38f) if has(p), else 0
 *            (mpt_get_noise's standard error of the mean, squared, in the filter's demodulated space; a valid pixel without two
 *             groups carries no evidence of noise)
 *   for i = 0 .. iterations-1, s = 2^i, every valid p:
 *       g(p) = (sum b[dx] b[dy] v_i(q)) / (sum b[dx] b[dy])  over the 3x3 taps q = p + (dx, dy) at stride 1 inside the film and
 *              valid, b = [1/4, 1/2, 1/4], dx outer, dy inner, both ascending
 *       kc(p) = 1 / (sigma_variance^2 g(p) + 1e-10f)         (sigma_variance^2 = sigma_variance sigma_variance, rounded once)
 *       w(q) as above with |e_i(p)-e_i(q)|^2 kc(p) for the colour term; the albedo and normal terms and the order of the sums unchanged
 *       e_{i+1}(p) = sum w e_i(q) / sum w
 *       v_{i+1}(p) = (sum (w w) v_i(q)) / ((sum w) (sum w))  (0 where p is not valid)
 *   and the epilogue as above.  sigma_color is validated and otherwise unused: the variance narrows by itself as it is filtered.
 * mpt_denoise_set_variance: context state like mpt_mlt_set_param's; 0 (the default) = off, the filter above bit for bit; a positive
 *   finite value = on (4 is a good start); anything else fails and changes nothing.  While on, mpt_get_denoised and mpt_get_display
 *   with the denoised source run the guided filter and fail without a mark -- checked before anything else, also for iterations = 0,
 *   which otherwise stays mpt_get_image(ctx, 0, out).  The two variance planes, 4 bytes per pixel each, are allocated at the first
 *   guided read-back and released with the film.  No film pass and not the mark is written.
 * mpt_denoise_eval: test door in the mpt_noise_eval idiom: the SAME launches on caller-supplied accumulators f0, f1, f2 and mark
 *   [nx*ny][4], any nx, ny >= 1 with nx*ny <= max_filmsize, in buffers of its own; touches no film pass, not the context's mark and
 *   not the context's variance setting.  sigma_variance == 0 is the fixed filter; mark must be NULL then and given otherwise.
 *   var_out [nx][ny] (NULL, or guided only) = v_final, 0 where not valid; v_0 for iterations = 0. */
int mpt_denoise_set_variance(mpt_ctx *ctx, float sigma_variance);
int mpt_denoise_get_variance(mpt_ctx *ctx, float *out);
int mpt_denoise_eval(mpt_ctx *ctx, const mpt_denoise_params *params, float sigma_variance, const float *f0, const float *f1,
                     const float *f2, const float *mark /* NULL iff sigma_variance == 0 */, int nx, int ny,
                     float *out /* [nx][ny][4] */, float *var_out /* [nx][ny] or NULL */);

/* The film as a screen, a PNG or a viewport wants it: metered, tone-mapped, transfer-encoded, dithered and quantised to 8-bit RGBA on
 * the device, a quarter of mpt_get_image's bytes (no reference counterpart: its scripts end in ti.imshow of linear radiance; the
 * operator it sketched and never wired in is ptina/wip/tonemapping.py:15-18).  With F the raw accumulators of the source (film index
 * x*ny + y), f32 arithmetic without contraction unless said otherwise:
 *   valid(p) = F.w != 0
 *   c = F.rgb / F.w                              (source = a film pass)
 *       or the denoised colour, exactly the floats mpt_get_denoised would return          (source = MPT_DISPLAY_DENOISED)
 *   c = fminf(fmaxf(c, 0), 3.0e38f) per channel  (fmaxf's NaN rule: NaN -> 0; -x -> 0; +inf -> 3e38)
 *   Y = (0.2126 r + 0.7152 g) + 0.0722 b
 *   metering over the valid pixels, N of them:
 *       Lavg = exp((1/N) sum log(1e-4 + Y))      (1e-4 + Y in f32; the logarithms, their sum, the mean, the exponential and the
 *                                                 division into `key` in f64, E rounded to f32 once: neither a rounded log nor
 *                                                 the order of the sum then reaches an f32 ulp)
 *       E = exposure if exposure > 0;  key / Lavg if exposure == 0 (auto);  1 if auto and N == 0
 *   v = fminf(E c, 1e18f) per channel            (every operator has saturated long before; keeps v v finite)
 *       MPT_TONE_LINEAR    t = v
 *       MPT_TONE_PTINA     t = v / (v + 0.155) * 1.019                                    (ptina/wip/tonemapping.py:15-18)
 *       MPT_TONE_REINHARD  t = v (1 + v / white^2) / (1 + v)
 *       MPT_TONE_ACES      t = v (2.51 v + 0.03) / (v (2.43 v + 0.59) + 0.14)
 *   t = fminf(fmaxf(t, 0), 1)
 *       MPT_TRANSFER_SRGB  s = t <= 0.0031308 ? 12.92 t : 1.055 t^(1/2.4) - 0.055
 *       MPT_TRANSFER_GAMMA s = t^(1/gamma)
 *   byte = clamp(floor(255 s + B), 0, 255);  B = 0.5 without dither, (M(x, y) + 0.5) / 64 with it, M the 8x8 Bayer index of
 *       (x & 7, y & 7): M = sum over i = 0..2 of (((x^y) >> i) & 1) << (2(2-i)+1) | ((y >> i) & 1) << (2(2-i))   (its 2x2 corner
 *       is [[0,2],[3,1]])
 *   alpha = 255;  a pixel that is not valid = the bytes (230, 102, 230, 0), mpt_get_image's marker at 8 bits, whatever the parameters.
 * op = PTINA, exposure = 0.3, transfer = GAMMA, gamma = 2.2 is the reference's functor as written.
 * Layouts: MPT_LAYOUT_FILM is [nx][ny][4] u8, x-major like mpt_get_image; MPT_LAYOUT_DISPLAY is [ny][nx][4] with rows top-down --
 * pixel (x, y) at ((ny-1-y) nx + x) 4 -- what a PNG or a GL blit reads (numpy: swapaxes(film layout, 0, 1)[::-1]).
 * The metering is a two-stage sum whose shape depends on nx*ny alone and uses no atomics: the exposure and every byte repeat bit
 * for bit; a manual exposure skips it.  Like mpt_get_denoised the call flushes what is enqueued, reads whatever film the context
 * holds, writes no film pass, neither uses nor disturbs an mpt_hint_image hint, and treats columns a slab or stripe split did not
 * render as not valid (in the bytes and in the metering).  Into an mpt_host_alloc array the conversion writes the bytes straight
 * over PCIe when option "zero_copy" is 1.  Fails, the film untouched, for an unknown op / transfer / layout, a pass out of range, a
 * null `out`, an exposure that is negative or not finite, and a key, white or gamma that is not finite and positive. */
#define MPT_DISPLAY_DENOISED (-1)
#define MPT_TONE_LINEAR   0
#define MPT_TONE_PTINA    1
#define MPT_TONE_REINHARD 2
#define MPT_TONE_ACES     3
#define MPT_TRANSFER_SRGB  0
#define MPT_TRANSFER_GAMMA 1
#define MPT_LAYOUT_FILM    0
#define MPT_LAYOUT_DISPLAY 1
typedef struct {
    int32_t source;     /* 0..max_filmpasses-1 = that film pass; MPT_DISPLAY_DENOISED = pass 0 through the filter; default 0 */
    int32_t op;         /* MPT_TONE_*;      default ACES */
    int32_t transfer;   /* MPT_TRANSFER_*;  default SRGB */
    int32_t layout;     /* MPT_LAYOUT_*;    default FILM */
    int32_t dither;     /* default 1 */
    float exposure;     /* 0 = auto (default) */
    float key;          /* 0.18 */
    float white;        /* 4.0  */
    float gamma;        /* 2.2  */
} mpt_display_params;
int mpt_get_display(mpt_ctx *ctx, const mpt_display_params *params /* NULL = the defaults above */,
                    const mpt_denoise_params *denoise /* used when source is denoised; NULL = its defaults */,
                    uint8_t *out /* [nx][ny][4] or [ny][nx][4] */, float *exposure_used /* may be NULL */);
/* HIP-event time (ms) of the kernels (the filter's for a denoised source, metering, conversion) of the mpt_get_display calls since the
 * last call, and their count */
int mpt_display_kernel_time(mpt_ctx *ctx, double *ms, int *launches);
/* Test door in the mpt_unit_eval / mpt_comm_selftest idiom: the SAME metering and conversion kernels on a caller-supplied accumulator
 * array raw[nx*ny][4], any nx, ny >= 1 with nx*ny <= max_filmsize; touches no film pass (params->source is ignored) */
int mpt_display_eval(mpt_ctx *ctx, const mpt_display_params *params, const float *raw, int nx, int ny,
                     uint8_t *out, float *exposure_used);

/* Is the image converged?  A noise estimate of film pass 0 on the device, from the film and a copy of it taken earlier, so that a
 * progressive render can stop at a noise threshold instead of a hand-picked sample count (no reference counterpart: its scripts and
 * its Blender loop count samples).  With F the raw accumulator of pass 0 (film index x*ny + y, rgb sums, w the sample weight) and M
 * the mark -- the device copy of F that mpt_film_mark took -- f32 arithmetic without contraction, IEEE division and square root:
 *   nA = M.w;  n = F.w;  nB = n - nA                 (the samples fall into two groups: those of the mark, those added since)
 *   valid(p) = nA > 0 and nB > 0
 *   a = clamp0(M.rgb / nA);  m = clamp0(F.rgb / n)   clamp0(x) = fminf(fmaxf(x, 0), 3.0e38f) per channel
 *                                                    (mpt_get_display's rule: NaN -> 0, -x -> 0, +inf -> 3e38)
 *   k = sqrtf(nA / nB)                               (exactly 1 for equal halves)
 *   d = |m - a| k   per channel                      (the standard error of m from the two groups' means a and b:
 *                                                     |a - b| sqrt(nA nB) / n, written through m and a)
 *   e(p) = clamp0((((d.r + d.g) + d.b) / 3) / (1e-4f + sqrtf(((m.r + m.g) + m.b) / 3)))
 *                                                    (the last clamp0 moves only a value that is not finite -- saturated channels
 *                                                     whose sums overflow -- so that e is finite whatever the film holds)
 * With equal halves this is the convergence criterion of Cycles' adaptive sampling as written, so `threshold` is the "noise
 * threshold" a Blender user knows (Cycles: 0.01 final, 0.1 viewport).  Results:
 *   map    e as [nx][ny] f32 in film order, 0 where the pixel is not valid                               (optional)
 *   stats  over the valid pixels: valid = their count, above = the count of e > threshold, max = the largest e (exact), sum = the
 *          sum of the f32 values e, taken in f64; threshold echoes the argument.  The sum is two-stage with a shape that depends
 *          on nx*ny alone and uses no atomics: every field repeats bit for bit.
 * mpt_film_mark: flushes what is enqueued, then M := F on the main stream behind it.  The mark is 16 bytes per pixel, allocated at
 *   the first mark and released with the film.  mpt_clear and mpt_set_size drop the mark; a scene, camera or light change does not.
 * mpt_get_noise: map may be NULL, stats may be NULL, not both.  remark != 0 also sets M := F, in the same pass over the film: a
 *   loop that doubles the sample count between checks pays one pass per check.
 * mpt_get_mark: test door; out [nx*ny][4] = the mark's raw accumulators.
 * Like mpt_get_denoised the calls flush what is enqueued, read whatever film the context holds, write no film pass and neither use
 * nor disturb an mpt_hint_image hint; columns a slab or stripe split did not render have w = 0 and are not valid.  mpt_get_noise
 * and mpt_get_mark fail without a mark, mpt_get_noise and mpt_noise_eval for a threshold that is negative or not finite,
 * mpt_get_noise with both outputs NULL; a failed call leaves film and mark untouched.
 * The estimate means what it says for the engines that add one sample of weight 1 per pixel and frame (mpt_render,
 * mpt_render_brute).  On the Metropolis engine's splats it is defined and computed, and is not a noise estimate. */
typedef struct {
    int64_t valid, above;
    double sum;
    float max;
    float threshold;
} mpt_noise_stats;
int mpt_film_mark(mpt_ctx *ctx);
int mpt_get_noise(mpt_ctx *ctx, float threshold, int remark, float *map /* [nx][ny] or NULL */, mpt_noise_stats *stats /* or NULL */);
int mpt_get_mark(mpt_ctx *ctx, float *out /* [nx*ny][4] */);
/* Test door in the mpt_display_eval idiom: the SAME kernels on caller-supplied accumulators film_raw and mark_raw [nx*ny][4], any
 * nx, ny >= 1 with nx*ny <= max_filmsize; touches no film pass and not the context's mark.  map [nx*ny] and new_mark [nx*ny][4] (the
 * mark the re-mark mode leaves: film_raw) may be NULL */
int mpt_noise_eval(mpt_ctx *ctx, float threshold, const float *film_raw, const float *mark_raw, int nx, int ny,
                   float *map, float *new_mark, mpt_noise_stats *stats);
/* HIP-event time (ms) of the kernels (estimate, fold) of the mpt_get_noise calls since the last call, and their count */
int mpt_noise_kernel_time(mpt_ctx *ctx, double *ms, int *launches);

/* Adaptive sampling: render only the pixels whose noise estimate is still above the threshold -- what a Blender user means by
 * "noise threshold": Cycles stops sampling a pixel once it passes (no reference counterpart).  A pass beside the render kernels:
 * a selection kernel, a compacted pixel list the context keeps (THE SELECTION), and a list render kernel that traces the
 * PathEngine's path (path_step) for the listed pixels.  With e and valid of mpt_get_noise above:
 *   above(p)  = valid(p) and e(p) > threshold                                (>, not >=)
 *   active(p) = valid(p) and (above(p) or (dilate == 1 and one of p's up to eight neighbours inside the film is above))
 * A pixel that is not valid is never active: no samples on one side of the mark, which covers every column a slab or stripe split
 * did not render -- a context only ever lists pixels of its own share.  dilate = 1 is Cycles' filter: a converged pixel beside a
 * noisy one keeps sampling.
 * The list holds the int32 film indices x*ny + y of the active pixels in an order that is a function of the film alone: by 16x16
 * tile of the whole film, tile (tx, ty) before (tx, ty + 1) before (tx + 1, 0), and within a tile x - 16 tx ascending, then y.  It is
 * made without atomics and repeats bit for bit.
 * mpt_adapt_select: flushes what is enqueued, then selects on the main stream from pass 0 and the mark; writes no film pass and
 *   leaves the mark alone.  stats (may be NULL) = exactly what mpt_get_noise(threshold) reports, field for field; count (may be
 *   NULL) = the length of the list.  Fails without a mark, for a threshold mpt_get_noise refuses, for dilate outside {0, 1}.
 * mpt_adapt_get_list: the selection's indices; out = NULL with cap = 0 asks for the count alone.  Fails when cap < count.
 * mpt_adapt_set_list: a selection from the host (a region, a user mask; the tests' door).  The indices must be strictly ascending --
 *   so no pixel is listed twice -- in [0, nx*ny) and in columns of the context's slab or stripes; otherwise the call fails, names
 *   the first offender and keeps the selection there was.  count = 0 is a selection of nothing.
 * mpt_render_selected: nframes samples for every pixel of the selection, launched at the call like mpt_render_brute and ordered
 *   with the other engines' frames the same way.  Per launch the Sobol sampler advances exactly as for mpt_render (also when the
 *   selection is empty) and work item f*count + k traces frame f of list entry k; a fold then adds each pixel's samples to pass 0
 *   in frame order, (r, g, b, 1) per sample -- the PathEngine's order of additions, so the film does not depend on how the frames
 *   were split into launches (a launch's samples stay under 64 MiB), and in the strict build the listed pixels hold exactly what
 *   mpt_render would have added to them.  remark != 0 (needs a mark) first sets M := F for the listed pixels -- the samples of this
 *   call are then their second group -- and does nothing when nframes = 0.  Pixels off the list keep film and mark.  Fails when
 *   there is no selection.
 * mpt_set_size and mpt_clear drop the selection (they change what an index means, or drop the mark); nothing else does.
 * mpt_adapt_eval: test door in the mpt_noise_eval idiom: the SAME selection kernels on caller-supplied accumulators film_raw and
 *   mark_raw [nx*ny][4] in buffers of its own; touches no film pass, not the context's mark and not its selection.  list_out
 *   [cap], count and stats may each be NULL, not all three.
 * mpt_adapt_kernel_time: HIP-event time (ms) of the selections (mpt_adapt_select) and of the list passes (mpt_render_selected, render
 *   kernels and folds of the whole call) since the last call, and how many such calls there were (a list pass that launched
 *   nothing is not counted); the test door is not timed. */
int mpt_adapt_select(mpt_ctx *ctx, float threshold, int dilate, mpt_noise_stats *stats /* or NULL */, int *count /* or NULL */);
int mpt_adapt_get_list(mpt_ctx *ctx, int32_t *out /* [cap] or NULL */, int cap, int *count /* or NULL */);
int mpt_adapt_set_list(mpt_ctx *ctx, const int32_t *pix /* [count] */, int count);
int mpt_render_selected(mpt_ctx *ctx, int nframes, int remark);
int mpt_adapt_eval(mpt_ctx *ctx, float threshold, int dilate, const float *film_raw, const float *mark_raw, int nx, int ny,
                   int32_t *list_out, int cap, int *count, mpt_noise_stats *stats);
int mpt_adapt_kernel_time(mpt_ctx *ctx, double *select_ms, double *render_ms, int *launches);

/* Scene composition on the device: what the reference's add-on does on the host at every scene change -- compose_multiple_meshes over
 * all meshes, then load_model (blender.py:555-571; ptina/multimesh.py:9-87) -- with the meshes and the object table resident on the
 * device.  A MESH is k faces in object space, [3k][8] f32 records pos3 nrm3 uv2 (mpt_load_model's layout); an OBJECT is a mesh, a
 * world matrix (16 doubles, row-major as numpy holds it) and a material id.  mpt_compose writes the model mpt_build_tree reads:
 * the objects in the order they were added, each object's faces contiguous, per vertex in f64 (multimesh.py:58-65)
 *   ph = (p, 1) . W^T, pos = ph.xyz / ph.w;   nh = (n, 0) . W^T, nrm = nh.xyz / |nh.xyz|;   uv copied
 * rounded to f32 once.  Normals go through W itself and a zero normal gives NaN, as in the reference.
 * mpt_mesh_add: copies the records to the device; k = 0 is a mesh (the reference accepts one).
 * mpt_object_add / mpt_object_set_world / mpt_object_set_material: refuse an unknown mesh or object id, a matrix entry that is not
 *   finite, a material id outside [-1, max_materials); they change the table only.
 * mpt_scene_clear: drops the objects, and with meshes != 0 the meshes too.  The composed model stays what it was until mpt_compose.
 * mpt_compose: after objects were added or dropped (or mpt_load_model took the model back) it writes every face; otherwise only the
 *   faces of the objects changed since the last call, and only those objects' table records (160 bytes each) cross to the device.  Fails with
 *   "too many faces" when the objects' faces reach max_faces.  Leaves the model as mpt_load_model of the same arrays would --
 *   face count, largest material id, bounding sphere -- and the tree invalid; the host's copy of the model is fetched only when
 *   something reads it (the host tree passes, mpt_get_model).  mpt_load_model afterwards replaces the composed model as ever.
 * mpt_compose_stats: faces of the model, faces the last mpt_compose wrote, objects it found changed, how often the host's copy of a
 *   composed model has been fetched since mpt_create, and the model's bounding sphere as the render launches use it (it reads
 *   whichever of mpt_load_model and mpt_compose came last).
 * mpt_get_model: the model as loaded or composed, verts [3n][8] and mtlids [n] (either may be NULL); fails when cap_faces < n.
 * mpt_compose_kernel_time: HIP-event time (ms) of the kernels of the mpt_compose calls since the last call, and their count.
 * mpt_compose_plan: the layout and the launch of a composition as a pure function (no context, no GPU): faces[nobj] per object and
 *   dirty[nobj] (NULL: all) give first[nobj + 1], the objects' first output faces and the total, and the runs of 256-vertex
 *   workgroups of the output that overlap a dirty object with faces, merged where they touch: the first `cap` of them as
 *   wg_begin / wg_count (any output may be NULL).  Returns the number of runs, -1 for arguments that name no layout (a negative
 *   count, 3 x total beyond 31 bits). */
typedef struct {
    int64_t faces, recomposed, dirty_objects, host_fetches;
    double scene_cen[3], scene_rad;
} mpt_compose_info;
int mpt_mesh_add(mpt_ctx *ctx, const float *verts /* [3k][8] */, int k, int *mesh_id);
int mpt_object_add(mpt_ctx *ctx, int mesh_id, const double world[16], int mtlid, int *obj_id);
int mpt_object_set_world(mpt_ctx *ctx, int obj_id, const double world[16]);
int mpt_object_set_material(mpt_ctx *ctx, int obj_id, int mtlid);
int mpt_scene_clear(mpt_ctx *ctx, int meshes);
int mpt_compose(mpt_ctx *ctx);
int mpt_compose_stats(mpt_ctx *ctx, mpt_compose_info *out);
int mpt_get_model(mpt_ctx *ctx, float *verts, int32_t *mtlids, int cap_faces, int *nfaces);
int mpt_compose_kernel_time(mpt_ctx *ctx, double *ms, int *launches);
int mpt_compose_plan(const int32_t *faces, const int32_t *dirty, int nobj, int64_t *first, int64_t *wg_begin, int64_t *wg_count, int cap);

/* Mesh deformation on the device: glTF 2.0's morph targets and linear-blend skinning for the meshes of the pool, so that a pose
 * change costs the upload of the pose, one kernel over that object's corners, the partial mpt_compose and mpt_refit_tree.  A MESH
 * may carry T morph targets (a position and a normal delta per corner) and a skin (four joint indices and four weights per corner,
 * over njoints joints); an OBJECT of such a mesh carries its own pose: T weights (default 0) and njoints joint matrices (default
 * identity; 4x4 affine, glTF's globalJoint . inverseBind, in the object's space).  Two objects of one mesh pose independently.
 * Per corner, in f64, sums left to right without contraction, rounded to f32 once:
 *   q = p + w_0 dp_0 + w_1 dp_1 + ...   (index order; a target whose weight is exactly 0 is skipped)      m = n + w_0 dn_0 + ...
 *   with a skin:  M = ((a0 J[j0] + a1 J[j1]) + a2 J[j2]) + a3 J[j3]  per entry of the upper 3x4 (weights as given, not renormalised),
 *                 q' = M . (q, 1),  m' = M . (m, 0)
 *   nrm = m' / |m'| (always);  uv copied.
 * The normal goes through M itself, not its inverse transpose -- the rule mpt_compose applies to the world matrix -- and a zero
 * normal gives NaN.  The result, the object's DEFORMED COPY, is an ordinary mesh record in the pool that mpt_compose reads instead
 * of the mesh.
 * mpt_mesh_set_morph / mpt_mesh_set_skin: once per mesh, before the mesh has an object.  Refuse, naming the argument: an unknown
 *   mesh; a mesh that already has an object (or already has targets / a skin); T outside [1, 64] or njoints outside [1, 256]; a
 *   joint index >= njoints; a delta or weight that is not finite; a negative weight.
 * mpt_object_set_morph_weights / mpt_object_set_joints (mats: [n][16] row-major): refuse an unknown object; n different from the
 *   mesh's count; an object whose mesh has no targets / no skin; a value that is not finite; a bottom row that is not exactly
 *   0 0 0 1.  They mark the object changed for mpt_compose.
 * mpt_compose, for every deformable object whose pose changed: uploads the pose, launches the deform kernel (one launch for all of
 *   them), then composes as ever.  After objects were added or dropped the copies get their room in the pool behind the meshes and
 *   every deformable object is deformed again; mpt_mesh_add while copies exist takes their room (the next mpt_compose assigns it
 *   again), mpt_scene_clear gives it back.  mpt_object_set_world on a deformable object recomposes it without deforming it again.
 * mpt_get_deformed: the object's deformed copy [3k][8] as the last mpt_compose wrote it; fails for an object that is not
 *   deformable, before the first mpt_compose, and when cap_faces < k.
 * mpt_deform_stats: deformable objects of the table; objects and corners the last mpt_compose deformed; pool vertices held by copies.
 * mpt_deform_kernel_time: HIP-event time (ms) of the deform kernels of the mpt_compose calls since the last call, and their count.
 * mpt_deform_plan: the run table of a deform launch as a pure function (no context, no GPU): corners[nobj] per object and dirty[nobj]
 *   (NULL: all) give, for every flagged object with corners, its index and its first block, blocks of 1024 corners, the first
 *   `cap` of them (any output may be NULL), and the blocks' sum.  Returns the number of runs, -1 for arguments that name no launch.
 * mpt_skin_check: the validation of a skin's arrays as a pure function.  Returns 0, or 1 bad arrays, 2 njoints outside [1, 256], 3 a joint
 *   index >= njoints, 4 a weight that is not finite, 5 a negative weight, with the words in why[why_size] (may be NULL). */
typedef struct {
    int64_t deformable_objects, deformed_objects, deformed_corners, copy_verts;
} mpt_deform_info;
int mpt_mesh_set_morph(mpt_ctx *ctx, int mesh_id, const float *deltas /* [T][3k][6] */, int T);
int mpt_mesh_set_skin(mpt_ctx *ctx, int mesh_id, const uint16_t *joints /* [3k][4] */, const float *weights /* [3k][4] */, int njoints);
int mpt_object_set_morph_weights(mpt_ctx *ctx, int obj_id, const double *w, int n);
int mpt_object_set_joints(mpt_ctx *ctx, int obj_id, const double *mats /* [n][16] */, int n);
int mpt_get_deformed(mpt_ctx *ctx, int obj_id, float *verts, int cap_faces);
int mpt_deform_stats(mpt_ctx *ctx, mpt_deform_info *out);
int mpt_deform_kernel_time(mpt_ctx *ctx, double *ms, int *launches);
int mpt_deform_plan(const int32_t *corners, const int32_t *dirty, int nobj, int32_t *run_obj, int64_t *run_block, int cap, int64_t *blocks);
int mpt_skin_check(const uint16_t *joints, const float *weights, int64_t ncorners, int njoints, char *why, int why_size);

/* Keyframe animation on the device: glTF 2.0's animations (samplers, channels, joint hierarchy) for the deformable meshes of the pool,
 * so that a frame of any number of animated objects costs mpt_scene_set_time -- one double -- and one kernel that writes their poses
 * where the deform kernel reads them.  Reading animations from files is not part of it.  The rule (csrc/anim_rule.h states it once,
 * for host and device; f64, every sum in one written order, no contraction):
 *   SKELETON of a mesh with a skin: parents[j] in [-1, j) (parents come before children), a rest pose per joint (rest [j][10]:
 *     translation3, rotation4 x y z w, scale3) and inverse_bind [j][12] (3x4 row-major).  Its joint count is the skin's.
 *   CLIP of a mesh: tracks, each (target, path, interpolation, nkeys): target a joint, or -1 for the morph weights; path 0 T, 1 R, 2 S,
 *     3 W; interpolation 0 STEP, 1 LINEAR, 2 CUBICSPLINE; f32 key times, finite and strictly increasing; f32 values, C = 3, 4, 3 or
 *     ntargets per key, three times that for CUBICSPLINE (in-tangent, value, out-tangent, as glTF lays them out).  At most one track per
 *     (target, path).  A key's rotation is used as given, not renormalised; a zero one is refused.  The clip's span [t0, t1]: the least
 *     first key to the greatest last key.  A mesh with targets and no skin has no skeleton and may have clips of W tracks.
 *   BINDING of an object: (clip, offset, speed, loop).  Local time at scene time t: tau = (t - offset) * speed; with loop and t1 > t0,
 *     tau = t0 + (x - floor(x / d) * d), x = tau - t0, d = t1 - t0; otherwise as it is: each track clamps for itself.
 *   A TRACK at tau: one key, or tau <= the first key: the first value; tau >= the last key: the last; else k the largest index with
 *     time[k] <= tau, dt = time[k+1] - time[k], u = (tau - time[k]) / dt, and STEP v_k; LINEAR v_k + u (v_k+1 - v_k), for R the slerp:
 *     d = dot(a, b); d < 0: b = -b, d = -d; d > 0.9995: normalise(a + u (b - a)); else theta = acos d,
 *     (sin((1 - u) theta) a + sin(u theta) b) / sin theta; CUBICSPLINE glTF's Hermite form with the tangents scaled by dt
 *     (coefficients: anim_rule.h), an R result normalised.
 *   A joint's T, R or S without a track is its rest value; local = [R(q) diag(s) | t]; global[j] = local[j] for a root, else
 *     global[parent] . local[j] (affine 3x4 product, each entry ((a0 b0 + a1 b1) + a2 b2) (+ a3)); palette[j] = global[j] . inverse_bind[j].
 *     Morph weights without a W track are 0.  The pose: ntargets weights, then njoints x 12 doubles.
 *   Only the slerp's theta branch calls library functions (acos, sin); everything else is + - * / sqrt floor and reproducible bit for bit.
 * mpt_mesh_set_skeleton: once per mesh, behind mpt_mesh_set_skin and before the mesh has an object.  mpt_mesh_add_clip: any number
 *   per mesh, before the mesh has an object; tracks [ntracks][4], times and values the tracks' arrays back to back; *clip_id counts over
 *   the scene.  They refuse, naming the argument: an unknown mesh or one that has an object; a mesh without a skin, or njoints not the
 *   skin's; parents out of order; a value that is not finite; a zero rotation; key times that are not finite or not increasing; a track
 *   on a joint beyond njoints; a W track on a mesh without targets; two tracks on one (target, path).
 * mpt_object_set_animation: binds a deformable object to a clip of its mesh (refuses a clip of another mesh; offset and speed finite);
 *   clip -1 unbinds: the pose is again what mpt_object_set_joints / mpt_object_set_morph_weights last gave, and while an object is
 *   bound those two refuse it (unbind first).  mpt_scene_set_time: the scene's time (0 at first; finite); marks every bound object
 *   changed for mpt_compose, as mpt_object_set_joints marks one; the same time again marks nothing.
 * mpt_compose: the changed bound objects' poses are not uploaded but evaluated, all in one launch in front of the deform kernel; after
 *   objects were added or dropped every bound object is evaluated again.  A scene without a binding is composed as ever.
 * mpt_get_pose: a deformable object's pose as it lies on the device after the last mpt_compose (ntargets + 12 njoints doubles; cap: the
 *   room of `pose` in doubles), bound or not.
 * mpt_anim_stats: skeletons, clips and tracks of the scene; bound objects; objects the last mpt_compose evaluated.
 * mpt_anim_kernel_time: HIP-event time (ms) of the animation kernels of the mpt_compose calls since the last call, and their count.
 * mpt_anim_rule: the whole evaluation of one object's pose as a pure function (no context, no GPU) from flat arrays, at scene time t;
 *   returns 0, or 100 + mpt_clip_check's verdict, or 200 + the skeleton's (1 bad arrays, 2 njoints outside [1, 256], 3 parents out of
 *   order, 4 a value not finite, 5 a zero rest rotation); njoints 0: no skeleton.
 * mpt_clip_check: the validation of a clip's arrays as a pure function.  Returns 0, or 1 bad arrays, 2 an unknown path or interpolation,
 *   3 a track on a joint beyond njoints (or a W track whose target is not -1), 4 a W track without targets, 5 nkeys < 1, 6 a key time not
 *   finite, 7 key times not increasing, 8 two tracks on one (target, path), 9 a zero key rotation, 10 a value not finite, with the
 *   words in why[why_size] (may be NULL).
 * mpt_anim_trig: the measurement door of the slerp's library functions: acos and sin of x [n] as the device evaluates them. */
typedef struct {
    int64_t skeletons, clips, tracks, bound_objects, evaluated_objects;
} mpt_anim_info;
int mpt_mesh_set_skeleton(mpt_ctx *ctx, int mesh_id, int njoints, const int32_t *parents, const double *rest /* [njoints][10] */,
                          const double *inverse_bind /* [njoints][12] */);
int mpt_mesh_add_clip(mpt_ctx *ctx, int mesh_id, int ntracks, const int32_t *tracks /* [ntracks][4] */, const float *times, int64_t ntimes,
                      const float *values, int64_t nvalues, int *clip_id);
int mpt_object_set_animation(mpt_ctx *ctx, int obj_id, int clip_id, double offset, double speed, int loop);
int mpt_scene_set_time(mpt_ctx *ctx, double t);
int mpt_get_pose(mpt_ctx *ctx, int obj_id, double *pose, int cap);
int mpt_anim_stats(mpt_ctx *ctx, mpt_anim_info *out);
int mpt_anim_kernel_time(mpt_ctx *ctx, double *ms, int *launches);
int mpt_anim_rule(int njoints, int ntargets, const int32_t *parents, const double *rest, const double *inverse_bind, int ntracks,
                  const int32_t *tracks, const float *times, int64_t ntimes, const float *values, int64_t nvalues, double offset, double speed,
                  int loop, double t, double *pose /* [ntargets + 12 njoints] */);
int mpt_clip_check(int njoints, int ntargets, int ntracks, const int32_t *tracks, const float *times, int64_t ntimes, const float *values,
                   int64_t nvalues, char *why, int why_size);
int mpt_anim_trig(mpt_ctx *ctx, const double *x, int n, double *acos_out, double *sin_out);

/* Two clips blended, and objects moved by clips (the rule stands once in csrc/anim_rule.h, f64 in one written
 * order without contraction, and adds no library call to the slerp's acos and sin).
 *   A SECOND BINDING of a bound deformable object: (clip_b, offset, speed, loop, w0, w1, fade_start, fade_duration); clip_b a clip of the
 *     object's mesh, offset, speed and fade_start finite, fade_duration finite and >= 0, w0 and w1 in [0, 1].  The weight at SCENE time t:
 *     with fade_duration > 0, x = (t - fade_start) / fade_duration, s = 0 below 0, 1 above 1, else x; with fade_duration == 0, s = 1 from
 *     fade_start on, else 0; s == 0: w = w0 itself, s == 1: w = w1 itself, else w = w0 + s (w1 - w0).  A constant weight is w0 = w1.
 *     Each clip has its own local time, from its own binding and span.  Every joint's T, R, S and the morph weights are evaluated for both
 *     clips (a from A, b from B; without a track the rest value, 0 for the weights).  w == 0: a, bit for bit; w == 1: b, bit for bit; else
 *     T, S, W: a + w (b - a) per component; R the normalised lerp over the shorter arc: d = ((a0 b0 + a1 b1) + a2 b2) + a3 b3; d < 0:
 *     b = -b; q = a + w (b - a); q / |q|.  Then local matrices, hierarchy and palette as for one clip.
 *   An OBJECT CLIP has no mesh: its tracks name target 0, the object's node, on the paths T, R and S (a W track is refused); clip ids
 *     count on in the scene's one list.  A MOTION BINDING of an object -- any object that is not an instance of a scatter -- holds (clip,
 *     offset, speed, loop, rest [10], base [16]): rest translation3 rotation4 xyzw scale3, finite with a rotation that is not zero (NULL:
 *     0 0 0, 0 0 0 1, 1 1 1); base a finite row-major 4x4, the node's static parents (NULL: the identity).  trs = rest, overwritten by the
 *     clip's tracks at the local time; L = local(trs), 3x4; world = base . [L; 0 0 0 1], every row r of the four by
 *     W[r][c] = (B[r][0] L[0][c] + B[r][1] L[1][c]) + B[r][2] L[2][c], c < 3, and W[r][3] = ((B[r][0] L[0][3] + B[r][1] L[1][3]) + B[r][2] L[2][3]) + B[r][3].
 * mpt_object_set_animation_blend: the second binding of an object that mpt_object_set_animation has bound; clip_b -1 removes it;
 *   mpt_object_set_animation with clip -1 removes both, and binding A again leaves B.  Refuses an unbound object, an object clip, a clip
 *   of another mesh, w0 or w1 outside [0, 1], a negative duration, a value that is not finite.  Blended objects are evaluated in the same
 *   one launch as the others.
 * mpt_scene_add_object_clip: at any time; the clips go with mpt_scene_clear(1), every binding with any mpt_scene_clear.
 * mpt_object_set_motion: binds; clip -1 unbinds, and the object returns to the matrix mpt_object_add / mpt_object_set_world last gave.
 *   While an object is bound mpt_object_set_world refuses it (unbind first).  Refuses an instance of a scatter, a mesh's clip (and
 *   mpt_object_set_animation refuses an object clip), a value that is not finite, a zero rest rotation.  mpt_scene_set_time marks the
 *   bound objects; mpt_compose evaluates the marked ones, those whose row goes up for another reason, and after a change of layout all,
 *   in one launch of a lane per object behind the table's upload and in front of the scatters and the composition.  The same time again
 *   marks nothing.
 * mpt_get_object_world: an object's matrix [16] as it lies on the device after the last mpt_compose, moved or not; refuses before it.
 * mpt_anim_blend_stats: object clips; objects with a second binding; objects with a motion binding; how many of each the last
 *   mpt_compose evaluated.  mpt_motion_kernel_time: as mpt_anim_kernel_time, of the motion kernel.
 * mpt_anim_blend_rule / mpt_motion_rule: the whole evaluation of one blended pose / one world matrix at scene time t as pure functions
 *   (no context, no GPU).  They return 0; 201 for bad arrays; 100 + mpt_clip_check's verdict of clip A (of the object clip, checked as a
 *   clip of one joint and no targets); 300 + that of clip B; 200 + the skeleton's; 400 + the second binding's (1 a value not finite,
 *   2 a negative duration, 3 a weight outside [0, 1]); 500 + the motion binding's (1 rest not finite, 2 a zero rest rotation, 3 base not
 *   finite, 4 offset or speed not finite). */
typedef struct {
    int64_t object_clips, blended_objects, moved_objects, evaluated_blended, evaluated_moved;
} mpt_anim_blend_info;
int mpt_object_set_animation_blend(mpt_ctx *ctx, int obj_id, int clip_b, double offset, double speed, int loop, double w0, double w1,
                                   double fade_start, double fade_duration);
int mpt_scene_add_object_clip(mpt_ctx *ctx, int ntracks, const int32_t *tracks /* [ntracks][4] */, const float *times, int64_t ntimes,
                              const float *values, int64_t nvalues, int *clip_id);
int mpt_object_set_motion(mpt_ctx *ctx, int obj_id, int clip_id, double offset, double speed, int loop, const double *rest /* [10] or NULL */,
                          const double *base /* [16] or NULL */);
int mpt_get_object_world(mpt_ctx *ctx, int obj_id, double *world /* [16] */);
int mpt_anim_blend_stats(mpt_ctx *ctx, mpt_anim_blend_info *out);
int mpt_motion_kernel_time(mpt_ctx *ctx, double *ms, int *launches);
int mpt_anim_blend_rule(int njoints, int ntargets, const int32_t *parents, const double *rest, const double *inverse_bind, int ntracks_a,
                        const int32_t *tracks_a, const float *times_a, int64_t ntimes_a, const float *values_a, int64_t nvalues_a, double offset_a,
                        double speed_a, int loop_a, int ntracks_b, const int32_t *tracks_b, const float *times_b, int64_t ntimes_b,
                        const float *values_b, int64_t nvalues_b, double offset_b, double speed_b, int loop_b, double w0, double w1,
                        double fade_start, double fade_duration, double t, double *pose /* [ntargets + 12 njoints] */);
int mpt_motion_rule(int ntracks, const int32_t *tracks, const float *times, int64_t ntimes, const float *values, int64_t nvalues, double offset,
                    double speed, int loop, const double *rest, const double *base, double t, double *world /* [16] */);

/* Objects parented to objects and to joints (the rule stands once at the end of csrc/anim_rule.h, f64 in one
 * written order without contraction, no new library call).
 *   A PARENT BINDING of an object is (parent, joint): another object of the table, and -1 or a joint of the skin of the parent's mesh.
 *   Once bound, the object's own matrix is its LOCAL matrix: what mpt_object_add / mpt_object_set_world gave (mpt_object_set_world stays
 *   allowed and sets it), or with a motion binding base . T R S exactly as above.  Then
 *     joint -1:  world(child) = world(parent) . local
 *     joint j:   world(child) = world(parent) . ([M_j; 0 0 0 1] . local), the inner product first,
 *   M_j the 3x4 entry j of the parent's pose as it lies in the device's pose buffer this compose (what mpt_get_pose returns: the skinning
 *   matrix global . inverse bind, set by mpt_object_set_joints, by one clip or by two blended), so that the child moves as a vertex
 *   skinned to j with weight 1.  Every product is W[r][c] = ((A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c]) + A[r][3] B[3][c];
 *   neither factor need be affine.
 * mpt_object_set_parent: binds; parent -1 unparents, and the object's matrix is read as its world again.  It refuses, by the number
 *   mpt_parent_check returns, and changes nothing: 1 an unknown object or parent; 2 an object as its own ancestor; 3 a child or a parent
 *   that is an instance of a scatter; 4 joint >= 0 when the parent's mesh has no skin; 5 a joint outside the parent's joints; 6 a chain
 *   deeper than 64 (a child of a root has depth 1).  A child may be a scatter's surface, deformable, subdivided, or of a mesh without
 *   faces.  The bindings go with any mpt_scene_clear.
 * mpt_compose first marks, level by level, every child whose parent's row is dirty for any reason, or that names a joint of a parent
 *   whose pose is dirty; then, behind the moved objects and in front of the scatters and the composition, hierarchy.hip's kernel, a lane
 *   per child, evaluates the marked children, after a change of layout all, and any whose own row went up: in one launch while they are
 *   at most 1024, else in one launch per level evaluated.  A bound child with a motion binding is evaluated there and not by the motion
 *   kernel.  The same time again marks nothing and launches nothing.
 * mpt_object_get_parent: the binding (-1, -1: none).  mpt_hierarchy_stats: bound children and the deepest chain; children evaluated,
 *   levels and launches of the last mpt_compose.  mpt_hierarchy_kernel_time: as mpt_anim_kernel_time, of the hierarchy kernel.
 * mpt_parent_check: the refusals above as a pure function of the bindings as they stand (parents [nobj]), instance [nobj] (not 0: an
 *   instance of a scatter) and njoints [nobj] (of each object's mesh's skin).
 * mpt_hierarchy_rule: one object's world matrix at scene time t as a pure function (no context, no GPU) of its chain of n links, link 0
 *   the root and link n - 1 the object: locals [n][16] (a link's local matrix, or its motion binding's base); ntracks [n] (-1: no motion
 *   binding; else the tracks of the link's object clip, which stand back to back in tracks, times and values; ntimes [n] and nvalues [n]
 *   say how many of each are the link's); bindings [n][3] (offset, speed, loop != 0) and rests [n][10] of the motion bindings (NULL with
 *   no motion binding in the chain); joints [n] (joints[k] >= 0: link k follows a palette entry) and palette [n][12] (the entries; NULL
 *   when no joint is named).  It returns 0; 601 for bad arrays; 602 for n outside [1, 65]; 603 for a local matrix and 604 for a named
 *   palette entry that is not finite; 100 + mpt_clip_check's verdict of a link's object clip; 500 + the motion binding's, as
 *   mpt_motion_rule. */
typedef struct {
    int64_t bound_children, deepest, evaluated, levels, launches;
} mpt_hierarchy_info;
int mpt_object_set_parent(mpt_ctx *ctx, int obj_id, int parent_id, int joint);
int mpt_object_get_parent(mpt_ctx *ctx, int obj_id, int *parent_id, int *joint);
int mpt_hierarchy_stats(mpt_ctx *ctx, mpt_hierarchy_info *out);
int mpt_hierarchy_kernel_time(mpt_ctx *ctx, double *ms, int *launches);
int mpt_parent_check(int nobj, const int32_t *parents, const int32_t *instance, const int32_t *njoints, int obj, int parent, int joint, char *why,
                     int why_size);
int mpt_hierarchy_rule(int n, const double *locals, const int32_t *ntracks, const int32_t *tracks, const float *times, const int64_t *ntimes,
                       const float *values, const int64_t *nvalues, const double *bindings, const double *rests, const int32_t *joints,
                       const double *palette, double t, double *world /* [16] */);

/* Loop subdivision on the device (triangles in, four triangles out per level) as a property of a mesh of the pool, evaluated inside
 * mpt_compose behind morph targets and skinning and before composition, so that a pose change of a subdivided character costs the
 * upload of the pose, the deform kernel, L + 2 kernels over that object, the partial mpt_compose and mpt_refit_tree: topology and face
 * count stay constant.  The result, the SUBDIVIDED COPY, is an ordinary mesh record [3 k 4^L][8] in the pool that mpt_compose reads
 * instead of the mesh.  A mesh that is not deformable has one copy, computed once and shared by its objects; a deformable mesh has
 * one per object, computed again when that object's pose changes.  Face g of an object of such a mesh descends from face g >> 2L of
 * the mesh (what mpt_pick and mpt_intersect report is the refined face).
 * The definition.  All arithmetic is f64, every sum in the order written, without contraction; a value is rounded to f32 once, when
 * a record is written.
 *   Control vertices: corners whose f32 positions are equal as values (-0 equals +0) are one vertex; ids are ranks of first
 *     appearance in corner order; a vertex's position is its FIRST corner's, read from the mesh or -- a mesh with targets or a skin
 *     -- from the object's deformed copy.  A pose that pulls welded corners apart leaves the first corner speaking for the vertex (no
 *     cracks).  The mesh's own normals are not used.
 *   Level l -> l + 1: even vertices keep their ids 0 .. V_l - 1; the vertex of edge e is V_l + e, edges numbered in lexicographic
 *     order of (lower endpoint id, higher endpoint id); face f = (v0, v1, v2) becomes faces 4f .. 4f + 3: (v0, e01, e20),
 *     (v1, e12, e01), (v2, e20, e12), (e01, e12, e20).  Windings are kept.
 *   Ring of a vertex: its neighbours in the order of the faces' winding (in face (v, a, b), a comes before b); an interior vertex's
 *     ring starts at the neighbour with the lowest id, a boundary vertex's at the boundary neighbour that begins the fan.
 *   Rules (a the lower endpoint id, b the higher; c opposite in the face that runs a -> b, d opposite in the other):
 *     interior edge    (0.375 * (a + b)) + (0.125 * (c + d))            boundary edge    0.5 * (a + b)
 *     interior vertex  (w * v) + (beta * s):  s = ((r_0 + r_1) + r_2) + ... the ring left to right, n its length,
 *                      beta = 0.1875 for n = 3, else 3.0 / (8.0 * n), w = 1.0 - n * beta   (Warren's weights: rational, no cosine)
 *     boundary vertex  (0.75 * v) + (0.125 * (p + q)), p and q the first and the last of its ring.  There is no corner rule: a corner
 *                      of an open mesh shrinks.
 *   Normals, per vertex of the last level, on the unrounded positions: N = 0, then for its faces (v, r_i, r_i+1) in ring order (an
 *     interior ring closes) N += cross(r_i - v, r_i+1 - v), each component x1 y2 - x2 y1 as written;
 *     nrm = N / sqrt((Nx Nx + Ny Ny) + Nz Nz); a zero N gives NaN.  Every corner on a vertex gets that vertex's normal.
 *   Texcoords are face-varying (seams survive): a child face takes its corners' uv from its parent's three corner uvs by the face
 *     rule above, midpoints 0.5 * (u_i + u_j), level by level.
 * mpt_mesh_set_subdivision: once per mesh, before the mesh has an object; before or after mpt_mesh_set_morph / mpt_mesh_set_skin.
 *   Builds the topology on the host.  Refuses, naming the face or the vertex: an unknown mesh; a mesh that already has an object or a
 *   level; levels outside [1, 5]; k 4^L that reaches max_faces ("too many faces"); a position that is not finite; a face with two
 *   corners on one vertex; an edge with more than two faces; an edge that both its faces run in the same direction; a vertex whose
 *   faces are not one fan (a bow-tie).
 * mpt_object_add / mpt_compose count k 4^L faces for an object of such a mesh.  mpt_compose, behind the deform kernel: after objects
 *   were added or dropped the copies get their room in the pool behind the meshes and the deformed copies and every copy is made
 *   again; else the copies of the objects whose pose changed.  One refine launch per level, one for the normals, one for the
 *   records, whatever the number of copies.  mpt_object_set_world / mpt_object_set_material alone subdivide nothing.  mpt_mesh_add
 *   while copies exist takes their room (the next mpt_compose assigns it again), mpt_scene_clear gives it back.
 * mpt_get_subdivided: the object's subdivided copy [3 k 4^L][8] as the last mpt_compose wrote it; fails for an object whose mesh has
 *   no level, before the first mpt_compose, and when cap_faces < k 4^L.
 * mpt_subdiv_stats: objects of subdivided meshes; copies; copies and faces the last mpt_compose refined; pool vertices the copies hold.
 * mpt_subdiv_kernel_time: HIP-event times (ms) of the refine launches, the normals and the records of the mpt_compose calls since
 *   the last call (any may be NULL), and the number of kernels launched.
 * mpt_subdiv_topology: the topology as a pure function (no context, no GPU) of verts [3k][8] and levels: counts [levels + 1][3]
 *   (vertices, edges, faces per level), and ONE block of 32-bit words, the layout the device reads -- offsets[0..5]: [0] the first
 *   corner of every control vertex, [l] the rules of the vertices of level l, two words each, { kind | n << 2, ring }: kind 0 an
 *   interior vertex with its n neighbours at word `ring`, 1 a boundary vertex with its n neighbours (first to last), 2 an interior
 *   edge (a b c d), 3 a boundary edge (a b), ids of level l - 1; offsets[6]: the rules of the last level's rings (kinds 0 and 1);
 *   offsets[7]: the last level's faces [F][3]; offsets[8] = *need_words: the words of the block, which is written when cap_words holds
 *   it.  Returns 0, or 1 bad arguments, 2 levels outside [1, 5], 3 more than 2^24 faces, 4 a position that is not finite, 5 a face
 *   with two corners on one vertex, 6 an edge with more than two faces, 7 an edge run twice in one direction, 8 a bow-tie, with the
 *   words in why[why_size] (may be NULL).
 * mpt_subdiv_plan: the run table of one of the launches as a pure function: items[njobs] per job (0: the job sits the launch out)
 *   and dirty[njobs] (NULL: all) give, for every flagged job with items, its index and its first block, blocks of 256 items, the
 *   first `cap` of them (any output may be NULL), and the blocks' sum.  Returns the number of runs, -1 for arguments that name no launch. */
typedef struct {
    int64_t subdivided_objects, copies, refined_copies, refined_faces, copy_verts;
} mpt_subdiv_info;
int mpt_mesh_set_subdivision(mpt_ctx *ctx, int mesh_id, int levels);
int mpt_get_subdivided(mpt_ctx *ctx, int obj_id, float *verts, int cap_faces);
int mpt_subdiv_stats(mpt_ctx *ctx, mpt_subdiv_info *out);
int mpt_subdiv_kernel_time(mpt_ctx *ctx, double *refine_ms, double *normals_ms, double *records_ms, int *launches);
int mpt_subdiv_topology(const float *verts /* [3k][8] */, int k, int levels, int64_t *counts, int32_t *offsets /* [9] */, int32_t *words,
                        int64_t cap_words, int64_t *need_words, char *why, int why_size);
int mpt_subdiv_plan(const int32_t *items, const int32_t *dirty, int njobs, int32_t *run_job, int64_t *run_block, int cap, int64_t *blocks);

/* Semi-sharp creases, corners and hard edges of Loop subdivision (Blender's edge crease; the sharpness of OpenSubdiv).
 * mpt_mesh_set_subdivision_creased is mpt_mesh_set_subdivision with crease [k][3] f32, one sharpness per face edge -- edge j of face
 * f runs from corner j to corner (j + 1) % 3; in subdivision levels, 0 smooth, inf always sharp; the two faces on an edge may state
 * different values, the edge takes the larger -- and corner [k][3] bytes, one flag per face corner: a control vertex is a corner if any
 * of its welded corners is flagged.  Either may be NULL: all zero, none flagged.  They are fixed with the level.  A mesh whose
 * sharpnesses are all zero and that has no corner flagged is the mesh of mpt_mesh_set_subdivision, word for word and bit for bit.
 * Refuses what mpt_mesh_set_subdivision refuses, and a negative sharpness or a NaN, naming the face and the edge.
 * The definition.  Weld, ids, edge numbering, face split, uv rule and arithmetic are those of above.
 *   Sharpness per level: an edge of cage sharpness s0 (widened to f64) has at level l s_l = s0 - l if that is positive, else 0; inf
 *     stays inf.  Both halves of a split edge inherit s_{l+1}; the three edges new inside a face have 0; a boundary edge counts as inf
 *     everywhere.  Corner flags pass to even vertices only.
 *   Edge point of an interior edge of sharpness s at the level below, E the interior rule of above, H = 0.5 * (a + b):
 *     s == 0: E;  s >= 1: H;  else ((1 - s) * E) + (s * H), componentwise.  A boundary edge keeps its rule.
 *   Vertex point: S the sharpnesses > 0 of its incident edges in ring order from the ring's start, k their number, M the interior
 *     rule of above.  A flagged corner: v.  k <= 1 (a dart's end): M.  k == 2, p and q the far ends of the two sharp edges,
 *     C = (0.75 * v) + (0.125 * (p + q)), f = 0.5 * (s1 + s2): C if f >= 1, else ((1 - f) * M) + (f * C).  k >= 3,
 *     f = ((s1 + s2) + s3 + ...) / k: v if f >= 1, else ((1 - f) * M) + (f * v).  Where f >= 1 the blend is not evaluated.  A boundary
 *     vertex has k >= 2 with an inf in S: with its two boundary edges alone it is the boundary rule of above; a crease that reaches
 *     the boundary makes it a corner.
 *   Normals at the last level L: an edge is HARD if its sharpness at level L is > 0 (s0 > L, inf, or a boundary edge).  The hard
 *     edges cut a vertex's fan into sectors; a corner of face (v, r_i, r_i+1) takes the normal sum of above over the faces of its own
 *     sector, in ring order from the sector's first hard edge.  A vertex without a hard interior edge keeps its single normal, in the
 *     order of above; an interior vertex with one hard edge has one sector of all its faces, starting behind that edge.
 *   A displacement keeps taking its direction from the whole ring (a creased surface does not crack); the sector normals are then
 *     taken on the displaced positions.
 * mpt_subdiv_topology_creased: mpt_subdiv_topology with crease and corner (either may be NULL) and offsets [11].  A head is
 *   kind | n << 2 | variant << 28; variant 0 is the plain rule, and a creased mesh also has: kind 0 variant 1, the n neighbours, then p
 *   q, then the f64 f (low word first): ((1 - f) * M) + (f * C); kind 0 variant 2, the n neighbours, then the f64 f:
 *   ((1 - f) * M) + (f * v); kind 0 variant 3, n = 0: the vertex stays; kind 2 variant 1, a b c d, then the f64 s:
 *   ((1 - s) * E) + (s * H).  A vertex with f >= 1 on two sharp edges is a plain kind 1 of n = 2, p q; an interior edge with s >= 1 a
 *   plain kind 3.  offsets[6] stays the rules of the last level's whole rings.  offsets[9]: the rules of the last level's RECORDS,
 *   offsets[10] = R of them, then R vertex ids, then the sectors' rings; offsets[7]: the faces [F][3] as RECORD ids.  Record v < V_L
 *   is vertex v's first sector, or its whole ring where no interior edge of it is hard (its rule is then that at offsets[6]); the
 *   further sectors follow V_L in the order of the vertices, then of the ring.  A sector's rule is kind 1 with the neighbours from
 *   its first hard edge to its last.  An uncreased mesh has offsets[9] = 0, offsets[10] = V_L and the block of mpt_subdiv_topology.
 *   Returns what mpt_subdiv_topology returns, or 9: a sharpness that is negative or not a number. */
int mpt_mesh_set_subdivision_creased(mpt_ctx *ctx, int mesh_id, int levels, const float *crease /* [k][3] or NULL */, const uint8_t *corner /* [k][3] or NULL */);
int mpt_subdiv_topology_creased(const float *verts /* [3k][8] */, int k, int levels, const float *crease, const uint8_t *corner, int64_t *counts,
                                int32_t *offsets /* [11] */, int32_t *words, int64_t cap_words, int64_t *need_words, char *why, int why_size);

/* Catmull-Clark subdivision of a cage of quads and polygons (Blender's Subdivision Surface modifier), the second scheme a mesh of the
 * pool may carry: what is said of the subdivided copy, of mpt_compose and of the read-backs above holds for it, a displacement and a
 * scatter stand behind it as behind a Loop mesh, and the creases and corners are those of above.
 * mpt_mesh_set_subdivision_cc: polys [m] holds the corner count n_j of each polygon, 3 <= n_j <= 64, sum (n_j - 2) = k.  Polygon j
 *   is stored as n_j - 2 consecutive triangles of the mesh, a fan about its first corner: triangle i is (c_0, c_i+1, c_i+2).  NULL:
 *   every triangle is a polygon (m is ignored).  crease and corner are flat [sum n_j]: entry i of polygon j is the edge from corner i
 *   to corner (i + 1) % n_j, respectively corner i; either may be NULL.  An object of the mesh has F = 2 (sum n_j) 4^(L - 1) faces
 *   (an all-quad cage: k 4^L).  Refuses what mpt_mesh_set_subdivision_creased refuses (a crease is named by polygon and edge), and:
 *   polys that do not hold k triangles; an n outside [3, 64]; a triangle that does not continue its polygon's fan, named by face and
 *   polygon; a polygon with two corners on one vertex.  The mesh stays as it was.
 * The definition.  Arithmetic, weld, first-corner rule, ids of control vertices and edge numbering are those of above.
 *   Level l -> l + 1, ids: even vertices keep their ids; the edge point of edge e is V_l + e; the face point of face j is
 *     V_l + E_l + j.
 *   Face split: polygon or quad j of corners c_0 .. c_n-1 becomes n quads, quad i (c_i, e(c_i, c_i+1), f_j, e(c_i-1, c_i)); windings
 *     are kept.  At level 1 the quads of polygon j start at the sum of n_j' over j' < j; from level 1 on quad q becomes 4q .. 4q + 3.
 *   Emitted triangles: quad q = (v0, v1, v2, v3) of the last level is faces 2q (v0, v1, v2) and 2q + 1 (v0, v2, v3): face g of an
 *     object descends from level-1 quad (g >> 1) >> 2 (L - 1).
 *   Face point: F = (((c_0 + c_1) + c_2) + ...) / n.
 *   Edges (a the lower endpoint id, b the higher, F1 the point of the face that runs a -> b, F2 of the other):
 *     interior edge    E = 0.25 * ((a + b) + (F1 + F2))                  boundary edge    0.5 * (a + b)
 *   Ring of a vertex: its edge neighbours in winding order (in face (v, a, ..., b), a comes before b), the start as above.
 *   Interior vertex of valence n:  M = (((n - 2.0) / n) * v) + ((1.0 / (n * n)) * (S_r + S_f)),  S_r = ((r_0 + r_1) + r_2) + ... the
 *     ring left to right, S_f = ((F_0 + F_1) + F_2) + ... the face points in the same order, F_i the face between r_i and r_i+1.
 *   Boundary vertex: (0.75 * v) + (0.125 * (p + q)), p and q the first and the last of its ring; no corner rule unless it is flagged.
 *   A face point in an edge's or a vertex's rule is the value the face rule gives, bit for bit (a lane evaluates it again).
 *   Creases and corners: the text of above with E and M as here.  The halves of a split edge inherit, the edges new inside a face
 *     (edge point to face point) have sharpness 0, boundary edges count as inf; H, C, the blends by s and f and the cases k <= 1, 2 and
 *     >= 3 are those of above; a flagged vertex stays; where f >= 1 or s >= 1 no blend is evaluated.
 *   Normals at the last level: the sum of above over the ring of EDGE neighbours, N += cross(r_i - v, r_i+1 - v), one term per quad
 *     on the vertex, cut into sectors by the hard edges as above.  A displacement takes its direction from the whole ring.
 *   Texcoords are face-varying: a face point's uv is ((u_0 + u_1) + ...) / n, an edge's 0.5 * (u_i + u_j); a child quad takes its uvs
 *     by the split rule, level by level from the polygon's corner uvs.  Corner c_0's and c_1's uv are read from triangle 0 of the fan,
 *     corner c_i+2's from corner 2 of triangle i.
 * mpt_subdiv_topology_cc: the topology as a pure function, with offsets [12].  counts holds vertices, edges and faces per level
 *   (polygons at level 0, quads from level 1).  The block is mpt_subdiv_topology_creased's with these differences.  offsets[l]: the
 *   V + E + F rules of level l - 1's vertices, edges and then FACES.  A boundary vertex (kind 1), a boundary edge or one with s >= 1
 *   (kind 3, variant 0), a vertex that stays (kind 0 variant 3) and every rule of the last level's rings and records are as above;
 *   Catmull-Clark's own rules have bit 2 of the variant (4) set beside the blend: kind 3 variant 4, a face point, its n corners in
 *   the face's order; kind 2 variant 4 (4 | 1: then the f64 s), n = 4: a b, then the ids at level l of the face points F1 and F2 --
 *   a face point's rule is rule `id` of the same level; kind 0 variant 4, the n neighbours, then n face point ids (4 | 1: then p q
 *   and the f64 f; 4 | 2: then the f64 f).  offsets[11]: [Q_1][2], per quad of level 1 the first triangle of its polygon in the
 *   mesh and n | i << 8.  offsets[7]: [2 Q_L][3] record ids, the emitted triangles.  Returns what mpt_subdiv_topology_creased
 *   returns, or 10: polys that are not the mesh's triangles, an n outside [3, 64] or a triangle that does not continue its fan. */
int mpt_mesh_set_subdivision_cc(mpt_ctx *ctx, int mesh_id, int levels, const int32_t *polys /* [m] or NULL */, int m, const float *crease /* [sum n_j] or NULL */,
                                const uint8_t *corner /* [sum n_j] or NULL */);
int mpt_subdiv_topology_cc(const float *verts /* [3k][8] */, int k, int levels, const int32_t *polys, int m, const float *crease, const uint8_t *corner,
                           int64_t *counts, int32_t *offsets /* [12] */, int32_t *words, int64_t cap_words, int64_t *need_words, char *why, int why_size);

/* Texture displacement on the device as a property of a SUBDIVIDED mesh of the pool: the third step of the modifier stack armature ->
 * subdivision surface -> displace.  mpt_compose evaluates it on the vertices of the mesh's last level, behind the last refine launch
 * and before the normals, so the subdivided copy's normals are the displaced surface's.  Topology and face count stay constant: a
 * change of strength costs one vertex kernel, the normals, the records, the partial mpt_compose and mpt_refit_tree.
 * The definition.  All arithmetic is f64, every sum and product in the order written, without contraction; a value is rounded to
 * f32 once, when a record is written.
 *   Vertex uv: the FIRST CORNER of a last-level vertex i is the lowest index 3 g + c into the last level's face table with
 *     F[g][c] == i.  The vertex's uv is that corner's face-varying uv by the texcoord rule above: from the control records (the mesh
 *     or the object's deformed copy), down the base-4 digits of g, midpoints 0.5 * (u_i + u_j), unrounded.  The first corner to
 *     touch a vertex speaks for it (Blender's Displace modifier with UV coordinates; the weld rule above): a uv seam cannot crack
 *     the surface.
 *   Height: the image [nx][ny] holds f32 rgba texels at base + x * ny + y, x and y wrapped by Python's modulo (the reference's
 *     Image.subscript and Image.__call__, ptina/image.py:137-148).  px = u * (nx - 1), py = v * (ny - 1); fx = floor(px),
 *     fy = floor(py), the integer parts 64-bit; x0 = px - fx, x1 = py - fy, y0 = 1 - x0, y1 = 1 - x1; per channel
 *     t = (((t11 * x0) * x1 + (t10 * x0) * y1) + (t00 * y0) * y1) + (t01 * y0) * x1 with the texels widened to f64, t11 the texel
 *     at (fx + 1, fy + 1), t10 at (fx + 1, fy), t00 at (fx, fy), t01 at (fx, fy + 1).  Channel 0 to 3 picks r, g, b or a; channel
 *     4 is ((r + g) + b) / 3.0.
 *   MPT_DISPLACE_NORMAL: p' = p + (strength * (h - midlevel)) * n, n = N / sqrt((Nx Nx + Ny Ny) + Nz Nz) the unrounded smooth
 *     normal of the UNDISPLACED last level by the normal rule above.  A zero N gives a NaN position, as it gives a NaN normal.
 *   MPT_DISPLACE_VECTOR: p' = p + strength * ((r, g, b) - midlevel), component by component in object space; channel is ignored.
 *   The copy's normals are the normal rule evaluated on p'.  Texcoords are untouched.
 * mpt_mesh_set_displacement: once per mesh, after mpt_mesh_set_subdivision and before the mesh has an object; before or after its
 *   targets and skin.  The image need not be loaded yet.  Refuses: an unknown mesh; a mesh without a subdivision level
 *   ("displacement needs a subdivided mesh"); a mesh that already has an object or a displacement; a mode or a channel outside the
 *   enums; image_id < 0; a strength or midlevel that is not finite; a corner uv of the mesh that is not finite or exceeds 2^20 in
 *   magnitude, naming the corner (midpoints of admitted uvs are admitted, and px stays far inside 64-bit integers).
 * mpt_mesh_set_displacement_params: any time.  Every copy of the mesh is displaced again by the next mpt_compose and every object of
 *   the mesh composed again (the objects of a rigid mesh share one copy).
 * mpt_compose displaces a displaced copy again with the copies it subdivides again (a relayout, a pose change), after
 *   mpt_mesh_set_displacement_params, and when mpt_load_image or mpt_reset_images ran since it was last displaced (they bump an
 *   image generation).  Before anything else it checks that the image of every copy it will displace is loaded: if not it fails,
 *   naming mesh and image, and leaves the scene as it was; it succeeds once the image is there.  One displacement launch whatever
 *   the number of copies: L_max + 3 kernels with a displaced copy among those written, L_max + 2 without.
 * mpt_displace_stats: displaced meshes; copies of displaced meshes; copies and vertices the last mpt_compose displaced; the image
 *   generation.
 * mpt_displace_kernel_time: HIP-event time (ms) of the displacement launches of the mpt_compose calls since the last call (may be
 *   NULL) and their number.  mpt_subdiv_kernel_time counts its own three kinds of launch only.
 * mpt_displace_corners: the first-corner table as a pure function (no context, no GPU) of faces [nfaces][3] over nverts vertices:
 *   corner[nverts].  Returns 0, or 1 for arguments that name no table, 2 for an id outside [0, nverts), 3 for a vertex no face
 *   touches. */
enum { MPT_DISPLACE_NORMAL = 0, MPT_DISPLACE_VECTOR = 1 };
enum { MPT_DISPLACE_R = 0, MPT_DISPLACE_G = 1, MPT_DISPLACE_B = 2, MPT_DISPLACE_A = 3, MPT_DISPLACE_MEAN = 4 };
typedef struct {
    int64_t displaced_meshes, copies, displaced_copies, displaced_verts, image_generation;
} mpt_displace_info;
int mpt_mesh_set_displacement(mpt_ctx *ctx, int mesh_id, int image_id, int mode, int channel, double strength, double midlevel);
int mpt_mesh_set_displacement_params(mpt_ctx *ctx, int mesh_id, double strength, double midlevel);
int mpt_displace_stats(mpt_ctx *ctx, mpt_displace_info *out);
int mpt_displace_kernel_time(mpt_ctx *ctx, double *displace_ms, int *launches);
int mpt_displace_corners(const int32_t *faces /* [nfaces][3] */, int64_t nfaces, int32_t nverts, int32_t *corner /* [nverts] */);

/* Scatter: N instances of a mesh placed over a SURFACE object of the table on the device -- grass on a displaced terrain, rivets on a
 * skinned character (Blender's "distribute points on faces" + "instance on points").  The instances are ordinary objects of the
 * table with contiguous ids; their world matrices are written on the device, inside mpt_compose, and they are STICKY: an instance
 * remembers the face and the barycentric point it was born on, so that when the surface is posed, displaced or moved again only the
 * placement kernel runs again.  Instance and face counts stay constant: mpt_refit_tree refits.
 * The definition.  All arithmetic is f64, every sum and product in the order written, without contraction.
 *   Draws: mix(z) is SplitMix64's finaliser: z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31, all modulo 2^64.  draw(i, k) = mix(mix(seed) + 16 i + k);
 *     unit(i, k) = ((draw(i, k) >> 11) + 0.5) * 2^-53.
 *   World points: corner c of face g of the surface S is record 3 g + c of S's final object-space copy in the pool -- the mesh, or
 *     its deformed / subdivided / displaced copy: what mpt_compose reads for S -- placed by S's world matrix W with the composition's
 *     expressions for a position, ph = (p, 1) . W^T, P = ph.xyz / ph.w, NOT rounded to f32.
 *   Weights: area(g) = 0.5 * |cross(P1 - P0, P2 - P0)|.  dens(g) = 1 without a density image; with one, its channel (the
 *     displacement's codes) sampled at the mean ((u0 + u1) + u2) / 3.0 of the face's three corner uvs by the displacement's bilinear
 *     rule, clamped to [0, 1], NaN counting as 0.  w(g) = area(g) * dens(g), 0 where that is not finite; wmax the largest;
 *     q(g) = (uint32) floor(w(g) / wmax * 2^24): integer shares make the scan exact whatever its shape.  A face whose weight is below
 *     2^-24 of the largest gets no instance.
 *   Selection: cdf is the exclusive scan of q in 64 bits, T = cdf[F].  For instance i: t = draw(i, 0) mod T, g the largest face with
 *     cdf[g] <= t; su = sqrt(unit(i, 1)), v = unit(i, 2), b1 = su * (1 - v), b2 = su * v, b0 = (1 - b1) - b2;
 *     scale = smin + (smax - smin) * unit(i, 3).  Yaw is a unit vector without trigonometry: for j = 0..7, x = 2 unit(i, 4 + 2j) - 1,
 *     y = 2 unit(i, 5 + 2j) - 1; the first pair with 2^-20 < x x + y y <= 1 gives (cy, sy) = (x, y) / sqrt(x x + y y); none, or
 *     random_yaw off: (1, 0).  The sticky record of an instance is {g, b1, b2, scale, cy, sy}.
 *   Placement: P = (b0 P0 + b1 P1) + b2 P2.  align MPT_SCATTER_ALIGN_NORMAL: N = cross(P1 - P0, P2 - P0) / its length, the geometric
 *     normal of the face as it is now (a collapsed face gives NaN); MPT_SCATTER_ALIGN_UP: N = up / |up|, normalised once.  Tangent and
 *     bitangent by Duff et al., "Building an Orthonormal Basis, Revisited": s = copysign(1, N.z), a = -1 / (s + N.z), b = (N.x N.y) a,
 *     B0 = (1 + (s (N.x N.x)) a, s b, -(s N.x)), T0 = (b, s + (N.y N.y) a, -N.y); Tn = cy T0 + sy B0, Bn = cy B0 - sy T0.  The
 *     instance's world matrix has the columns scale Tn, scale N, scale Bn, P and the bottom row 0 0 0 1: local +Y is the instance
 *     mesh's "up".
 * mpt_scatter_add: appends `count` objects of mesh_id with material mtlid; *first_obj is the first of their contiguous ids.  The mesh
 *   may be subdivided and displaced (the instances share its one copy).  Refuses, leaving the scene as it was: an unknown surface
 *   object or mesh; a surface that is itself an instance of a scatter; count < 1; a count that takes the scene to max_faces; smin or
 *   smax not finite, or smin > smax; an `up` that is zero or not finite; an align outside the enum; a mesh with morph targets or a
 *   skin (a deformable mesh has one copy per object); a density image id outside [-1, max_textures); a density channel outside the
 *   displacement's codes; with a density image, a corner uv of the surface's mesh that the displacement would refuse.
 * mpt_scatter_set_params: new parameters for a scatter (checked alike); the next mpt_compose selects and places again.
 * mpt_scatter_rescatter: a new seed; the next mpt_compose selects and places again.  The old seed on the same surface gives the old
 *   records bit for bit.
 * mpt_compose, with scatters: weights, scan and selection run for a scatter that is new or was changed by the two calls above;
 *   placement runs for the scatters that selected, for those whose surface is composed again in this call, and for all after
 *   objects were added or dropped; the instances placed are composed again with their surface.  One weight, one selection and one
 *   placement launch whatever the number of scatters.  Before anything changes it refuses a surface without faces and a density
 *   image that is not loaded, naming scatter, object and image; a surface whose largest weight is 0 is refused when the weights are
 *   there, and the scene and the composed model stay as they were.  A density image that changes later moves nothing until a rescatter.
 * mpt_object_set_world on an instance is refused, naming the scatter; mpt_object_set_material is allowed.  mpt_scene_clear drops the
 *   scatters with the objects.  The host's copy of an instance's matrix is not kept: mpt_scatter_get fetches the device's.
 * mpt_scatter_stats: scatters and their instances; what the last mpt_compose did: scatters that selected, scatters and instances
 *   placed, its weight / scan / selection / placement launches, and its reads of the largest weights by the host.
 * mpt_scatter_kernel_time: HIP-event times (ms) of the selection (weights, scan, records) and of the placement launches of the
 *   mpt_compose calls since the last call (either may be NULL), and the kernels launched.
 * mpt_scatter_get: the sticky records [count], the world matrices [count][16] and the shares q [F] of a scatter as the last
 *   mpt_compose left them on the device (any may be NULL); fails before that mpt_compose.
 * mpt_scatter_rule: selection and placement as a pure function (no context, no GPU): for world corners [nfaces][3][3], shares
 *   q [nfaces] and parameters (the density fields are not read), the records [count] and matrices [count][16] of instances
 *   first .. first + count - 1.  Returns 0, or 1 for arguments that name no scatter, 2 for shares that sum to 0.
 *
 * Spacing: a scatter with a minimum distance (Blender's "Poisson Disk" mode of "distribute points on faces").  A SPACED scatter has a
 * minimum distance r > 0 and a candidate count M >= count.  All of it is f64, every sum and product in the order written, without
 * contraction, as the rest of the definition.
 *   Candidates: candidate j (0 <= j < M) is, bit for bit, instance j of the selection above (draw(j, k), face, b1, b2, scale, yaw)
 *     over the same shares and cdf: a spaced scatter of `count` from M candidates and a plain scatter of M share their records.
 *   Position: the placement's point P_j = (b0 P0 + b1 P1) + b2 P2, the world corners those of the surface as it stands in this
 *     mpt_compose, unrounded.
 *   Conflict: d2 = ((dx dx) + (dy dy)) + (dz dz), r2 = r r; j and k conflict iff d2 < r2.  A distance of exactly r is allowed.  A
 *     coordinate that is not finite makes every comparison false: such a point conflicts with nothing.
 *   Elimination: in candidate order, j is kept iff no kept k < j conflicts with it -- the greedy pass over the list of points, the
 *     lexicographically first maximal independent set; candidate order is the priority, and the draws make it a random one.
 *   Instances: the first `count` kept candidates in candidate order; instance i's sticky record is that candidate's.  Placement,
 *     stickiness, refit and every later call are unchanged: when the surface deforms the instances keep their faces and points, so
 *     their distances follow the surface (stickiness wins, as with a density image); mpt_scatter_rescatter draws and eliminates again.
 *   Refusal: fewer than `count` kept: mpt_compose refuses, naming the scatter, the number kept, M, r and count; scene and composed
 *     model stay as they were, as for a surface without weight, and the scatters that were due stay due.
 * On the device the greedy pass runs as rounds over a state per candidate (undecided, kept, rejected): an undecided j looks at its
 *   conflicting lower-index neighbours; any kept: rejected; else none undecided: kept; else it waits.  A round is a launch; the host
 *   looks after every batch of rounds whether a scatter still waits.  Neighbours are found through a uniform grid, which is no
 *   part of the rule.  One launch of each kind per mpt_compose whatever the number of spaced scatters; a compose in which no
 *   spaced scatter selects launches none of it.
 * mpt_scatter_set_spacing: the minimum distance and the candidates of a scatter; min_distance == 0 makes it plain again (candidates
 *   is not read).  Refuses, naming them, a distance that is negative or not finite and candidates below the scatter's count or above
 *   2^24.  The next mpt_compose selects and places again.
 * mpt_scatter_get_spacing: the scatter's last elimination: candidates M, the number kept, the rounds it took on the device (at most
 *   the synchronous count of mpt_scatter_space_rule: states are updated in place), kept_flags [M] (1 or 0) and index [count], the
 *   candidate that became instance i (any may be NULL).  Fails before that mpt_compose and for a plain scatter.
 * mpt_scatter_spacing_stats: of the last mpt_compose: the spaced scatters that selected, their candidates and kept candidates, the
 *   most rounds one of them took, the grid kernels (5: positions, box, count, scan, fill), round kernels and compaction kernels
 *   launched, and the host's waits for the elimination (one per batch of rounds and one for the kept counts; mpt_scatter_stats
 *   counts them among its host_fetches).  All zero when no spaced scatter selected.
 * mpt_scatter_spacing_kernel_time: the HIP-event time (ms) of the eliminations of the mpt_compose calls since the last call -- from
 *   before the grid to behind the compaction, the host's waits between the batches of rounds included; it is part of the selection's
 *   time of mpt_scatter_kernel_time -- and their number.
 * mpt_scatter_space_rule: the elimination as a pure function (no context, no GPU) over points [n][3]: kept [n] (1 or 0) and *rounds,
 *   the rounds of the synchronous form, in which every candidate reads the states the round before left (either may be NULL).  All
 *   pairs are tested.  Returns 0, or 1 for n < 0, n > 0 without points, or an r that is negative or NaN.
 * mpt_scatter_space_points: a test door (as mpt_walk_trace): the device's grid and round kernels on explicit points [n][3], n up to
 *   2^24; kept [n] and *rounds as the device made them.  It follows a query's contract: launched at the call on the main stream
 *   and waited for; it changes nothing else in the context. */
enum { MPT_SCATTER_ALIGN_NORMAL = 0, MPT_SCATTER_ALIGN_UP = 1 };
typedef struct {
    double smin, smax;                  /* the range of the instances' scale */
    double up[3];                       /* MPT_SCATTER_ALIGN_UP: the instances' up direction (any length) */
    int32_t align, random_yaw;
    int32_t density_image, channel;     /* an image of the image pool (-1: none) and MPT_DISPLACE_R .. MPT_DISPLACE_MEAN */
} mpt_scatter_params;
typedef struct {
    int32_t face, pad;
    double b1, b2, scale, cy, sy;
} mpt_scatter_point;
typedef struct {
    int64_t scatters, instances, selected_scatters, placed_scatters, placed_instances;
    int64_t weight_launches, scan_launches, select_launches, place_launches, host_fetches;
} mpt_scatter_info;
int mpt_scatter_add(mpt_ctx *ctx, int surface_obj, int mesh_id, int count, uint64_t seed, int mtlid, const mpt_scatter_params *params,
                    int *scatter_id, int *first_obj);
int mpt_scatter_set_params(mpt_ctx *ctx, int scatter_id, const mpt_scatter_params *params);
int mpt_scatter_rescatter(mpt_ctx *ctx, int scatter_id, uint64_t seed);
int mpt_scatter_stats(mpt_ctx *ctx, mpt_scatter_info *out);
int mpt_scatter_kernel_time(mpt_ctx *ctx, double *select_ms, double *place_ms, int *launches);
int mpt_scatter_get(mpt_ctx *ctx, int scatter_id, mpt_scatter_point *points, double *worlds /* [count][16] */, uint32_t *q /* [F] */);
int mpt_scatter_rule(const double *corners /* [nfaces][3][3] */, const uint32_t *q, int64_t nfaces, const mpt_scatter_params *params,
                     uint64_t seed, int64_t first, int64_t count, mpt_scatter_point *points, double *worlds /* [count][16] */);
typedef struct {
    int64_t scatters, candidates, kept, rounds;
    int64_t grid_launches, round_launches, compact_launches, host_reads;
} mpt_scatter_spacing_info;
int mpt_scatter_set_spacing(mpt_ctx *ctx, int scatter_id, double min_distance, int64_t candidates);
int mpt_scatter_get_spacing(mpt_ctx *ctx, int scatter_id, int64_t *candidates, int64_t *kept, int32_t *rounds, uint8_t *kept_flags /* [candidates] */,
                            int64_t *index /* [count] */);
int mpt_scatter_spacing_stats(mpt_ctx *ctx, mpt_scatter_spacing_info *out);
int mpt_scatter_spacing_kernel_time(mpt_ctx *ctx, double *ms, int *eliminations);
int mpt_scatter_space_rule(const double *points /* [n][3] */, int64_t n, double r, uint8_t *kept, int32_t *rounds);
int mpt_scatter_space_points(mpt_ctx *ctx, const double *points /* [n][3] */, int64_t n, double r, uint8_t *kept, int32_t *rounds);

/* Refit: after the model's faces moved (mpt_compose after mpt_object_set_world, or mpt_load_model of as many faces), keep the trees
 * of the last mpt_build_tree and fit their boxes to the model again, on the device -- what a viewport does for a moved object instead of
 * building (the reference's add-on builds: blender.py:555-571).
 * mpt_refit_tree: keeps the topology of the last successful mpt_build_tree -- the hierarchy, the leaf order, every id row, tree_depth,
 *   fast_depth, wide_nodes, wide_depth, wide_stack, wide_ratio_permille -- and writes again, from the model as it is on the device now
 *   (uploaded first if mpt_load_model brought it), everything that build derived from vertex positions and material ids: the boxes
 *   of the reference tree (mpt_get_tree's bmin / bmax), of the binary tree the fast build walks and of the 4-wide records exact
 *   and quantised (mpt_get_wide), and the triangle records.  The bytes are those a build over the same topology would write.
 *   The leaf order never changes: a scene that was rearranged wholesale keeps a valid but slow tree, which mpt_refit_stats shows.
 *   Leaves the tree valid.  Never reads the host's copy of a composed model.  Refuses, each time naming build_tree(): when no
 *   tree was ever built; when an option that steers the build was set since; when the last build failed; when the tree was built
 *   with gpu_build = 0; when the model's face count is not the one the tree was built for (both numbers are named).
 *   0 and 1 faces are legal: there are no nodes, the triangle records alone are written.
 * mpt_refit_stats: faces the records hold a topology for (-1: none), its wide nodes, refits since the build, fetches of the model's
 *   host copy that refits caused since mpt_create (stays 0), whether mpt_refit_tree would be allowed for the model as it stands, and the cost of the binary tree -- the sum over every child box of
 *   every node record of area(child) / area(root), the boxes a random ray is expected to meet, summed in 2^-40 fixed point so
 *   that the same records give the same bits -- as built (taken by the first refit after a build, from the build's records)
 *   and as it is now; growth = cost_now / cost_built, 1 where cost_built is 0 or nothing was refitted yet.
 * mpt_refit_kernel_time: HIP-event time (ms) of the kernels of the mpt_refit_tree calls since the last call, and their count.
 * mpt_refit_allowed / mpt_refit_growth: the rule above and the growth figure as pure functions (no context, no GPU).  state: 0 no
 *   tree was ever built, 1 the records hold a topology, 2 an option was set since, 3 a later build failed.  Returns 0 when a refit
 *   is allowed, else 1 .. 5 in the order of the refusals above, with the words in why[why_size] (may be NULL). */
typedef struct {
    int64_t faces, wide_nodes, refits, host_fetches, allowed;
    double cost_built, cost_now, growth;
} mpt_refit_info;
int mpt_refit_tree(mpt_ctx *ctx);
int mpt_refit_stats(mpt_ctx *ctx, mpt_refit_info *out);
int mpt_refit_kernel_time(mpt_ctx *ctx, double *ms, int *launches);
int mpt_refit_allowed(int state, int built_faces, int built_on_device, int nfaces, char *why, int why_size);
double mpt_refit_growth(uint64_t cost_built, uint64_t cost_now);

/* Batch ray queries on the built tree: LinearBVH.intersect(ray, avoid), ptina/tree/lbvh.py:314-347, for n rays at once, by the
 * build the context's "mode" selects (strict: the reference tree in the reference's order; fast: the binary production tree) --
 * ptina_amd/csrc/query_kernel.hip, DESIGN.md section 3.15.
 * o, d: [n][3] origins and directions in world space.  A direction of any length: it is normalised for the caller, so depths are
 *   world distances.  A ray with a non-finite component, a zero direction, or a direction whose f32 normalisation is not finite is a miss.
 * avoid: [n] the face each ray ignores (-1, or any number that names no face: none), or NULL.
 * mpt_query_closest: per ray hit (0 / 1), depth (1e6, the reference's inf, on a miss), index (the face; -1 on a miss), u, v (the
 *   hit's barycentrics along the face's edges v1 - v0 and v2 - v0; 0 on a miss) and object: where mpt_compose made the model, the
 *   object whose range of faces holds index; -1 on a miss or where mpt_load_model brought the model.  Each [n]; each may be NULL.
 * mpt_query_occluded: occ [n] = !(hit == 0 || depth > dis), the reference's shadow test (path.py:50-51); dis [n], NULL = no limit.
 * Rays go to the device in chunks of at most `chunk` rays (0: 2^22; rounded up to a multiple of 256), which bounds the device
 *   memory whatever n is; the answers do not depend on it.  n = 0 succeeds and touches nothing.
 * Launched at the call, behind everything enqueued before (a deferred render lands first), and waited for.  A query changes
 *   nothing a render reads or writes: film, sampler, counters, selection and marks stay as they are.  Fails like mpt_render where
 *   no tree is built for the model as it stands (after mpt_load_model, mpt_compose, or an option that steers the build).
 * mpt_query_kernel_time: HIP-event time (ms) of the query kernels launched since the last call, and their launch count. */
int mpt_query_closest(mpt_ctx *ctx, int n, const float *o, const float *d, const int32_t *avoid,
                      int32_t *hit, float *depth, int32_t *index, float *u, float *v, int32_t *object, int chunk);
int mpt_query_occluded(mpt_ctx *ctx, int n, const float *o, const float *d, const float *dis, const int32_t *avoid, int32_t *occ, int chunk);
int mpt_query_kernel_time(mpt_ctx *ctx, double *ms, int *launches);

/* Test door in the mpt_unit_eval / mpt_mlt_trace idiom: n rays of the caller's through the traversal of the production PathEngine
 * kernels -- the in-wave state machine of ptina_amd/csrc/render_lane.h over one of its five walk types, each set up and stepped by
 * its render kernel's own code (ptina_amd/csrc/walk_eval.hip).  Production build only.
 * walk: MPT_WALK_*.  o, d, avoid, chunk and what is no ray: as mpt_query_closest takes them (chunks hold 2^16 rays at most).
 * dis == NULL: the closest hit.  hit (0 / 1), depth (1e6 on a miss), index (the face; -1), u, v (0): what the shading stage would
 *   be handed, the walk's own f32 numbers, no second evaluation.  Each [n]; each may be NULL.
 * dis [n]: the rays are shadow rays that look as far as dis; hit [n] = occluded, as the shading stage reads it; the other outputs
 *   are not written.
 * Fails -- it never falls back to another walk -- for a context in strict mode, where no tree is built for the model as it
 *   stands, for a 4-wide walk where the 4-wide tree was not built, and for an LDS walk of a scene that does not fit a CU's LDS
 *   (ptina_amd/csrc/lds_layout.h).  Launched at the call and waited for; changes nothing a render reads or writes. */
enum { MPT_WALK_GATHER = 0,      /* binary nodes gathered from memory (render_kernel_fast; 32 or 64 stack levels by the tree's depth) */
       MPT_WALK_LDS = 1,         /* binary nodes in LDS (render_kernel_lds) */
       MPT_WALK_WIDE_EXACT = 2,  /* 4-wide nodes with exact boxes, gathered (render_kernel_wide, wide_quant = 0) */
       MPT_WALK_WIDE_QUANT = 3,  /* 4-wide nodes with 8-bit boxes, gathered (render_kernel_wide) */
       MPT_WALK_LDS4 = 4,        /* 4-wide nodes in LDS (render_kernel_lds4, the headline kernel) */
       MPT_WALK_COUNT = 5 };
int mpt_walk_trace(mpt_ctx *ctx, int walk, int n, const float *o, const float *d, const int32_t *avoid, const float *dis,
                   int32_t *hit, float *depth, int32_t *index, float *u, float *v, int chunk);

/* Reprojection: after the camera or the model changed, carry film pass 0 over to the new view instead of starting from nothing --
 * the temporal half's first step of spatiotemporal variance-guided filtering (ptina_amd/csrc/history_kernel.hip, history.hip,
 * history_rule.h; the numpy restatement tests/reproject_ref.py).  A context remembers ONE rendered view,
 * the history:   render ... -> mpt_history_keep -> edit the scene / camera -> mpt_compose, mpt_refit_tree -> mpt_history_reproject -> render ...
 * The reference has nothing of the kind.  A context that never calls these entries behaves bit for bit as before.
 * mpt_history_keep: launches what is enqueued, then remembers the view as it stands: v2w and w2v as uploaded, the film size, the
 *   face count, a device copy of the model's vertex positions (36 bytes per face) and a G-buffer from one kernel that traces every
 *   pixel's centre ray, camera_generate(((i + 0.5) / nx) * 2 - 1, ((j + 0.5) / ny) * 2 - 1), by the build the context's "mode"
 *   selects: per pixel `face` (the face hit; -1 on a miss), `id` (the object of mpt_compose's table whose range of faces holds it;
 *   0 where mpt_load_model brought the model; -1 on a miss) and `depth` (the hit's distance along the normalised ray from its
 *   origin; 1e6 on a miss; in the production build evaluated once more in f64, as mpt_query_closest does).  Pixels outside the
 *   context's slab or stripes hold (-1, -1, 0).  Fails like mpt_render where no tree is built for the model as it stands.  Writes
 *   no film pass, no mark, no selection and no sampler state; a history kept before is replaced.
 * mpt_history_reproject: launches what is enqueued, then refuses -- naming the cause, and changing nothing -- when there is no
 *   history, when the film size or the model's face count is not the kept one, when no tree is built for the model as it
 *   stands, when max_history is not positive or +inf, when depth_tol is not finite and positive.  Else two kernels run.
 *   MOTION traces the centre ray of every pixel p = (i, j) of the context's share in the NEW view and scene; all arithmetic below
 *   is f32, one rounding per operation, never contracted.  A miss: cur_id = -1, and the pixel is BACKGROUND-KEPT (fx = i, fy = j,
 *   d_exp = 0) iff the kept and the current v2w and w2v are equal word for word; else it has no place in the kept view.  A hit on
 *   face f at barycentrics u, v and distance depth (the production build's second evaluation; the strict build's own values), with
 *   a, b, c the KEPT positions of f's corners: if the cameras are equal word for word and so are a, b, c and the current
 *   corners, the pixel is STATIC: fx = i, fy = j, d_exp = depth.  Else P = ((1 - u) - v) a + u b + v c per component, summed left
 *   to right; clip_k = ((M[k][0] P.x + M[k][1] P.y) + M[k][2] P.z) + M[k][3], M the kept w2v; no place unless clip.w > 0;
 *   x = clip.x / clip.w, y = clip.y / clip.w; fx = ((x + 1) 0.5) nx - 0.5, fy likewise with ny (pixel q's centre is q);
 *   o_k = ((V[k][0] x + V[k][1] y) + V[k][2] (-1)) + V[k][3], V the kept v2w, the kept camera's ray origin o.xyz / o.w;
 *   d_exp = sqrt((dx dx + dy dy) + dz dz) of d = P - that origin.  Per pixel one mpt_history_motion record: cur_id (the hit's
 *   object as `id` above), fx, fy, d_exp (NaN without a place) and flags (MPT_MOTION_*).  The records stay on the device until the
 *   next keep or drop; pixels outside the share hold all-ones words.
 *   RESAMPLE, one lane per pixel, reads the old pass 0 and writes a second buffer that then takes its place.  A pixel outside the
 *   share gets (0, 0, 0, 0) and is not counted.  A miss keeps its own old accumulators iff it is background-kept, the kept
 *   face there is -1 and they hold samples (background_kept), else zeros (background_reset).  A hit with no place, or with
 *   !(fx > -1 && fx < nx && fy > -1 && fy < ny) -- no tap of positive weight in the film -- gets zeros (offscreen).  Else, with
 *   x0 = floorf(fx), y0 = floorf(fy), tx = fx - x0, ty = fy - y0, the taps q = (x0 + a, y0 + b), a the outer loop and b the inner,
 *   both over 0, 1, weigh bw = (a ? tx : 1 - tx) (b ? ty : 1 - ty).  A tap is used iff bw > 0, q lies inside the film,
 *   F_old(q).w > 0, id_kept(q) == cur_id and |depth_kept(q) - d_exp| <= depth_tol d_exp.  A = sum bw F_old(q) over all four
 *   components (so taps weigh by their sample counts), B = sum bw, both started from -0 and summed in tap order; B == 0: zeros
 *   (disoccluded); else R = A / B per component, and if R.w > max_history then R = R (max_history / R.w): newer samples must be
 *   able to outweigh an old view.  F_new(p) = R (kept; statics counts the static ones among them).  A static pixel whose history
 *   is at or below the cap keeps its four accumulator words exactly.  The background-kept accumulators are capped the same way.
 *   Afterwards passes 1 and 2 are zero, the mark and the selection are dropped as mpt_clear drops them, the Sobol sampler and an
 *   mpt_hint_image hint are left alone, and the history is spent: the next reproject needs another keep (the G-buffer and the
 *   motion records stay readable).  stats (may be NULL): exact counts of the share's pixels by what became of them; kept +
 *   background_kept + disoccluded + offscreen + background_reset is the share.
 *   params NULL: max_history = 32, depth_tol = 0.02.
 * mpt_history_drop: forgets the history and releases its device memory (as growing the film does).
 * mpt_history_get_motion: the records of the last reproject, [nx * ny] at element x * ny + y.  mpt_history_get_gbuffer: the
 *   kept G-buffer, each [nx * ny] or NULL (a test door).  Both fail where there is nothing to read.
 * mpt_history_eval: test door in the mpt_noise_eval idiom -- the SAME resample launch on the caller's arrays, for any nx, ny >= 1
 *   with nx ny <= max_filmsize, the whole film as the share, in buffers of its own: f_old [nx * ny][4], face, id, depth, motion
 *   [nx * ny] in; f_new [nx * ny][4] and stats out (each may be NULL).  Touches nothing of the context's film or history.
 * mpt_history_kernel_time: HIP-event time (ms) of the kernels of the keep calls and of the reproject calls since the last call,
 *   and the count of both.
 * mpt_history_allowed: the refusal rule as a pure function (no context, no GPU).  Returns 0 when a reproject is allowed, else
 *   1 .. 6 in the order of the refusals above, with the words in why[why_size] (may be NULL). */
#define MPT_MOTION_NONE       0
#define MPT_MOTION_STATIC     1
#define MPT_MOTION_BACKGROUND 2
typedef struct { float max_history, depth_tol; } mpt_history_params;
typedef struct { int64_t kept, statics, background_kept, disoccluded, offscreen, background_reset; } mpt_history_stats;
typedef struct { int32_t cur_id; float fx, fy, d_exp; int32_t flags; } mpt_history_motion;
int mpt_history_keep(mpt_ctx *ctx);
int mpt_history_reproject(mpt_ctx *ctx, const mpt_history_params *params /* NULL = the defaults above */, mpt_history_stats *stats /* or NULL */);
int mpt_history_drop(mpt_ctx *ctx);
int mpt_history_get_motion(mpt_ctx *ctx, mpt_history_motion *out /* [nx*ny] */);
int mpt_history_get_gbuffer(mpt_ctx *ctx, int32_t *face, int32_t *id, float *depth);
int mpt_history_eval(mpt_ctx *ctx, const mpt_history_params *params, const float *f_old, const int32_t *face, const int32_t *id,
                     const float *depth, const mpt_history_motion *motion, int nx, int ny, float *f_new, mpt_history_stats *stats);
int mpt_history_kernel_time(mpt_ctx *ctx, double *keep_ms, double *reproject_ms, int *launches);
int mpt_history_allowed(int have_history, int kept_nx, int kept_ny, int nx, int ny, int kept_faces, int nfaces, int tree_valid,
                        float max_history, float depth_tol, char *why, int why_size);

/* Page-locked host buffers for the read-backs above: into such a buffer mpt_get_image /
 * mpt_fast_export_image / mpt_get_film_raw are one DMA; any other buffer is served through a
 * page-locked staging copy.  (The reference's get_image returns a fresh numpy array,
 * ptina/filmtable.py:48; FilmTable.get_image here builds that array on a recycled buffer of these.) */
void *mpt_host_alloc(size_t bytes);
void  mpt_host_free(void *p);

/* measurement */
int mpt_get_counters(mpt_ctx *ctx, mpt_counters *out);
/* Diagnostics (option "timeline" = 1): per wave of the last LDS-kernel launch, eight words: four 100 MHz timestamps
 * {start, scene copied to LDS, work queues found empty, exit}, then {time the wave left the tail finalisation, tiles it
 * finalised} and two words that are zero.
 * *nwaves = waves recorded. */
int mpt_get_timeline(mpt_ctx *ctx, unsigned long long *out /* [cap_waves][8] */, int cap_waves, int *nwaves);
int mpt_reset_counters(mpt_ctx *ctx);
/* Which SHADE stage the last render launch was compiled for: *feat = the feature mask (what option "shade_inst" reads: 0 plain,
 * 31 generic), *lean = 1 when it was the lean variant of the plain instantiation -- every material the model uses, and the default
 * material, has sheen and subsurface exactly 0 and untextured, and the kernel holds neither term -- else 0.  Both are -1 before
 * the first launch.  The variant renders the plain and the generic kernel's film bit for bit; the environment variable
 * MIPTINA_SHADE_LEAN=0, read when the context is created, keeps every launch off it (A/B timing). */
int mpt_get_shade_variant(mpt_ctx *ctx, int *feat, int *lean);
/* Diagnostics (options "lane_hist" = 1 and "count" = 1; no counterpart in the reference): out[0 .. 195) = how many NODE / LEAF / SHADE
 * stages the waves issued with k of their 64 lanes taking part ([3][65]); out[195 .. 231) = the lane-steps of those stages by bounce
 * depth and ray kind ([3][6][closest, shadow]); out[231 .. 255) = the gather kernels' NODE lane-steps by log2 bucket of the node's
 * (breadth-first) number.  n = words `out` holds (>= 255). */
int mpt_get_lane_hist(mpt_ctx *ctx, unsigned long long *out, int n);
/* Diagnostics: launch a one-workgroup kernel (`threads` lanes, `lds_bytes` of LDS) on a stream of its own
 * while the enqueued render launches keep running, and return the wall time until it has completed --
 * what a collective's kernel would wait for a CU beside the persistent render workgroups. */
int mpt_probe_kernel(mpt_ctx *ctx, int threads, int lds_bytes, double *usec);
/* Test door (the tail finalisation's soak: tools/soak.py, tests/test_parity_gpu.py): enqueue `count` device-to-device copies of
 * `mbytes` MiB on a stream of their own and return at once -- HBM / L2 traffic beside the render launches; count = 0 waits for
 * the copies enqueued so far.  Nothing in the reference corresponds (its film add is one kernel's `+=`, ptina/engine/path.py:93). */
int mpt_stress_copies(mpt_ctx *ctx, int mbytes, int count);
/* HIP-event time of the render kernels launched since the last call (ms) and their count */
int mpt_kernel_time(mpt_ctx *ctx, double *ms, int *launches);

/* Test door: ONE device function of the hot path evaluated on n rows of inputs by the build the context's "mode"
 * selects (the strict build's reference-order IEEE code or the production build's fast forms) -- the same inlined
 * functions the render kernels run.  Rows are 4-byte words (f32; i32 for the two hash kinds); the column counts
 * per kind are fixed (checked).  Holds the HIP code directly to vectors computed by the reference's own function
 * bodies (tests/golden/reference_l1.npz, reference_disney_cube.npz); each kind names the reference function it evaluates. */
enum {
    MPT_UNIT_SCHLICK = 0,         /* materials/microfacet.py:9-10   in: cos                                  out: 1 */
    MPT_UNIT_DIELECTRIC = 1,      /* materials/microfacet.py:14-27  in: etai, etao, cosi                     out: 1 */
    MPT_UNIT_GTR1 = 2,            /* materials/microfacet.py:31-34  in: cosh, alpha                          out: 1 */
    MPT_UNIT_GTR2 = 3,            /* materials/microfacet.py:38-41  in: cosh, alpha                          out: 1 */
    MPT_UNIT_SMITHGGX = 4,        /* materials/microfacet.py:45-48  in: cos, alpha                           out: 1 */
    MPT_UNIT_SAMPLE_GTR1 = 5,     /* materials/microfacet.py:69-71  in: u, v, alpha                          out: 3 */
    MPT_UNIT_SAMPLE_GTR2 = 6,     /* materials/microfacet.py:75-77  in: u, v, alpha                          out: 3 */
    MPT_UNIT_TANSPACE = 7,        /* common.py:213-217              in: normal3, v3                          out: tanspace(normal) @ v */
    MPT_UNIT_SPHERICAL = 8,       /* common.py:221-225              in: h, p                                 out: 3 */
    MPT_UNIT_DIR2TEX = 9,         /* common.py:234-239              in: dir3                                 out: 2 */
    MPT_UNIT_REFLECT = 10,        /* common.py:247-249              in: I3, N3                               out: 3 */
    MPT_UNIT_REFRACT = 11,        /* common.py:252-260              in: I3, N3, eta                          out: has_r, T3 */
    MPT_UNIT_BOX = 12,            /* geometries.py:24-46            in: lo3, hi3, o3, d3                     out: hit, near, far (fast build: far = -1) */
    MPT_UNIT_FACE = 13,           /* geometries.py:96-148           in: v0 v1 v2, o3, d3, vn0 vn1 vn2, vt0 vt1 vt2 (30)  out: hit, depth, s, t, normal3, texcoord2 */
    MPT_UNIT_SPHERE = 14,         /* geometries.py:159-177          in: pos3, rad2, o3, d3                   out: t */
    MPT_UNIT_AREA = 15,           /* geometries.py:58-74            in: pos3, dirx3, diry3, o3, d3           out: hit, depth, u, v */
    MPT_UNIT_DISNEY_BRDF = 16,    /* materials/disney.py:13-106     in: 14 parameters, normal3, sign, indir3, outdir3 (24)  out: rgb */
    MPT_UNIT_DISNEY_BOUNCE = 17,  /* materials/disney.py:13-50,115-233  in: 14 parameters, normal3, sign, indir3, samp3 (24) out: outdir3, pdf, color3 */
    MPT_UNIT_POWER_HEURISTIC = 18,/* engine/path.py:11-15           in: a, b                                 out: 1 */
    MPT_UNIT_WANGHASH = 19,       /* sampling/__init__.py:9-16      in: i32                                  out: i32 */
    MPT_UNIT_WANGHASH2 = 20,      /* sampling/__init__.py:20-23     in: i32, i32                             out: i32 */
    /* The kinds below read the context's SCENE (lights, images, materials, world light, camera) as the render kernels do,
     * through the launch parameters; vectors: tests/golden/reference_scene_units.npz.  A kind whose rows name something the
     * context does not hold (an image that is not loaded, a material id outside the table) fails with a message. */
    MPT_UNIT_LIGHT_HIT = 21,      /* light/__init__.py:51-81        in: ro3, rd3                             out: hit, dis, pdf, color3 */
    MPT_UNIT_LIGHT_SAMPLE = 22,   /* light/__init__.py:83-121       in: hitpos3, samp3                       out: dis, dir3, pdf, color3 */
    MPT_UNIT_IMAGE_SAMPLE = 23,   /* image.py:137-148 + common.py:183-192  in: id (as a float), x, y         out: rgba */
    MPT_UNIT_WORLD_AT = 24,       /* light/world.py:22-29           in: dir3                                 out: rgb */
    MPT_UNIT_MATERIAL_GET = 25,   /* mtllib.py:30-38,79-95 + materials/disney.py:13-50  in: mtlid (as a float), tu, tv  out: 14 parameters, speccolor3, sheencolor3, alpha, clearcoatAlpha (22) */
    MPT_UNIT_CAMERA_GENERATE = 26,/* camera.py:34-39                in: x, y                                 out: ro3, rd3 */
    MPT_UNIT_FACE_SIDE = 27,      /* model.py:88-101                in: rd3, vn0 vn1 vn2, s, t (14)          out: the normal get_geometries returns, 1 if it flipped Face.normal; the shading record is packed by the door, not by mpt_load_model: only the flip is under test */
    /* Disney.brdf / Disney.bounce as the plain and the plain + lean instantiation of the production SHADE compile them
     * (csrc/shade_feat.h; pt_device.h disney_brdf<MPT_FEAT_PLAIN, LEAN> / disney_bounce<...>): the columns of kinds 16 and 17.  On a
     * material the instantiation admits (plain: clearcoat = transmission = 0; lean: sheen = subsurface = 0 as well) the output is the
     * generic kind's word for word, up to the sign of a zero; vectors: tests/golden/reference_disney_cube.npz.  Production build only:
     * the strict build has no such instantiation and refuses the kinds with a message. */
    MPT_UNIT_DISNEY_BRDF_PLAIN = 28,   /* materials/disney.py:13-106     in: as kind 16 (24)                  out: rgb */
    MPT_UNIT_DISNEY_BOUNCE_PLAIN = 29, /* materials/disney.py:13-50,115-233  in: as kind 17 (24)              out: outdir3, pdf, color3 */
    MPT_UNIT_DISNEY_BRDF_LEAN = 30,    /* materials/disney.py:13-106     in: as kind 16 (24)                  out: rgb */
    MPT_UNIT_DISNEY_BOUNCE_LEAN = 31,  /* materials/disney.py:13-50,115-233  in: as kind 17 (24)              out: outdir3, pdf, color3 */
    MPT_UNIT_KINDS = 32
};
int mpt_unit_eval(mpt_ctx *ctx, int kind, const void *in, int in_cols, void *out, int out_cols, int n);

/* multi-GPU film gather over RCCL (one process per GPU).  uid = ncclUniqueId bytes (128). */
int mpt_comm_unique_id(char uid[128]);
int mpt_comm_init(mpt_ctx *ctx, const char uid[128], int nranks, int rank);
/* The split of the film between R ranks as a pure function (no context, no GPU): the float4 ranges (film index
 * x*ny + y) rank r owns, in ascending x = the order they are packed into its one message of the gather.
 * stripe_w == 0: one slab [r*nx/R, (r+1)*nx/R); stripe_w > 0: stripes r, r+R, ... of stripe_w columns.  Writes the
 * first `cap` pieces (offsets / counts in float4 elements; either may be NULL) and returns the number of pieces,
 * -1 for arguments that name no split. */
int mpt_comm_plan(int nx, int ny, int stripe_w, int r, int R, int64_t *offsets, int64_t *counts, int cap);
/* One message per peer: a share of several stripes is packed side by side, sent as one range and scattered into
 * the root's film by one kernel in front of the resolve; a one-range share travels film to film. */
int mpt_comm_gather_film(mpt_ctx *ctx, int pass, int root);
/* Test door, one GPU, no communicator: the pack and scatter halves of the gather for rank `as_rank` of `nranks`
 * sending to `root`, with a device copy standing in for the message.  film_in: the sender's film [nx*ny][4];
 * film_out: the root's film, updated in place.  Uses the context's film size and stripe width. */
int mpt_comm_selftest(mpt_ctx *ctx, int as_rank, int nranks, int root, const float *film_in, float *film_out);
int mpt_comm_barrier(mpt_ctx *ctx);
int mpt_comm_allreduce_max(mpt_ctx *ctx, double *value);
int mpt_comm_destroy(mpt_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif

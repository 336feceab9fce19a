// mpt_types.h -- structures shared by the host runtime (miptina.cpp) and the gfx950 kernels.
//
// HBM layout (all SoA-of-records, 16-byte aligned so every fetch is a dwordx4):
//   snode  float4[(n-1)*2]  reference-shaped node: {bmin.xyz, child0}, {bmax.xyz, child1}
//                           (tree/lbvh.py:48-53 keeps four separate arrays; one 32-B record here)
//   fnode  float4[(n-1)*4]  traversal node: both CHILD boxes + child ids in one 64-B record, axis by axis
//                           with the two children side by side so that a dwordx4 fetch lands in the
//                           register pairs v_pk_fma_f32 wants:
//                           {c0.lo.x, c1.lo.x, c0.hi.x, c1.hi.x} {..y..} {..z..} {id0, id1, -, -}
//                           id >= 0: internal node index; id < 0: leaf, slot = ~id
//   qnode  float4[nw*4]     quantised 4-wide node (the production gather kernel): {origin.xyz, scale.x} {scale.yz, lo_x, hi_x}
//                           {lo_y, hi_y, lo_z, hi_z} {ids}: a plane of child c is origin + byte c of the word * scale, boxes
//                           rounded outwards; four 16-B gathers per step instead of seven (the gathers are what the big
//                           scenes wait for, whatever their width)
//   wnode  float4[nw*8]     4-wide traversal node (gather kernel): the binary tree collapsed so that one 128-B
//                           record holds four child boxes, component by component with the four children side
//                           by side: {lo.x[4]} {hi.x[4]} {lo.y[4]} {hi.y[4]} {lo.z[4]} {hi.z[4]} {id[4]} {-};
//                           id >= 0: wide node index, id < 0: leaf, slot = ~id; an unused child is a point box at
//                           1e30 that no ray reaches
//   tgeo   float4[n*4]      per-leaf-slot triangle, ray-independent terms of geometries.py:118-148
//                           hoisted: {v0.xyz, D} {u.xyz, uu} {v.xyz, uv} {n.xyz, vv}
//   tfast  float4[n*3]      the production kernels' triangle record: plane normal n = u x v, the dual edge vectors
//                           a = (uv v - vv u) / D, c = (uv u - uu v) / D, and v0 in the .w lanes (derive_tfast_kernel)
//   tshade float4[n*4]      per-leaf-slot shading data: {n0.xyz, n1.x} {n1.yz, n2.xy} {n2.z, uv0.xy, uv1.x}
//                           {uv1.y, uv2.xy, mtlid}
//   mats   MptMaterial[m+1] the 12 Disney parameters of mtllib.py:44-56 + the terms derived from them, 160 B; the
//                           last record is the default material of mtllib.py:82-93 (mtlid -1)
//   P      float[B][dim]    Sobol points of the B frames of a batch (sobol.py:82-83 keeps one)
//   film   float4[passes][nx*ny], element x*ny + y (filmtable.py:14,37-39)
#pragma once

#include <stdint.h>

#define MPT_BLOCK 256          // 4 waves of 64; one 16x16 pixel tile, an 8x8 sub-tile per wave
#define MPT_TILE 16
#define MPT_MAX_BATCH 64       // frames per launch
// The eight per-XCD queue heads of a persistent launch sit MPT_QUEUE_STRIDE words apart -- each on a cache line of its own: device-
// scope atomics on words of ONE line are served one after the other (a single head saturates near 88 pulls per microsecond; the
// benchmark launch makes 52), so eight heads in one 32-byte block were still one queue to the memory system.  The tail
// finalisation's tile counter follows them on its own line.  MPT_QUEUE_WORDS = what a launch's block holds (zeroed per launch).
#ifndef MPT_QUEUE_STRIDE
#define MPT_QUEUE_STRIDE 32
#endif
#define MPT_QUEUE_WORDS (10 * MPT_QUEUE_STRIDE)
#define MPT_TIMELINE_WORDS 8    // diagnostics: 64-bit words per wave of the launch timeline (option "timeline")
#define MPT_MAX_LIGHTS 64
#define MPT_MAX_DEVICES 64     // device ids a process may hold contexts on (per-device launch caches)

struct MptVec4 { float x, y, z, w; };

// kernel launchers: C linkage between the objects of libmiptina.so, not part of its ABI
#define MPT_KERNEL_API extern "C" __attribute__((visibility("hidden")))

struct MptMaterial {
    float p[16];               // [0..2] basecolor, [3] metallic, [4] roughness, [5] specular, [6] specularTint,
                               // [7] subsurface, [8] sheen, [9] sheenTint, [10] clearcoat, [11] clearcoatGloss,
                               // [12] transmission, [13] ior
    int32_t tex[12];           // per parameter texture id, -1 = none
    int32_t any_tex;           // 1 if any tex != -1
    int32_t pad[3];
    float d[8];                // fast build, untextured materials: what Disney.__init__ derives from the parameters
                               // (disney.py:36-50) -- speccolor[3], sheencolor[3], alpha, clearcoatAlpha -- computed
                               // once per material by derive_materials_kernel with the same device code
};

struct MptLight {              // light/__init__.py:14-18
    MptVec4 color_size;        // rgb, size
    MptVec4 pos_type;          // xyz, type (as int bits)
    MptVec4 ax0, ax1, ax2;     // rows of the 3x3 axes matrix
};

// one contiguous float4 range of the film gather's pack / unpack (comm.cpp): count elements from src to dst
struct MptPiece { long long src, dst, count; };

// what the last SAH re-partition did (diagnostics / the traffic model of profiles/r06_build_table.json)
struct MptSahStats {
    int levels;                      // binned levels
    long long elems;                 // positions streamed, summed over the binned levels
    long long chunks, segments;      // summed over the binned levels
    long long part_words;            // words of chunk bins written, summed over the levels
    int tasks_small, tasks_big;      // ranges finished in LDS: <= 512 triangles, 513 ... 1024
    int t_sort_k, t_loop_k, t_max_k; // finish kernels, units of 1024 ticks of s_memtime: summed over the tasks in the sort / in the level loop, the longest task
    int task_levels, task_levels_max; // levels the tasks ran, summed / the most of one task
};

// device workspace of the SAH re-partition (sah_build.hip); capacities from mpt_sah_*_capacity(n)
struct MptSahBuffers {
    const float *verts; const int *leaf; int n;          // the LBVH build's inputs / leaf order, on the device
    MptVec4 *prim[2];                                    // [n][2]: {box lo, slot} {box hi, -} per position (ping-pong)
    int *seg[2]; size_t seg_cap;                         // [seg_cap][16] segment tables (this level / the next)
    int *dec;                                            // [seg_cap][8] this level's decisions
    int *ch_seg, *ch_left; size_t chunk_cap;             // [2][chunk_cap] chunk -> segment (this level / the next), [chunk_cap] left counts
    int *part; size_t part_words;                        // chunk bins of one level
    int *segbins; size_t segbin_words;                   // the bins of the segments that have several chunks
    int *tasks; size_t task_cap;                         // [task_cap][8] ranges the finish kernel takes
    int *meta;                                           // [16]
    MptSahStats *stats;                                  // host, optional
    volatile int *mail_host; int *mail_dev;              // host-pinned, device-mapped [32]: where the plan kernel leaves a level's outcome, or null
    MptVec4 *fnode;                                      // out: [n-1][4]
};

struct MptImage { int32_t nx, ny, base, pad; };   // image.py:14-16

// the LDS-resident kernels' record strides, region sizes and fit rule
#include "lds_layout.h"

// 16-bit tags of a launch's sample entries (film_ops.h): 0 = zeroed memory, 1 = a launch that keeps the combine pass, 2 ... 65535 =
// finalising launches in turn
enum { MPT_TAG_COMBINE = 1, MPT_TAG_FIRST = 2, MPT_TAG_PERIOD = 65534 };
enum { MPT_HIST_BASE = 32, MPT_HIST_WORDS = 3 * 65 + 3 * 6 * 2 + 24, MPT_COUNTER_WORDS = MPT_HIST_BASE + MPT_HIST_WORDS };   // + 24: node steps by log2 of the node's number (gather kernels)

struct MptRenderParams {
    int32_t nx, ny, x0, x1;                 // film size and the slab [x0,x1) this context renders
    int32_t nframes, chunk, nchunks, n;     // batch frames; frames per work item; items per tile; #triangles
    int32_t sobol_dim, nlights, world_tex, tiles_x;   // tiles_* : 16x16 tiles of the slab (strict build)
    int32_t tiles_y, ntiles;
    float sobol_inv_dim;                    // 1 / sobol_dim (quotient estimate of the draw index reduction)
    int32_t nitems, tile_w_shift, tile_h_shift;   // fast build: (2^w x 2^h tile, chunk) work items of this launch
    int32_t nwide;                          // records of qnode (render_kernel_lds4 copies them into LDS)
    // columns rendered: x = x0 + s*stripe_pitch + w, w < stripe_w, x < x1 (one contiguous slab: stripe_w = 2^30)
    int32_t stripe_w, stripe_pitch;
    int32_t partial_stride;                 // float4 per frame of the sample slab = (tile-padded columns of the share) * ny
    int32_t lds_nmats;                      // material records render_kernel_lds4 keeps in LDS besides the default one
    int32_t skip_dark;                      // 1: shadow rays whose candidate direct light is exactly zero are not traced (production build)
    int32_t default_mtl;                    // index of the default material's record in mats (fast build)
    float world_fac[4];
    float v2w[16];
    const MptVec4 *snode;
    const MptVec4 *fnode;
    const MptVec4 *wnode;                    // 4-wide traversal nodes (scenes that do not fit LDS), or null
    const MptVec4 *qnode;                    // the same nodes with the child boxes quantised to 8 bits (64-B records), or null
    const MptVec4 *tgeo;
    const MptVec4 *tshade;
    const MptVec4 *tfast;                    // production build: 48-byte triangle records {n, v0.x}{a, v0.y}{c, v0.z} derived from tgeo
    const MptMaterial *mats;
    const MptLight *lights;
    const MptImage *images;
    const MptVec4 *texels;
    const float *P;                          // [nframes][sobol_dim]
    MptVec4 *film0;                          // pass 0 (path) / unused by preview
    MptVec4 *film1;                          // pass 1 (albedo)
    MptVec4 *film2;                          // pass 2 (normal)
    MptVec4 *partial;                        // fast build: per-sample radiance [nframes][columns of the share][ny]
    unsigned long long *counters;            // mpt_counters when counting, else unused
    unsigned int *work_counter;              // persistent kernels: 8 per-range item counters
    int *stack_spill;                        // wide kernel: the overflow stack entries (128 - the LDS levels) of every lane of the grid
    unsigned int *watchdog;                  // host-pinned flag a persistent wave raises when it gives up
    // Tail finalisation (fast build): a wave that has run out of work sums, resolves and writes out the tiles
    // whose samples are all in the slab, while other waves still drain their last paths.  fin_counter: the next tile to
    // finalise (zeroed with the queue heads), null = the combine pass does it after the launch; slab_tag: the 16-bit tag both
    // 8-byte halves of every sample entry of THIS launch carry (their ready flags, film_ops.h; 1 when fin_counter is null);
    // image_out: where the resolved pixel goes as well (FilmTable.get_image's array, device-visible), or null
    unsigned int *fin_counter;
    MptVec4 *image_out;
    uint32_t slab_tag;                       // MPT_TAG_COMBINE, or MPT_TAG_FIRST + launch number mod MPT_TAG_PERIOD
    // Diagnostics (option "lane_hist", counting kernels only): counters + MPT_HIST_BASE holds, per issued NODE / LEAF / SHADE stage, how
    // many of the wave's 64 lanes took part ([3][65] stage counts) and whose lanes they were ([3][6 depths][2 ray kinds] lane-steps)
    int32_t lane_hist;
    // render_kernel_lds4 measures distances along a ray in units of 1 / t_scale (a power of two, so every comparison comes out as it
    // would unscaled): no box of the scene is entered farther than 1 / t_scale from any ray origin, which lets the clamp bit of an
    // FMA stand for max(t, 0) (pt_device.h LdsWalk4::T_SCALED).  t_unscale = 1 / t_scale
    float t_scale, t_unscale;
    int32_t pad3;
    unsigned long long *timeline;            // diagnostics: per wave {start, scene ready, queue empty, exit} in
                                             // 100 MHz ticks, or null
};

// one launch of the Metropolis chain kernel (mlt_kernel.hip): chain state, splat records, the engine's parameters
struct MptMltArgs {
    float *X;                                // [2][nchains][32] chain vectors; bit[c] names chain c's current half
    float *L;                                // [nchains][3] the current path's radiance (L_old)
    int32_t *bit;
    uint32_t *keys;                          // [K][nchains] film element of iteration t0 + k's proposal
    MptVec4 *vals;                           // [K][nchains] its radiance (r, g, b, 0)
    int32_t nchains, t0, K;
    uint32_t seed;
    float lsp, sigma;                        // MLTPathEngine.LSP / Sigma
};

// one launch of a batch-query kernel (query_kernel.hip): n rays, what names their faces, and where the answers go.  The tracers speak
// in leaf slots (the order of tgeo / tfast); callers speak in faces of the model: leaf and slot_of translate
struct MptQueryArgs {
    const float *o, *d;                      // [n][3] origins and directions (any length: the lane normalises)
    const int32_t *avoid;                    // [n] the face each ray ignores (-1: none), or null
    const float *dis;                        // [n] occlusion: how far each ray looks, or null (as far as MPT_INF)
    const int32_t *leaf, *slot_of;           // [faces] slot -> face and face -> slot of the built tree
    const int32_t *first;                    // [nobj] the objects' first faces (compose.hip), or null: the model has no object table
    int32_t nobj, n;
    // structure-of-arrays answers, each [n] or null: the closest kernel's ...
    int32_t *hit; float *depth; int32_t *index; float *u, *v; int32_t *object;
    int32_t *occ;                            // ... and the occlusion kernel's
};

// The film's reprojection.  One launch of the G-buffer or the motion kernel (history_kernel.hip): the tables
// that name a hit's face and object, where the G-buffer goes or -- the motion kernel -- the kept view, the kept and the current
// vertex positions and where the motion records go
struct MptMotion;                           // history_rule.h
struct MptHistoryArgs {
    const int32_t *leaf;                     // [faces] slot -> face of the built tree
    const int32_t *first;                    // [nobj] the objects' first faces (compose.hip), or null: every hit is object 0
    int32_t nobj;
    int32_t same_camera;                     // motion: the kept and the current camera matrices are equal word for word
    int32_t *face, *id; float *depth;        // G-buffer: [nx * ny] each
    const float *kept_verts;                 // motion: [faces][3][3] the positions the kept view saw
    const float *cur_verts;                  // motion: [faces * 3][8] the model as it is on the device now
    float kept_w2v[16], kept_v2w[16];        // motion: the kept camera, as uploaded
    MptMotion *motion;                       // motion: [nx * ny]
};
// one launch of the resample kernel (history.hip): the old accumulators, the kept G-buffer, the motion records, the share of the
// film this context renders (stripe_w = 0: the slab [x0, x1) alone) and the two parameters
struct MptResampleArgs {
    const MptVec4 *f_old; MptVec4 *f_new;
    const int32_t *face, *id; const float *depth;
    const MptMotion *motion;
    int32_t nx, ny, x0, x1, stripe_w, stripe_idx, stripe_mod;
    float max_history, depth_tol;
};

// one conversion launch of mpt_get_display (display.hip): mpt_display_params as the kernels take it
struct MptDisplayArgs {
    int32_t op, transfer, layout, dither;    // MPT_TONE_*, MPT_TRANSFER_*, MPT_LAYOUT_* of include/miptina.h
    float exposure;                          // a manual exposure (the metered one is read from the device)
    float white2, inv_gamma;                 // white * white and 1 / gamma, in f32
};

// A run of a launch's blocks (run_table.h: the plan of a table of them, the lookup a block does in it).  For the deform and subdivision
// launches `item` is a row of the launch's table -- an object, a job -- and the run takes the blocks from `block`, a chunk of the row's items
// each; for compose_kernel `item` is the run's first output workgroup: [item, item + next run's `block` - block) are the blocks from `block`
struct MptRun { int32_t item, block; };

// scene composition (compose.hip): one object of the table -- a mesh of the pool placed by a world matrix.  `epoch` names the
// mpt_compose call that last changed the record: a partial launch rewrites the output of the objects that carry its epoch
struct alignas(16) MptComposeObj {          // 160 bytes: the matrix is read as 16-byte words
    int32_t first_face, nfaces;              // the object's range of output faces
    int32_t mesh_vert;                       // its mesh's first vertex in the pool (nfaces * 3 records from there)
    int32_t mtlid;
    uint32_t epoch;
    int32_t pad[3];
    double world[16];                        // row-major, as numpy holds it
};

// mesh deformation (deform.hip): the caps of a mesh's skin and morph targets and one deformable object of a launch -- where its
// mesh's records and its deformed copy lie in the pool, and where its mesh's deltas / skin and its own pose lie in their arenas
#define MPT_DEFORM_MAX_JOINTS 256           // 96 bytes of LDS each: 24 KB of the CU's 160 KiB
#define MPT_DEFORM_MAX_TARGETS 64
#define MPT_DEFORM_CHUNK 1024               // corners per workgroup: four per lane
struct MptDeformObj {                       // 48 bytes
    int32_t src_vert, dst_vert;              // first pool vertex of the mesh and of the object's deformed copy
    int32_t nverts;                          // corners: 3 x faces
    int32_t ntargets, njoints;               // 0: no morph targets / no skin
    int32_t pad;
    int64_t delta_at;                        // the mesh's deltas [ntargets][nverts][6] f32: first float in the arena
    int64_t skin_at;                         // its skin: first corner in the arenas of indices [.][4] u16 and weights [.][4] f32
    int64_t pose_at;                         // the object's pose: ntargets weights, then njoints 3x4 matrices, f64: first double
};

// keyframe animation (anim.hip, anim_rule.h): a track of a clip as the arenas hold it, and one bound object of a launch -- where its
// mesh's skeleton, its clip's tracks and its own pose lie in their arenas, and its binding
enum { MPT_ANIM_T = 0, MPT_ANIM_R = 1, MPT_ANIM_S = 2, MPT_ANIM_W = 3 };            // a track's path: translation, rotation, scale, morph weights
enum { MPT_ANIM_STEP = 0, MPT_ANIM_LINEAR = 1, MPT_ANIM_CUBICSPLINE = 2 };          // ... and its interpolation
#define MPT_ANIM_REST 10                    // doubles of a joint's rest pose: translation3 rotation4 (xyzw) scale3
struct MptAnimTrack {                       // 32 bytes
    int32_t target, path, interp, nkeys;     // the joint (-1: the morph weights), MPT_ANIM_T .. _W, MPT_ANIM_STEP .. _CUBICSPLINE, keys >= 1
    int64_t time_at;                         // its key times [nkeys] f32: first float in the arena of times
    int64_t value_at;                        // its values [nkeys][C] f32 (CUBICSPLINE: [nkeys][3][C], in-tangent value out-tangent): first float
};
struct MptAnimObj {                         // 160 bytes
    int32_t njoints, ntargets;               // of its mesh (0: no skeleton / no targets)
    int32_t ntracks, loop;                   // of its clip; of its binding
    int32_t levels, blend;                   // the greatest depth of a joint of the skeleton (a root: 0); 1: it has a second binding (the fields below)
    int64_t joint_at;                        // the skeleton: first joint in the arenas of parents, depths, rest poses [.][10] and inverse binds [.][12]
    int64_t track_at;                        // the clip: first track in the arena of tracks
    int64_t pose_at;                         // the object's pose (MptDeformObj::pose_at): what the kernel writes
    double offset, speed, t0, t1;            // the binding, and the clip's span
    // the second binding: its clip, its own offset, speed, loop and span, and the weight's fade
    int32_t ntracks_b, loop_b;
    int64_t track_b_at;
    double offset_b, speed_b, t0_b, t1_b;
    double w0, w1, fade_start, fade_duration;
};
// ... and one object of a launch that an object clip moves (motion_kernel): its row of the object table, its clip and its binding
struct MptMotionObj {                       // 264 bytes
    int32_t obj, ntracks;                    // the row of the object table whose world matrix the kernel writes; the clip's tracks (T, R, S of target 0: at most 3)
    int32_t loop, pad;
    int64_t track_at;
    double offset, speed, t0, t1;
    double rest[MPT_ANIM_REST];              // translation3 rotation4 (xyzw) scale3: what a path without a track keeps
    double base[16];                         // row-major 4x4: world = base . local
};
// ... and one bound child of a launch of hierarchy_kernel (hierarchy.hip): its row of the object table, its
// parent's, the palette entry it follows, and its local matrix -- as it stands, or as a motion binding gives it
#define MPT_HIER_MAX_DEPTH 64               // the deepest chain: a child of a root has depth 1
#define MPT_HIER_ONE_GROUP 1024             // up to this many children to evaluate, one workgroup walks the levels in one launch
struct MptHierObj {                         // 272 bytes
    int32_t obj, parent;                     // the row whose world matrix the kernel writes; the row it reads the parent's from
    int32_t ntracks, loop;                   // -1: no motion binding, `local` is the local matrix; else the clip's tracks, and local = `local` . T R S
    int64_t track_at;
    int64_t joint_at;                        // -1: world = world(parent) . local; else the first double of the palette entry M_j in the pose buffer
    double offset, speed, t0, t1;
    double rest[MPT_ANIM_REST];
    double local[16];                        // row-major 4x4: the local matrix, or the motion binding's base
};
struct MptHierLevels { int32_t at[MPT_HIER_MAX_DEPTH + 1]; };   // a launch's items are ordered by depth: level l holds the items [at[l], at[l + 1])

// Loop subdivision (subdiv.hip): the caps, the kinds of a vertex rule (subdiv_rule.h), one job of a launch -- a subdivided copy: where
// its control records and the copy lie in the pool, where its mesh's topology block lies in the arena of words and its own f64
// vertices in the workspace
#define MPT_SUBDIV_MAX_LEVELS 5
#define MPT_SUBDIV_MAX_FACES (1 << 24)      // faces of a last level the topology function takes (the context's max_faces is lower)
#define MPT_SUBDIV_CHUNK 256                // items (vertices or faces) per workgroup: one per lane
enum { MPT_SUBDIV_VERT_INT = 0, MPT_SUBDIV_VERT_BND = 1, MPT_SUBDIV_EDGE_INT = 2, MPT_SUBDIV_EDGE_BND = 3 };
// A rule's head is kind | n << 2 | variant << 28.  Variant 0 is the plain rule, all an uncreased mesh has; a creased mesh (section
// 3.19.1) has beside it, on kind VERT_INT, a vertex of two sharp edges that blends, one of three or more that blends, one that stays,
// and on kind EDGE_INT an edge of fractional sharpness
#define MPT_SUBDIV_VARIANT_SHIFT 28
#define MPT_SUBDIV_N_MASK ((1 << 26) - 1)
enum { MPT_SUBDIV_PLAIN = 0, MPT_SUBDIV_BLEND_CREASE = 1, MPT_SUBDIV_BLEND_CORNER = 2, MPT_SUBDIV_FIXED = 3, MPT_SUBDIV_BLEND_EDGE = 1 };
// Catmull-Clark (section 3.19.2): a rule that is Catmull-Clark's and not Loop's has this bit in its variant, beside the blend -- on
// kind VERT_INT the interior vertex (ring, then its faces' points), on EDGE_INT the interior edge (a b, then two face points), on
// EDGE_BND the face point (its corners).  A Loop mesh has no such head
#define MPT_SUBDIV_CC 4
#define MPT_SUBDIV_MAX_CORNERS 64           // corners of a polygon of a Catmull-Clark cage
struct MptSubdivJob {                       // 128 bytes, and no more: with a word added the refine launches measured slower
    int32_t src_vert, dst_vert;              // first pool vertex of the control records (the mesh or a deformed copy) and of the subdivided copy
    int32_t levels, nfaces;                  // L, and the faces of the last level: k * 4^L
    int64_t topo_at;                         // the mesh's topology block: first word in the arena
    int64_t work_at;                         // the job's workspace: first double (even)
    int32_t nv[MPT_SUBDIV_MAX_LEVELS + 1];   // vertices of level 0..L
    int32_t rule_at[MPT_SUBDIV_MAX_LEVELS + 1];   // words from topo_at: [l] the rules of level l's vertices; [0] (the first corners are the block's first words): a Catmull-Clark mesh's table of level-1 quads (the polygon's first triangle, n | i << 8), 0 for a Loop mesh
    int32_t pos_at[MPT_SUBDIV_MAX_LEVELS + 1];    // doubles from work_at: [l] the positions [V_l][3] of level l ([0]: level 0 is read from the pool; a displaced copy's displaced positions [V_L][3])
    int32_t nrule_at, face_at;               // words from topo_at: the last level's rings, its faces' vertex ids
    int32_t vrec_at;                         // doubles from work_at (even): the last level's records (one per vertex, or per sector of a creased mesh), 32 bytes each: pos3 nrm3 as f32, 8 bytes unused
    int32_t npos_at;                         // doubles from work_at: the positions the normals are taken of -- pos_at[L], or pos_at[0] of a displaced copy
    int32_t srule_at, nrec;                  // words from topo_at: the rules of the last level's records, and their number -- nrule_at and V_L, or a creased mesh's sectors
};

// Texture displacement of a subdivided copy (displace.hip): the row of the displacement launch's table beside the copy's MptSubdivJob
// (same index) -- the image as the host knows it, the first-corner table of the mesh's last level and the parameters
struct MptDisplaceJob {                     // 48 bytes
    int32_t mode, channel;                   // MPT_DISPLACE_NORMAL / _VECTOR, MPT_DISPLACE_R .. _MEAN of include/miptina.h
    int32_t nx, ny;                          // the image [nx][ny] ...
    int64_t texel_at;                        // ... its first texel in the arena of rgba f32 texels
    int64_t corner_at;                       // first word in the arena of topology words: [V_L] the first corner 3 g + c of every last-level vertex
    double strength, midlevel;
};

// Scatter (scatter.hip): instances of a mesh placed over a surface object of the table.  MptScatterPoint is the STICKY RECORD of an
// instance -- the face it was born on, its barycentric point there, its scale and its yaw as a unit vector -- which the placement
// kernel turns into the instance's world matrix whenever the surface moves.  MptScatterJob is one scatter of a compose's launches:
// the rows of the object table it reads and writes, where its faces' weights and its records lie in their arenas, its parameters
struct MptScatterPoint {                    // 48 bytes (include/miptina.h has it as mpt_scatter_point)
    int32_t face, pad;
    double b1, b2;                           // the barycentric weights of corners 1 and 2 (b0 = (1 - b1) - b2)
    double scale, cy, sy;
};
enum { MPT_SCATTER_CHUNK = 256 };           // items (faces or instances) per workgroup: one per lane
struct MptScatterJob {                      // 112 bytes
    int32_t surf_obj, first_obj;             // rows of the object table: the surface, the first instance
    int32_t nfaces, count;                   // F of the surface, N instances
    int64_t face_at;                         // first entry of the arenas w, q and cdf (F + 1 entries each)
    int64_t point_at;                        // first sticky record in the arena of points
    uint64_t key;                            // mix(seed)
    int32_t align, random_yaw;               // MPT_SCATTER_ALIGN_NORMAL / _UP of include/miptina.h
    int32_t density, channel;                // 1: a density image is sampled; MPT_DISPLACE_R .. _MEAN
    int32_t nx, ny;                          // the image [nx][ny] ...
    int64_t texel_at;                        // ... its first texel in the arena of rgba f32 texels
    double smin, smax;
    double up[3];                            // unit length (the host normalises it once)
};
// Spacing (scatter_space.hip): MptSpaceJob is one spaced scatter of a compose's elimination launches -- or the explicit points of
// mpt_scatter_space_points -- and MptSpaceGrid the uniform grid the fold kernel lays over its candidates' positions
struct MptSpaceJob {                        // 72 bytes
    int32_t job;                             // its row of the compose's table of scatters (-1: explicit points, nothing is selected or compacted)
    int32_t m, count;                        // M candidates, the first `count` kept become the instances
    uint32_t mask;                           // buckets of its hash table - 1 (a power of two)
    int64_t cand_at;                         // its candidates' records in the arena of records (behind the sticky ones)
    int64_t at;                              // its first entry of the workspace arrays: positions (3 each) and items
    int64_t bucket_at;                       // its first bucket
    int64_t state_at;                        // its candidates' states, which stay until its next elimination
    int64_t point_at;                        // its sticky records, and beside them the candidates they came from
    double r, r2;                            // the minimum distance and r r
};
struct MptSpaceGrid {                       // 48 bytes
    double lo[3], h;                         // the corner of the finite positions' box and the cell edge
    int32_t n[3], pad;                       // cells along each axis
};
enum { MPT_SPACE_BATCH = 8 };               // rounds launched between two looks of the host at the scatters still undecided

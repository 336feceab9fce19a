/* lds_layout.h -- how the two LDS-resident render kernels lay a scene out in a CU's LDS, which scenes fit, and which kernel a
 * launch gets: written once, for the host that asks for the bytes and the kernels that carve them up.
 *
 * A launch of render_kernel_lds / render_kernel_lds4 (render_kernel.hip) takes its whole scene into dynamic LDS.  The host
 * (miptina.cpp mpt_flush) decides whether the scene fits and how many bytes to ask for; the kernel places its regions in those
 * bytes.  If the two disagreed the kernel would read or write LDS it did not ask for, so both take the sizes from the functions
 * below.  The regions, in order, in float4 (16-byte) units:
 *
 *   binary nodes (render_kernel_lds):  [ (n-1) node records MPT_LDS_NODE_STRIDE bytes apart, the region padded to 16 | n x 3 triangle
 *       float4 (tfast) | (default_mtl+1) x 6 material float4 | n material-record bytes, padded to 16 | stack levels x 1024 int16 ]
 *   4-wide nodes (render_kernel_lds4): [ nwide node records of MPT_LDS4_NODE_STRIDE bytes | (n+1) x 3 triangle float4 (tfast; record n:
 *       the unused slots' NaNs) | (lds_nmats+1) x 6 material float4 (the records the model uses, then the default one) |
 *       n material-record bytes, padded to 16 | stack levels x 1024 int16 ]
 *
 * Plain C, no dependencies, like shade_feat.h: the host runtime and the kernels include it, and a CPU test
 * (tests/test_lds_layout_cpu.py) compiles it on its own and holds it to an independent restatement.  Everything is 32-bit
 * arithmetic, as in the kernels; the fit predicates test the counts' bounds BEFORE they compute a size, so that no face count the
 * API accepts (up to 2^26, where (n - 1) x 72 leaves 32 bits) overflows.
 */
#pragma once

#if defined(__HIPCC__)
#define MPT_LDS_FN __host__ __device__ static inline
#else
#define MPT_LDS_FN static inline
#endif

/* LDS-resident kernel: bytes from one node record to the next in LDS.  72, not 64: a ds_read_b64 is served in two
 * groups of 32 lanes over 64 banks of 4 bytes, and with 64-byte records every lane's read of a given plane lands
 * on one of FOUR bank pairs (16 i mod 64); with 72-byte records on one of 32 (18 i mod 64) -- reads stay 8-byte aligned */
#ifndef MPT_LDS_NODE_STRIDE
#define MPT_LDS_NODE_STRIDE 72
#endif
#ifndef MPT_LDS4_NODE_STRIDE
#define MPT_LDS4_NODE_STRIDE 112     /* bytes between the 4-wide node records in LDS (render_kernel_lds4: seven float4 of a wnode record) */
#endif
#define MPT_LDS_MAT_VEC4 6           /* float4 of a material record kept in LDS: p[0..15] and the derived terms d[0..7] */

enum {
    MPT_LDS_BUDGET = 160 * 1024,     /* a gfx950 CU's LDS: what one persistent workgroup per CU can ask for */
    MPT_LDS_LANES = 1024,            /* lanes the 16-bit stacks are laid out for (the largest workgroup) */
    MPT_LDS_LEVEL_BYTES = MPT_LDS_LANES * 2   /* one stack level: an int16 per lane */
};

/* region sizes in float4 units; a region starts where the one before it ends */
typedef struct { int nnode4, ntri4, nmat4, nmtl4; } MptLdsRegions;

/* binary nodes: node records MPT_LDS_NODE_STRIDE bytes apart (bank spreading), the region rounded up to whole float4 */
MPT_LDS_FN MptLdsRegions mpt_lds_regions(int n, int default_mtl) {
    MptLdsRegions r;
    r.nnode4 = ((n - 1) * MPT_LDS_NODE_STRIDE + 15) >> 4;
    r.ntri4 = n * 3;
    r.nmat4 = (default_mtl + 1) * MPT_LDS_MAT_VEC4;
    r.nmtl4 = (n + 15) >> 4;
    return r;
}

/* 4-wide nodes: one triangle record more (the unused slots' leaf), only the material records the model uses (+ the default one) */
MPT_LDS_FN MptLdsRegions mpt_lds4_regions(int n, int nwide, int lds_nmats) {
    MptLdsRegions r;
    r.nnode4 = nwide * (MPT_LDS4_NODE_STRIDE / 16);
    r.ntri4 = (n + 1) * 3;
    r.nmat4 = (lds_nmats + 1) * MPT_LDS_MAT_VEC4;
    r.nmtl4 = (n + 15) >> 4;
    return r;
}

/* where the stacks start = float4 the scene takes */
MPT_LDS_FN int mpt_lds_scene_vec4(MptLdsRegions r) { return r.nnode4 + r.ntri4 + r.nmat4 + r.nmtl4; }

/* the launch's dynamic LDS: the scene + 2 KiB per stack level */
MPT_LDS_FN int mpt_lds_launch_bytes(MptLdsRegions r, int stack_levels) {
    return mpt_lds_scene_vec4(r) * 16 + stack_levels * MPT_LDS_LEVEL_BYTES;
}

/* stack levels the binary kernel asks for: the sentinel + one pending sibling (node or leaf) per level of the tree */
MPT_LDS_FN int mpt_lds_stack_levels(int fast_depth) { return fast_depth + 1; }

/* Can render_kernel_lds serve this scene?  The launch's LDS bytes if so, 0 if not. */
static inline int mpt_lds_fit_bytes(int n, int max_materials, int fast_depth) {
    if (n < 2) return 0;                                         /* a tree has a node */
    if (n >= 32768) return 0;                                    /* leaf ids (~slot) in an int16 stack */
    if ((n - 1) * (MPT_LDS_NODE_STRIDE / 8) >= 32768) return 0;  /* the LDS copy's node ids are byte offsets / 8 in an int16 stack */
    if (max_materials >= 256) return 0;                          /* a triangle names its record in one byte; the default one is record max_materials */
    if (fast_depth < 0 || fast_depth >= MPT_LDS_BUDGET / MPT_LDS_LEVEL_BYTES) return 0;   /* (the stacks alone: keeps the sum below in 32 bits) */
    const int bytes = mpt_lds_launch_bytes(mpt_lds_regions(n, max_materials), mpt_lds_stack_levels(fast_depth));
    return bytes <= MPT_LDS_BUDGET ? bytes : 0;                  /* the CU's 160 KiB */
}

/* Can render_kernel_lds4 serve it?  wide_stack: every stack level the 4-wide tree can ask for (a step leaves up to three entries
 * behind); lds_nmats: the material records the model uses (max_mtlid + 1).  The launch's LDS bytes if so, 0 if not. */
static inline int mpt_lds4_fit_bytes(int n, int nwide, int wide_stack, int lds_nmats) {
    if (n < 2 || nwide <= 0 || wide_stack <= 0) return 0;        /* the 4-wide tree was built (not too deep) */
    if (n >= 4095) return 0;                                     /* 16-bit ids: a leaf's is 16 * slot + 1, slot n the unused slots' */
    if (nwide > 65535 / MPT_LDS4_NODE_STRIDE) return 0;          /* 16-bit ids: a node's is its record's LDS address (nwide x stride < 65536) */
    if (lds_nmats < 0 || lds_nmats >= 255) return 0;             /* a triangle names its record in one byte; the default one is record lds_nmats */
    if (wide_stack > MPT_LDS_BUDGET / MPT_LDS_LEVEL_BYTES) return 0;   /* (the stacks alone: keeps the sum below in 32 bits) */
    const int bytes = mpt_lds_launch_bytes(mpt_lds4_regions(n, nwide, lds_nmats), wide_stack);
    return bytes <= MPT_LDS_BUDGET ? bytes : 0;                  /* the CU's 160 KiB */
}

/* Levels of the per-lane traversal stack of the kernels that gather the binary tree -- the gather render kernels, preview, brute,
 * Metropolis and the list pass, two instantiations each (path_common.h launch_by_stack): the sentinel and one pending sibling per
 * level of a tree `depth` levels deep, in 32 levels if they fit and in 64 otherwise */
MPT_LDS_FN int mpt_gather_stack_levels(int depth) { return depth + 2 <= 32 ? 32 : 64; }

/* ---------------------------------------------------------------- which kernel a render launch gets
 * The values are the public "last_kernel" numbers (include/miptina.h); 3 and 4 are retired. */
enum { MPT_KERNEL_GATHER = 0, MPT_KERNEL_LDS = 1, MPT_KERNEL_WIDE = 2, MPT_KERNEL_LDS4 = 5 };

/* what the choice reads: the build, three options, and the scene as mpt_build_tree left it */
typedef struct {
    int fast;                /* production build (the strict build has one kernel: the gather over the reference's tree) */
    int use_lds;             /* option "lds": scenes that fit a CU's LDS are served from it */
    int lds_wide;            /* option "lds_wide": ... over the 4-wide nodes (0: the binary ones) */
    int use_wide;            /* option "wide": walk the 4-wide nodes where the collapse was built */
    int nfaces;
    int wide_nodes;          /* 0: the 4-wide tree was not built (too deep) */
    int wide_stack;
    int have_wnode;          /* the exact-box 4-wide records exist on the device */
    int max_mtlid;           /* largest material id of the model (-1: only the default material) */
    int max_materials;       /* caps.max_materials: the default material's record */
    int fast_depth;
} MptKernelFacts;

typedef struct { int kernel, lds_bytes; } MptKernelChoice;   /* lds_bytes: of the chosen kernel (0: it takes no dynamic LDS) */

static inline MptKernelChoice mpt_choose_kernel(const MptKernelFacts *f) {
    MptKernelChoice ch = { MPT_KERNEL_GATHER, 0 };
    if (!f->fast) return ch;
    if (f->use_lds) {
        /* the 4-wide nodes with exact boxes in LDS: the headline kernel */
        if (f->lds_wide && f->use_wide && f->have_wnode)
            ch.lds_bytes = mpt_lds4_fit_bytes(f->nfaces, f->wide_nodes, f->wide_stack, f->max_mtlid + 1);
        if (ch.lds_bytes) { ch.kernel = MPT_KERNEL_LDS4; return ch; }
        /* ... or the binary nodes */
        ch.lds_bytes = mpt_lds_fit_bytes(f->nfaces, f->max_materials, f->fast_depth);
        if (ch.lds_bytes) { ch.kernel = MPT_KERNEL_LDS; return ch; }
    }
    /* scenes that do not fit LDS walk the 4-wide nodes (option "wide"; built by mpt_build_tree unless too deep)
     * A wide step costs ~2x the VALU instructions of a binary one (four slab tests and a sorting network) and makes
     * half the dependent fetches; with the planes picked by direction sign it wins on both big configurations
     * (MI355X: C4 963 -> 1135 Msamples/s, C5 494 -> 520), so it is the default wherever the collapse was built. */
    if (f->use_wide && f->wide_nodes > 0) ch.kernel = MPT_KERNEL_WIDE;
    return ch;
}

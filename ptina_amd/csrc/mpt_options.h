// mpt_options.h -- the settable options of a context, each stated once: its member of MptOptions with the default, and its row of
// MPT_OPTION_TABLE with the key, the accepted domain, how the value is stored, what a set does to the built tree and the words
// of the refusal.  mpt_set_option / mpt_get_option (miptina.cpp) are two calls into this table; include/miptina.h documents the
// same keys for callers.  Plain C++17 with nothing of HIP, so that tests/test_options_cpu.py holds it to a restatement on the CPU
// (as tests/test_lds_layout_cpu.py does lds_layout.h).
#pragma once

#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "mpt_types.h"    // MPT_MAX_BATCH (plain structures; wants size_t declared)

enum { MPT_MAX_PIPE = 6 };     // slots of the launch ring (mpt_ctx::ring): the most batches in flight

struct MptOptions {
    // ---- what a render launch reads
    int mode = 0;                // MPT_MODE_FAST (0) / MPT_MODE_STRICT (1) of include/miptina.h: which build of the kernels renders
    int batch = 32;              // most frames one launch renders
    int chunk = 0;               // frames per work item; 0 = auto
    int count = 0;               // 1: the kernels accumulate mpt_counters (slower)
    int lds = 1;                 // 1: the LDS-resident persistent kernel serves a scene that fits a CU's 160 KiB; 0: always gather from HBM / L2
    int lds_wide = 1;            // 1: scenes that fit LDS beside them walk the 4-wide nodes there (render_kernel_lds4), 0: the binary ones (render_kernel_lds)
    int lds_block = 0;           // lanes per persistent workgroup of the LDS kernels; 0 = auto (1024; 768 for a short launch of the binary one)
    int wide = 1;                // 1: walk the 4-wide nodes when the scene does not fit LDS (default), 0: the binary tree
    int wide_quant = 1;          // 1: the gather kernel reads the 4-wide nodes with child boxes quantised to 8 bits (qnode), 0: the exact ones (wnode)
    int shade_spec = 1;          // 1: a scene whose feature mask (shade_feat.h) is empty runs the plain instantiation of render_kernel_lds4; 0: always the generic one (A/B, tests)
    int skip_dark = -1;          // -1 auto (production build on, strict build off), 0 / 1 as set: do not trace shadow rays whose candidate direct light is exactly zero (production build: default;
                                 // the strict build traces them like the reference unless the option is set explicitly to 1 there)
    int tile_w_shift = 3, tile_h_shift = 3;   // work-item tile 2^w x 2^h pixels
    int pipe_depth = 0;          // batches in flight (slots of P / partial / queue heads); 0 = auto
    int grid_div = 0;            // each launch takes 1/grid_div of the CUs; 0 = auto
    int reserve_cus = 0;         // CUs no persistent workgroup claims (experiments: see mpt_flush); at most num_cus - 1, which only the context knows
    // tail finalisation (render_kernel.hip finalise_tiles): 1 = launches that find the ring idle sum, resolve and write out their
    // tiles themselves; 2 = the same without the early image (A/B); 0 = always the combine pass
    int finalise = 1;

    // ---- read-backs
    int zero_copy = 1;           // 1: a read-back into an mpt_host_alloc array is written there by the kernel over PCIe; 0: device buffer + DMA
    int spin_us = 20000;         // mpt_get_image polls a finalising launch for this long before it blocks
    int denoise_lds = 1;         // 1: mpt_get_denoised's strides 1 and 2 filter from a tile in LDS (same bits as the gathers)

    // ---- what mpt_build_tree reads (a set that can change the tree leaves it to be built again: MPT_TREE_* below)
    int tree = 1;                // fast build: 1 = SAH re-partition of the LBVH's leaves, 0 = the LBVH itself
    int gpu_build = 1;           // 1 = LBVH built on the device (lbvh_build.hip), 0 = host build
    int sah_build = -1;          // SAH re-partition: 1 on the device (sah_build.hip), 0 host pass, -1 auto
                                 // (device above 8192 faces; below, all of the host pass's splits are exact
                                 // sweeps and it costs a millisecond)
    int sah_max = 1 << 22;       // above this many faces the fast build walks the LBVH itself (the threaded host
                                 // SAH pass takes ~0.2 s at 1 M faces; it was 1.5 s on one core, hence 2^18 in round 1)
    int sah_exact_max = 8192;    // host SAH pass: ranges up to this size are swept exactly (diagnostics)
    int sah_inject_fail = 0;     // test door: treat the device SAH pass as failed after it ran
    int wide_build = 1;          // 1: the 4-wide collapse runs on the device (wide_build.hip), 0: host pass

    // ---- diagnostics
    int timeline = 0;            // 1: the LDS kernel records per-wave timestamps of its last launch
    int lane_hist = 0;           // counting kernels fill the lane histogram (mpt_get_lane_hist)
    int build_phases = 0;        // synchronise at the end of every phase of mpt_build_tree and time it
};

enum MptOptStore { MPT_STORE_VALUE, MPT_STORE_FLAG };             // as given | any non-zero value as 1
enum MptOptTree { MPT_TREE_KEEP, MPT_TREE_ON_CHANGE, MPT_TREE_ALWAYS };   // a set invalidates the tree: never | when the stored value changes | always

struct MptOptionRow {
    const char *key;
    int MptOptions::*member;
    int lo, hi;                  // accepted: lo <= value <= hi ...
    bool (*also)(int);           // ... and this, where the domain is not an interval (else null)
    MptOptStore store;
    MptOptTree tree;
    const char *domain;          // the refusal reads "<key> must be <domain>"; a %d in it stands for hi
};

#define MPT_ANY INT_MIN, INT_MAX, nullptr
inline constexpr MptOptionRow MPT_OPTION_TABLE[] = {
    { "mode",            &MptOptions::mode,            0, 1, nullptr,             MPT_STORE_VALUE, MPT_TREE_KEEP, "0 (fast) or 1 (strict)" },
    { "batch",           &MptOptions::batch,           1, MPT_MAX_BATCH, nullptr, MPT_STORE_VALUE, MPT_TREE_KEEP, "in 1..%d" },
    { "chunk",           &MptOptions::chunk,           0, INT_MAX, nullptr,       MPT_STORE_VALUE, MPT_TREE_KEEP, ">= 0" },
    { "count",           &MptOptions::count,           MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_KEEP, "" },
    { "lds",             &MptOptions::lds,             MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_KEEP, "" },
    { "lds_wide",        &MptOptions::lds_wide,        0, 1, nullptr,             MPT_STORE_VALUE, MPT_TREE_KEEP, "0 or 1" },
    { "lds_block",       &MptOptions::lds_block,       0, 1024, [](int v) { return v % 256 == 0; },
                                                                                  MPT_STORE_VALUE, MPT_TREE_KEEP, "0 (auto), 256, 512, 768 or 1024" },
    { "wide",            &MptOptions::wide,            MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_KEEP, "" },
    { "wide_quant",      &MptOptions::wide_quant,      MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_KEEP, "" },
    { "shade_spec",      &MptOptions::shade_spec,      0, 1, nullptr,             MPT_STORE_VALUE, MPT_TREE_KEEP,
      "0 (always the generic SHADE) or 1 (the plain one for plain scenes)" },
    { "skip_dark",       &MptOptions::skip_dark,       -1, 1, nullptr,            MPT_STORE_VALUE, MPT_TREE_KEEP, "-1 (auto), 0 or 1" },
    { "tile_w_shift",    &MptOptions::tile_w_shift,    0, 3, nullptr,             MPT_STORE_VALUE, MPT_TREE_KEEP, "in 0..3" },
    { "tile_h_shift",    &MptOptions::tile_h_shift,    0, 3, nullptr,             MPT_STORE_VALUE, MPT_TREE_KEEP, "in 0..3" },
    { "pipe_depth",      &MptOptions::pipe_depth,      0, MPT_MAX_PIPE, [](int v) { return v != 1; },
                                                                                  MPT_STORE_VALUE, MPT_TREE_KEEP, "0 (auto) or 2..%d" },
    { "grid_div",        &MptOptions::grid_div,        0, 8, nullptr,             MPT_STORE_VALUE, MPT_TREE_KEEP, "0 (auto) or 1..8" },
    { "reserve_cus",     &MptOptions::reserve_cus,     0, INT_MAX, nullptr,       MPT_STORE_VALUE, MPT_TREE_KEEP, "in 0..%d" },   // hi: mpt_set_option puts num_cus - 1
    { "finalise",        &MptOptions::finalise,        0, 2, nullptr,             MPT_STORE_VALUE, MPT_TREE_KEEP,
      "0 (combine pass), 1 (tail finalisation) or 2 (the same without the early image: A/B)" },
    { "zero_copy",       &MptOptions::zero_copy,       MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_KEEP, "" },
    { "spin_us",         &MptOptions::spin_us,         0, INT_MAX, nullptr,       MPT_STORE_VALUE, MPT_TREE_KEEP, ">= 0" },
    { "denoise_lds",     &MptOptions::denoise_lds,     MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_KEEP, "" },
    { "tree",            &MptOptions::tree,            0, 1, nullptr,             MPT_STORE_VALUE, MPT_TREE_ON_CHANGE, "0 (LBVH) or 1 (SAH)" },
    { "gpu_build",       &MptOptions::gpu_build,       MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_ON_CHANGE, "" },
    { "sah_build",       &MptOptions::sah_build,       -1, 1, nullptr,            MPT_STORE_VALUE, MPT_TREE_ON_CHANGE, "-1 (auto), 0 (host) or 1 (device)" },
    { "sah_max",         &MptOptions::sah_max,         MPT_ANY,                   MPT_STORE_VALUE, MPT_TREE_ALWAYS, "" },
    { "sah_exact_max",   &MptOptions::sah_exact_max,   2, INT_MAX, nullptr,       MPT_STORE_VALUE, MPT_TREE_ALWAYS, ">= 2" },
    { "sah_inject_fail", &MptOptions::sah_inject_fail, MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_ALWAYS, "" },
    { "wide_build",      &MptOptions::wide_build,      MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_ON_CHANGE, "" },
    { "timeline",        &MptOptions::timeline,        MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_KEEP, "" },
    { "lane_hist",       &MptOptions::lane_hist,       MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_KEEP, "" },
    { "build_phases",    &MptOptions::build_phases,    MPT_ANY,                   MPT_STORE_FLAG,  MPT_TREE_KEEP, "" },
};
#undef MPT_ANY
enum { MPT_OPTION_COUNT = sizeof MPT_OPTION_TABLE / sizeof MPT_OPTION_TABLE[0] };

inline const MptOptionRow *mpt_option_row(const char *key) {          // null: no settable option of that name
    for (const MptOptionRow &r : MPT_OPTION_TABLE)
        if (key && !strcmp(key, r.key)) return &r;
    return nullptr;
}

enum MptOptStatus { MPT_OPT_OK = 0, MPT_OPT_UNKNOWN, MPT_OPT_REFUSED };

// One set through a row.  Refused: `msg` says why and `o` is untouched.  Ok: *tree_invalid says whether the built tree is stale now.
inline MptOptStatus mpt_option_set_row(MptOptions &o, const MptOptionRow &r, int value, char *msg, size_t msg_size, bool *tree_invalid) {
    *tree_invalid = false;
    if (value < r.lo || value > r.hi || (r.also && !r.also(value))) {
        const char *d = strstr(r.domain, "%d");
        if (d) snprintf(msg, msg_size, "%s must be %.*s%d%s", r.key, (int)(d - r.domain), r.domain, r.hi, d + 2);
        else snprintf(msg, msg_size, "%s must be %s", r.key, r.domain);
        return MPT_OPT_REFUSED;
    }
    const int stored = r.store == MPT_STORE_FLAG ? (value ? 1 : 0) : value;
    *tree_invalid = r.tree == MPT_TREE_ALWAYS || (r.tree == MPT_TREE_ON_CHANGE && o.*r.member != stored);
    o.*r.member = stored;
    return MPT_OPT_OK;
}

inline MptOptStatus mpt_option_set(MptOptions &o, const char *key, int value, char *msg, size_t msg_size, bool *tree_invalid) {
    const MptOptionRow *r = mpt_option_row(key);
    if (r) return mpt_option_set_row(o, *r, value, msg, msg_size, tree_invalid);
    *tree_invalid = false;
    snprintf(msg, msg_size, "unknown option '%s'", key ? key : "");
    return MPT_OPT_UNKNOWN;
}

inline MptOptStatus mpt_option_get(const MptOptions &o, const char *key, int *value) {
    const MptOptionRow *r = mpt_option_row(key);
    if (!r) return MPT_OPT_UNKNOWN;
    *value = o.*r->member;
    return MPT_OPT_OK;
}

// miptina.cpp -- host runtime behind the C ABI of include/miptina.h.
//
// Owns the device state of one PTina "scene" (the singletons of ptina/things.py:20-28 collapsed
// into one context), uploads the scene, advances the Sobol sampler, batches enqueued frames into
// single launches.  The engines that launch at the call (preview, Metropolis, brute force, the list pass) are in engines.cpp, the
// film's read-backs in film_read.cpp, the measurement and test doors in measure.cpp, the BVH builders in tree_build.cpp, the RCCL
// film gather in comm.cpp.  No PyTorch, no Python: plain HIP runtime calls.

#include "miptina_ctx.h"

// Up to MPT_MAX_PIPE render streams, the main stream and the aux stream carry work at the same time.
// The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless told
// otherwise) and streams that share one are serialised, so ask for more before the runtime starts --
// eight of our own plus room for what RCCL creates -- unless the user has chosen a value.
// The runtime reads the variable when it initialises: this constructor runs at dlopen, which is early enough in
// every process that loads libmiptina before touching HIP (the Python package does).  Where HIP is already up --
// another HIP user in the process, or rocprofv3 --pmc, whose preloaded tool initialises the GPU first -- the
// request has no effect and streams fold onto 4 hardware queues: launches of a multi-GPU share then overlap
// less (G = 4 is slower than G = 1 there), results do not change.  Export GPU_MAX_HW_QUEUES
// yourself in such a process.
// Where the request comes too late it is SAID (stderr, once) and option "hw_queues" reads negative; bench.py hands
// the variable to its rocprofv3 passes itself, so that counters and timings come from the same queue configuration.
static int g_hwq = 0;            // GPU_MAX_HW_QUEUES after the constructor (0: unparsable)
static bool g_hwq_late = false;  // set here while a preloaded profiler tool may already have initialised HIP
__attribute__((constructor)) static void mpt_want_hw_queues() {
    if (!getenv("GPU_MAX_HW_QUEUES")) {
        setenv("GPU_MAX_HW_QUEUES", "12", 0);
        const char *pre = getenv("LD_PRELOAD");
        if ((pre && strstr(pre, "rocprof")) || getenv("ROCP_TOOL_LIBRARIES")) {
            g_hwq_late = true;
            fprintf(stderr, "libmiptina: GPU_MAX_HW_QUEUES=12 requested after a preloaded profiler tool may have initialised HIP: "
                            "streams may fold onto the default 4 hardware queues (results unchanged; export the variable "
                            "before starting the profiler)\n");
        }
    }
    const char *v = getenv("GPU_MAX_HW_QUEUES");
    g_hwq = v ? atoi(v) : 0;
}

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;

int fail(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

extern "C" const char *mpt_last_error(void) { return g_err.c_str(); }
extern "C" int mpt_version(void) { return 100; }

extern "C" int mpt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int use_ro(mpt_ctx *c) {   // entry of calls that only read results
    if (!c) return fail("null context");
    HIP_TRY(hipSetDevice(c->device));
    return 0;
}

int use(mpt_ctx *c) {      // entry of calls that may change what the next render launch reads
    if (use_ro(c)) return 1;
    // frames enqueued so far render with the state they were enqueued under
    if (mpt_flush(c)) return 1;
    // Marked AFTER that flush: the flush records ev_main and clears the mark, and what this call is
    // about to enqueue on the main stream (a Sobol reset, an upload, a film clear) must be behind the
    // ev_main the NEXT batch's aux / render streams wait for.
    c->main_dirty = true;
    c->spec.valid = false;     // whatever this call changes, the points computed ahead are not trusted across it
    return 0;
}


static void default_light(mpt_ctx *c) {
    // light/__init__.py:22-28: one POINT light at (1,2,3), radius 0.5, colour 32
    MptLight L{};
    L.color_size = { 32.f, 32.f, 32.f, 0.5f };
    L.pos_type = { 1.f, 2.f, 3.f, 0.f };
    int t = MPT_LIGHT_POINT;
    memcpy(&L.pos_type.w, &t, 4);
    c->h_lights.assign(1, L);
}

static int upload_lights(mpt_ctx *c) {
    if (!c->h_lights.empty())
        HIP_TRY(hipMemcpyAsync(c->lights, c->h_lights.data(), c->h_lights.size() * sizeof(MptLight),
                               hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// Wait for everything the context has in flight: the aux stream, the ring's streams (ring = false: nothing the caller is about to
// read was recorded on those, so the main stream alone) and the main stream.  mpt_destroy: a stream not made yet is skipped.
static int wait_all(mpt_ctx *c, bool ring = true) {
    if (ring && c->aux) HIP_TRY(hipStreamSynchronize(c->aux));
    for (auto &slot : c->ring)
        if (ring && slot.stream) HIP_TRY(hipStreamSynchronize(slot.stream));
    if (c->stream) HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" mpt_ctx *mpt_create(const mpt_caps *caps, int device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        fail("no HIP device available (%s): the MI355X path has no CPU fallback",
             e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return nullptr;
    }
    if (device < 0 || device >= ndev) { fail("device %d out of range (%d devices)", device, ndev); return nullptr; }
    mpt_ctx *c = new mpt_ctx();
    c->device = device;
    mpt_caps d = { 1 << 21, 1 << 22, 1 << 6, 1 << 6, 1 << 6, 1 << 21, 3 };
    c->caps = caps ? *caps : d;
    if (c->caps.max_lights > MPT_MAX_LIGHTS) c->caps.max_lights = MPT_MAX_LIGHTS;
    if (c->caps.max_filmpasses < 3) c->caps.max_filmpasses = 3;
    auto bail = [&](const char *what) -> mpt_ctx * {
        std::string m = g_err;
        mpt_destroy(c);              // what was allocated and created so far goes back
        fail("mpt_create: %s: %s", what, m.c_str());
        return nullptr;
    };
    if (hipSetDevice(device) != hipSuccess) return bail("hipSetDevice");
    if (c->stream.create()) return bail("stream");
    if (c->mats.reserve((size_t)c->caps.max_materials + 1)) return bail("materials");   // + the default material's record
    if (c->images.reserve(std::max<size_t>(c->caps.max_textures, 1))) return bail("images");
    if (c->lights.reserve(MPT_MAX_LIGHTS)) return bail("lights");
    if (c->d_counters.reserve(MPT_COUNTER_WORDS)) return bail("counters");
    if (c->d_scratch.reserve(2)) return bail("scratch");
    for (auto &slot : c->ring) {
        if (slot.ready.create() || slot.rendered.create() || slot.consumed.create()) return bail("event");
        if (slot.heads.reserve(MPT_QUEUE_WORDS)) return bail("work counters");
        hipMemsetAsync(slot.heads, 0, MPT_QUEUE_WORDS * sizeof(unsigned int), c->stream);
    }
    if (c->aux.create() || c->ev_main.create() || c->ev_film.create()) return bail("aux stream and events");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        if (prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
        c->clock_khz = prop.clockRate;
    }
    for (auto &slot : c->ring)       // (made after the aux stream, as ever: the runtime deals its hardware queues out in this order)
        if (slot.stream.create()) return bail("render streams");
    if (c->watchdog.create(1)) return bail("pinned watchdog flag");
    if (c->sah_mail.create(32)) return bail("pinned build mailbox");
    if (c->display.exposure.create(1)) return bail("pinned exposure word");
    *c->display.exposure.host = 1.0f;
    if (c->noise.stats.create(1)) return bail("pinned noise statistics");
    if (c->adapt.rec.create(1)) return bail("pinned selection record");
    if (c->compose.bounds.create(6)) return bail("pinned scene bounds");
    hipMemsetAsync(c->d_counters, 0, MPT_COUNTER_WORDS * sizeof(unsigned long long), c->stream);
    {   // unset materials: factor 0 (field-zero, mtllib.py:12-13), texture -1 (deviation Q6)
        std::vector<MptMaterial> z((size_t)c->caps.max_materials + 1);
        for (auto &m : z) { memset(&m, 0, sizeof m); for (int k = 0; k < 12; k++) m.tex[k] = -1; }
        // record max_materials: the default material of mtllib.py:82-93 (mtlid -1)
        const float dflt[14] = { 0.8f, 0.8f, 0.8f, 0.0f, 0.4f, 0.5f, 0.4f, 0.0f, 0.0f, 0.4f, 0.0f, 0.5f, 0.0f, 1.45f };
        memcpy(z.back().p, dflt, sizeof dflt);
        {   // its feature bits (none: no clearcoat, no transmission, no texture), from the same function as a loaded material's
            float fac[48] = {};
            fac[0] = dflt[0]; fac[1] = dflt[1]; fac[2] = dflt[2];
            for (int k = 1; k < 12; k++) fac[k * 4] = dflt[2 + k];
            c->default_feat = shade_feat_material(fac, nullptr);
            c->default_lean = shade_lean_material(fac, nullptr);
        }
        hipMemcpyAsync(c->mats, z.data(), z.size() * sizeof(MptMaterial), hipMemcpyHostToDevice, c->stream);
        mpt_launch_derive_materials(c->mats, (int)z.size(), c->stream);
        hipStreamSynchronize(c->stream);
    }
    for (int i = 0; i < 16; i++) c->v2w[i] = c->w2v[i] = (i % 5 == 0) ? 1.f : 0.f;
    default_light(c);
    if (upload_lights(c)) return bail("lights upload");
    // A/B timing of the lean SHADE variant (shade_feat.h): read here once, no option
    if (const char *v = getenv("MIPTINA_SHADE_LEAN")) c->lean_on = atoi(v) != 0;
    return c;
}

// Everything the streams still do for this context is waited for, the communicator goes while the main stream still exists, and
// `delete` gives everything else back: every buffer, stream and event is a member that owns it (miptina_ctx.h).  Also the way out
// of a failed mpt_create: what was not made yet is skipped.
extern "C" void mpt_destroy(mpt_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    (void)wait_all(c);
    if (c->stress_stream) hipStreamSynchronize(c->stress_stream);
    mpt_comm_release(c);
    delete c;
}

// ------------------------------------------------------------------ page-locked host buffers
// Read-backs into page-locked memory are one DMA (4 MiB film: ~80 us); into pageable memory the runtime
// stages them through its own bounce buffers at a fraction of that rate.  mpt_host_alloc hands out
// page-locked buffers (FilmTable.get_image builds its arrays on them); buffers of any other origin go
// through one page-locked staging buffer of the context and a memcpy.
static std::mutex g_host_mu;
static std::map<uintptr_t, size_t> g_host_bufs;   // base -> bytes

extern "C" void *mpt_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) {
        fail("hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_bufs[(uintptr_t)p] = bytes;
    return p;
}

extern "C" void mpt_host_free(void *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        g_host_bufs.erase((uintptr_t)p);
    }
    hipHostFree(p);
}

static bool is_locked_range(const void *p, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host_bufs.upper_bound((uintptr_t)p);
    if (it == g_host_bufs.begin()) return false;
    --it;
    return (uintptr_t)p + bytes <= it->first + it->second;
}

// the device alias of a caller array that is page-locked memory of ours, for kernels to write straight into (option "zero_copy"), or null
void *caller_alias(const mpt_ctx *c, void *p, size_t bytes) {
    void *mapped = nullptr;
    if (c->opt.zero_copy && is_locked_range(p, bytes) && hipHostGetDevicePointer(&mapped, p, 0) == hipSuccess) return mapped;
    return nullptr;
}

// device -> caller buffer on the main stream, blocking
int read_back(mpt_ctx *c, void *out, const void *dev, size_t bytes) {
    if (is_locked_range(out, bytes)) {
        HIP_TRY(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return 0;
    }
    if (c->h_stage.reserve(bytes, hipHostMallocDefault)) return 1;
    HIP_TRY(hipMemcpyAsync(c->h_stage, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(out, c->h_stage, bytes);
    return 0;
}

static int scene_feat_now(const mpt_ctx *c);

// ------------------------------------------------------------------ options
// The settable options are the rows of MPT_OPTION_TABLE (mpt_options.h); what follows adds what needs the context.
extern "C" int mpt_set_option(mpt_ctx *c, const char *key, int value) {
    if (use(c)) return 1;
    if (key && !strcmp(key, "launch_seq")) {
        // test door: the number of the next launch minus one (its slab tag is 2 + number mod 65534), so that a test can walk
        // the launches across the point where the tags come round and every slab is zeroed
        if (value < 0) return fail("launch_seq must be >= 0");
        if (mpt_flush(c)) return 1;
        c->launch_seq = (unsigned)value;
        // the slabs may hold entries with any tag of the old numbering: an epoch no launch number maps to makes the next
        // finalising launch zero them all (round-5 ADVICE: a jump inside an epoch, or to one whose tags overlap, met stale entries)
        c->tag_epoch = 0xffffffffu;
        return 0;
    }
    const MptOptionRow *row = mpt_option_row(key);
    if (!row) return fail("unknown option '%s'", key ? key : "");
    MptOptionRow r = *row;
    if (r.member == &MptOptions::reserve_cus) r.hi = c->num_cus - 1;     // the one bound that is no constant
    char why[160];
    bool tree_invalid = false;
    if (mpt_option_set_row(c->opt, r, value, why, sizeof why, &tree_invalid) != MPT_OPT_OK) return fail("%s", why);
    if (tree_invalid) { c->tree_valid = false; c->refit.lose(MPT_TOPO_OPTION); }
    return 0;
}

// What can be read and not set: results of the last build and the last launch, and facts of the device.
struct MptReadOnly { const char *key; int (*read)(const mpt_ctx *c); };
static const MptReadOnly g_read_only[] = {
    { "tree_depth", [](const mpt_ctx *c) { return c->tree_depth; } },
    { "fast_depth", [](const mpt_ctx *c) { return c->fast_depth; } },
    { "pending", [](const mpt_ctx *c) { return c->pending; } },
    { "last_finalised", [](const mpt_ctx *c) { return c->last_finalised; } },
    { "launch_seq", [](const mpt_ctx *c) { return (int)(c->launch_seq & 0x7fffffffu); } },
    { "tag_wraps", [](const mpt_ctx *c) { return (int)c->tag_wraps; } },
    { "scene_feat", [](const mpt_ctx *c) { return scene_feat_now(c); } },             // the scene's feature mask as loaded (shade_feat.h)
    { "shade_inst", [](const mpt_ctx *c) { return c->last_shade_feat; } },            // the mask the last render launch was compiled for (0 plain, 31 generic)
    { "cur_depth", [](const mpt_ctx *c) { return c->cur_depth; } },
    { "cur_div", [](const mpt_ctx *c) { return c->cur_div; } },
    { "last_div", [](const mpt_ctx *c) { return c->last_div; } },
    { "last_kernel", [](const mpt_ctx *c) { return c->last_kernel; } },
    { "num_cus", [](const mpt_ctx *c) { return c->num_cus; } },
    { "sah_fallback", [](const mpt_ctx *c) { return c->sah_fallback; } },
    { "sah_levels", [](const mpt_ctx *c) { return c->sah_stats.levels; } },
    { "sah_kelems", [](const mpt_ctx *c) { return (int)(c->sah_stats.elems / 1000); } },
    { "sah_chunks", [](const mpt_ctx *c) { return (int)c->sah_stats.chunks; } },
    { "sah_segments", [](const mpt_ctx *c) { return (int)c->sah_stats.segments; } },
    { "sah_part_kwords", [](const mpt_ctx *c) { return (int)(c->sah_stats.part_words / 1000); } },
    { "sah_tasks_small", [](const mpt_ctx *c) { return c->sah_stats.tasks_small; } },
    { "sah_tasks_big", [](const mpt_ctx *c) { return c->sah_stats.tasks_big; } },
    { "sah_t_sort_k", [](const mpt_ctx *c) { return c->sah_stats.t_sort_k; } },
    { "sah_t_loop_k", [](const mpt_ctx *c) { return c->sah_stats.t_loop_k; } },
    { "sah_t_max_k", [](const mpt_ctx *c) { return c->sah_stats.t_max_k; } },
    { "sah_task_levels", [](const mpt_ctx *c) { return c->sah_stats.task_levels; } },
    { "sah_task_levels_max", [](const mpt_ctx *c) { return c->sah_stats.task_levels_max; } },
    { "wide_nodes", [](const mpt_ctx *c) { return c->wide_nodes; } },
    { "wide_stack", [](const mpt_ctx *c) { return c->wide_stack; } },
    { "wide_ratio_permille", [](const mpt_ctx *c) { return (int)(c->wide_ratio * 1000.f + 0.5f); } },
    { "wide_depth", [](const mpt_ctx *c) { return c->wide_depth; } },
    { "nranks", [](const mpt_ctx *c) { return c->nranks; } },
    { "rank", [](const mpt_ctx *c) { return c->rank; } },
    { "device", [](const mpt_ctx *c) { return c->device; } },
    { "clock_khz", [](const mpt_ctx *c) { return c->clock_khz; } },
    { "hw_queues", [](const mpt_ctx *) { return g_hwq_late ? -g_hwq : g_hwq; } },
};

extern "C" int mpt_get_option(mpt_ctx *c, const char *key, int *value) {
    if (!c || !value) return fail("null argument");
    const char *k = key ? key : "";
    if (mpt_option_get(c->opt, k, value) == MPT_OPT_OK) return 0;
    for (const MptReadOnly &r : g_read_only)
        if (!strcmp(k, r.key)) { *value = r.read(c); return 0; }
    static const char stem[] = "build_phase_us_";                   // ... 0 to 5: the phases of the last mpt_build_tree
    const size_t n = sizeof stem - 1;
    if (!strncmp(k, stem, n) && k[n] >= '0' && k[n] <= '5' && !k[n + 1]) {
        *value = (int)(c->build_phase_us[k[n] - '0'] + 0.5);
        return 0;
    }
    return fail("unknown option '%s'", k);
}

// ------------------------------------------------------------------ film
extern "C" int mpt_set_size(mpt_ctx *c, int nx, int ny) {
    if (use(c)) return 1;
    if (nx <= 0 || ny <= 0) return fail("film size must be positive, got %dx%d", nx, ny);
    size_t npix = (size_t)nx * ny;
    if (npix > (size_t)c->caps.max_filmsize)
        return fail("film %dx%d exceeds max_filmsize=%d (init_things(max_filmsize=...))", nx, ny, c->caps.max_filmsize);
    if (npix > c->fb.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->history.gbuffer = c->history.motion = false;      // (the reprojection's buffers go with the film's)
        if (c->fb.reserve(npix, c->stream)) return 1;
    }
    // the reference keeps one flat buffer and only changes `res` (filmtable.py:41-42): stale sums
    // of another resolution are the caller's to clear(); same here.
    c->nx = nx; c->ny = ny; c->x0 = 0; c->x1 = nx; c->stripe_w = 0; c->stripe_idx = 0; c->stripe_mod = 1;
    c->film_version++;
    c->noise.marked = false;                     // a mark is a copy of the film as it was sized
    c->adapt.selected = false; c->adapt.count = 0;   // ... and a selection's indices mean pixels of that film
    return 0;
}

extern "C" int mpt_get_size(mpt_ctx *c, int *nx, int *ny) {
    if (!c) return fail("null context");
    if (nx) *nx = c->nx;
    if (ny) *ny = c->ny;
    return 0;
}

extern "C" int mpt_set_slab(mpt_ctx *c, int x0, int x1) {
    if (use(c)) return 1;
    if (x0 < 0 || x1 > c->nx || x0 > x1) return fail("slab [%d,%d) outside film width %d", x0, x1, c->nx);
    c->x0 = x0; c->x1 = x1;
    c->stripe_w = 0; c->stripe_idx = 0; c->stripe_mod = 1;
    return 0;
}

// The film dealt out in stripes of `width` columns: this context renders stripes index, index + modulo,
// ...  A contiguous slab per GPU leaves the GPUs unevenly loaded (the centre columns of a Cornell view
// cost 25 % more than the outer ones); interleaved stripes even that out.
extern "C" int mpt_set_stripes(mpt_ctx *c, int width, int index, int modulo) {
    if (use(c)) return 1;
    if (c->nx <= 0) return fail("film size not set: call set_size() first");
    if (width <= 0 || width % MPT_TILE != 0) return fail("stripe width must be a positive multiple of %d", MPT_TILE);
    if (modulo < 1 || index < 0 || index >= modulo) return fail("stripe index %d outside [0, %d)", index, modulo);
    if ((long long)width * modulo > (1 << 30)) return fail("stripe pitch too large");
    c->stripe_w = width; c->stripe_idx = index; c->stripe_mod = modulo;
    c->x0 = std::min((long long)index * width, (long long)c->nx); c->x1 = c->nx;
    return 0;
}

// columns of this context's share, and its tile columns for tiles `tile` pixels wide
static void share_extent(const mpt_ctx *c, int tile, long long *cols, int *tile_cols) {
    long long n = 0; int t = 0;
    if (c->stripe_w == 0) {
        n = c->x1 - c->x0; t = (c->x1 - c->x0 + tile - 1) / tile;
    } else {
        for (long long x = (long long)c->stripe_idx * c->stripe_w; x < c->nx; x += (long long)c->stripe_w * c->stripe_mod) {
            int w = (int)std::min<long long>(c->stripe_w, c->nx - x);
            n += w; t += (w + tile - 1) / tile;
        }
    }
    if (cols) *cols = n;
    if (tile_cols) *tile_cols = t;
}

// ------------------------------------------------------------------ scene upload
extern "C" int mpt_load_model(mpt_ctx *c, const float *verts, const int32_t *mtlids, int n) {
    if (use(c)) return 1;
    if (n < 0 || (n > 0 && !verts)) return fail("bad model arguments");
    if (n >= c->caps.max_faces) return fail("too many faces");                // model.py:84
    c->nfaces = n;
    c->verts.assign(verts, verts + (size_t)n * 24);
    if (mtlids) c->mtlids.assign(mtlids, mtlids + n);
    else c->mtlids.assign(n, -1);                                             // model.py:80-81
    c->max_mtlid = -1;
    for (int i = 0; i < n; i++) {
        if (c->mtlids[i] < -1 || c->mtlids[i] >= c->caps.max_materials)
            return fail("material id %d of face %d outside [-1, %d)", c->mtlids[i], i, c->caps.max_materials);
        c->max_mtlid = std::max(c->max_mtlid, (int)c->mtlids[i]);
    }
    {   // the bounding sphere of the model's box (MptRenderParams::t_scale)
        double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
        for (size_t v = 0; v < (size_t)n * 3; v++)
            for (int k = 0; k < 3; k++) {
                const double x = c->verts[v * 8 + k];
                if (x < lo[k]) lo[k] = x;
                if (x > hi[k]) hi[k] = x;
            }
        double r2 = 0;
        for (int k = 0; k < 3; k++) { c->scene_cen[k] = n ? 0.5 * (lo[k] + hi[k]) : 0.0; r2 += n ? 0.25 * (hi[k] - lo[k]) * (hi[k] - lo[k]) : 0.0; }
        c->scene_rad = std::sqrt(r2);
        if (!std::isfinite(c->scene_rad)) c->scene_rad = 1e30;
    }
    c->tree_valid = false;
    c->d_model_stale = true;
    c->h_model_stale = false;                    // the device model belongs to the host copy again ...
    c->compose.out_valid = false;                // ... so the next mpt_compose writes all of it
    return 0;
}

// The feature mask of the scene as it stands (shade_feat.h): the materials the model uses -- the records the LDS-resident kernel
// packs, 0 .. max_mtlid and the default one -- the light list and the world light.  Formed where it is used (a launch, the
// "scene_feat" option), so it follows every reload of materials, model, lights or world without a cache to invalidate.
static int scene_feat_now(const mpt_ctx *c) {
    return shade_feat_scene(c->mat_feat.data(), (int)c->mat_feat.size(), c->max_mtlid, c->default_feat, (int)c->h_lights.size(), c->world_tex);
}
// ... and whether the same materials leave sheen and subsurface at zero (shade_lean_scene), formed where it is used as well
static int scene_lean_now(const mpt_ctx *c) {
    return shade_lean_scene(c->mat_lean.data(), (int)c->mat_lean.size(), c->max_mtlid, c->default_lean);
}

// Which SHADE the last render launch ran: *feat as option "shade_inst" reports it, *lean = 1 for the lean variant of the plain
// instantiation, 0 for any other kernel; both -1 before the first launch
extern "C" int mpt_get_shade_variant(mpt_ctx *c, int *feat, int *lean) {
    if (!c || !feat || !lean) return fail("null argument");
    *feat = c->last_shade_feat;
    *lean = c->last_shade_lean;
    return 0;
}

extern "C" int mpt_load_materials(mpt_ctx *c, const float *fac, const int32_t *tex, int m) {
    if (use(c)) return 1;
    if (m < 0 || m > c->caps.max_materials) return fail("%d materials exceed max_materials=%d", m, c->caps.max_materials);
    std::vector<MptMaterial> h(std::max(m, 1));
    std::vector<unsigned char> feat((size_t)m), lean((size_t)m);
    int max_tex = -1;
    for (int i = 0; i < m; i++) {
        MptMaterial &M = h[i];
        memset(&M, 0, sizeof M);
        const float *f = fac + (size_t)i * 48;
        M.p[0] = f[0]; M.p[1] = f[1]; M.p[2] = f[2];                          // basecolor .xyz, mtllib.py:82
        for (int k = 1; k < 12; k++) M.p[2 + k] = f[k * 4];                   // scalars take .x, mtllib.py:83-93
        M.any_tex = 0;
        for (int k = 0; k < 12; k++) {
            int t = tex ? tex[(size_t)i * 12 + k] : -1;
            if (t < -1 || t >= c->caps.max_textures) return fail("texture id %d outside [-1, %d)", t, c->caps.max_textures);
            M.tex[k] = t;
            if (t != -1) M.any_tex = 1;
            max_tex = std::max(max_tex, t);
        }
        feat[i] = (unsigned char)shade_feat_material(f, M.tex);
        lean[i] = (unsigned char)shade_lean_material(f, M.tex);
    }
    c->max_mat_tex = max_tex;
    // records beyond m keep what an earlier call left in them on the device, so their bits are kept as well
    // (the scene's mask is formed from these at every launch: scene_feat_now)
    if (c->mat_feat.size() < feat.size()) c->mat_feat.resize(feat.size(), 0);
    std::copy(feat.begin(), feat.end(), c->mat_feat.begin());
    if (c->mat_lean.size() < lean.size()) c->mat_lean.resize(lean.size(), 1);      // (a record never loaded is all-zero: lean)
    std::copy(lean.begin(), lean.end(), c->mat_lean.begin());
    c->nmats = m;
    if (m) HIP_TRY(hipMemcpyAsync(c->mats, h.data(), (size_t)m * sizeof(MptMaterial), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(mpt_launch_derive_materials(c->mats, m, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mpt_reset_images(mpt_ctx *c) {                                  // image.py:90-92
    if (use(c)) return 1;
    c->h_images.clear();
    c->texels_used = 0;
    c->image_gen++;
    return 0;
}

extern "C" int mpt_load_image(mpt_ctx *c, const float *rgba, int nx, int ny, int *id) {   // image.py:51-88
    if (use(c)) return 1;
    if ((int)c->h_images.size() >= c->caps.max_textures) return fail("Out of ID!");       // allocator.py:53
    size_t need = (size_t)nx * ny;
    if (c->texels_used + need > (size_t)c->caps.max_texels) return fail("Out of memory!"); // allocator.py:24
    if (!c->texels && c->texels.reserve(std::max<size_t>(c->caps.max_texels, 1))) return 1;
    HIP_TRY(hipMemcpyAsync(c->texels + c->texels_used, rgba, need * sizeof(MptVec4), hipMemcpyHostToDevice, c->stream));
    MptImage im = { nx, ny, (int32_t)c->texels_used, 0 };
    c->h_images.push_back(im);
    c->texels_used += need;
    c->image_gen++;
    HIP_TRY(hipMemcpyAsync(c->images, c->h_images.data(), c->h_images.size() * sizeof(MptImage),
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (id) *id = (int)c->h_images.size() - 1;
    return 0;
}

extern "C" int mpt_set_camera(mpt_ctx *c, const float v2w[16], const float w2v[16]) {
    if (use(c)) return 1;
    memcpy(c->v2w, v2w, sizeof c->v2w);
    if (w2v) memcpy(c->w2v, w2v, sizeof c->w2v);
    return 0;
}

extern "C" int mpt_clear_lights(mpt_ctx *c) {
    if (use(c)) return 1;
    c->h_lights.clear();
    return 0;
}

extern "C" int mpt_add_light(mpt_ctx *c, int type, const float color[3], const float pos[3], const float axes[9],
                             float size, int *index) {
    if (use(c)) return 1;
    if (type != MPT_LIGHT_POINT && type != MPT_LIGHT_AREA) return fail("unknown light type %d", type);
    if ((int)c->h_lights.size() >= c->caps.max_lights) return fail("too many lights (max_lights=%d)", c->caps.max_lights);
    MptLight L{};
    L.color_size = { color[0], color[1], color[2], size };
    L.pos_type = { pos[0], pos[1], pos[2], 0.f };
    memcpy(&L.pos_type.w, &type, 4);
    L.ax0 = { axes[0], axes[1], axes[2], 0.f };
    L.ax1 = { axes[3], axes[4], axes[5], 0.f };
    L.ax2 = { axes[6], axes[7], axes[8], 0.f };
    c->h_lights.push_back(L);
    if (index) *index = (int)c->h_lights.size() - 1;
    return upload_lights(c);
}

extern "C" int mpt_set_world_light(mpt_ctx *c, const float fac[4], int tex) {
    if (use(c)) return 1;
    memcpy(c->world_fac, fac, sizeof c->world_fac);
    c->world_tex = tex;
    return 0;
}

// ------------------------------------------------------------------ sobol
extern "C" int mpt_sobol_init(mpt_ctx *c, const int32_t *V, int rows, int dim) {
    if (use(c)) return 1;
    if (rows < 2 || dim < 1 || !V) return fail("bad sobol grid %dx%d", rows, dim);
    if (wait_all(c)) return 1;
    c->sV.release(); c->sX.release(); c->spec.X.release(); c->sP.release();
    for (auto &slot : c->ring) slot.points.release();
    if (c->sV.reserve((size_t)rows * dim) || c->sX.reserve((size_t)dim) || c->spec.X.reserve((size_t)dim) ||
        c->sP.reserve((size_t)MPT_MAX_BATCH * dim)) return 1;
    for (auto &slot : c->ring)
        if (slot.points.reserve((size_t)MPT_MAX_BATCH * dim)) return 1;
    HIP_TRY(hipMemcpyAsync(c->sV, V, (size_t)rows * dim * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->sX, 0, (size_t)dim * sizeof(int), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->sdim = dim; c->srows = rows; c->stime = 0;
    return 0;
}

int sobol_advance(mpt_ctx *c, int count, int keep, hipStream_t stream, float *P) {
    // keep = number of trailing frames whose points are written to P[0..keep)
    if (!stream) stream = c->stream;
    if (!P) P = c->sP;
    while (count > 0) {
        int step = count;
        int k = std::min(keep, step);
        HIP_TRY(mpt_launch_sobol_update(c->sX, c->sX, c->sV, P, c->sdim, c->srows, c->stime, step, k, 1, stream));
        c->stime = (int32_t)((uint32_t)c->stime + (uint32_t)step);
        count -= step;
    }
    return 0;
}

extern "C" int mpt_sobol_reset(mpt_ctx *c, int skip) {                         // sobol.py:92-97
    if (use(c)) return 1;
    if (!c->sV) return fail("sobol sampler not initialised");
    c->stime = 0;
    HIP_TRY(hipMemsetAsync(c->sX, 0, (size_t)c->sdim * sizeof(int), c->stream));
    return sobol_advance(c, skip, 0);
}

extern "C" int mpt_sobol_update(mpt_ctx *c, int count) {                       // sobol.py:99-105
    if (use(c)) return 1;
    if (!c->sV) return fail("sobol sampler not initialised");
    return sobol_advance(c, count, 0);
}

extern "C" int mpt_sobol_get(mpt_ctx *c, int32_t *X, float *P, int32_t *time) {
    if (use(c)) return 1;
    if (!c->sV) return fail("sobol sampler not initialised");
    std::vector<int32_t> x(c->sdim);
    HIP_TRY(hipMemcpyAsync(x.data(), c->sX, (size_t)c->sdim * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (X) memcpy(X, x.data(), (size_t)c->sdim * sizeof(int32_t));
    if (P)
        for (int j = 0; j < c->sdim; j++) {                                    // construct_float, sobol.py:20-29
            float ret = 0.f, term = 0.5f;
            for (uint32_t v = (uint32_t)x[j]; v; v <<= 1, term *= 0.5f)
                if (v & 0x80000000u) ret += term;
            P[j] = ret;
        }
    if (time) *time = c->stime;
    return 0;
}

// ------------------------------------------------------------------ rendering
// the part of the launch parameters that describes the scene's lights, world light, camera, materials and images: what lights_hit,
// lights_sample, image_sample, world_at, material_get and camera_generate read (fill_params; measure.cpp's test door of the device functions, which needs no film,
// sampler or tree)
int fill_scene_params(mpt_ctx *c, MptRenderParams &p) {
    p.nlights = (int)c->h_lights.size(); p.world_tex = c->world_tex;
    memcpy(p.world_fac, c->world_fac, sizeof p.world_fac);
    memcpy(p.v2w, c->v2w, sizeof p.v2w);
    p.default_mtl = c->caps.max_materials;
    p.mats = c->mats; p.lights = c->lights; p.images = c->images; p.texels = c->texels;
    if (p.world_tex != -1 && (p.world_tex < 0 || p.world_tex >= (int)c->h_images.size()))
        return fail("world light texture %d is not a loaded image", p.world_tex);
    return 0;
}

// "not set up yet": fails at the call, not at the deferred launch
static int check_ready(const mpt_ctx *c) {
    if (c->nx <= 0) return fail("film size not set: call set_size() first");
    if (!c->sV) return fail("sobol sampler not initialised");
    if (!c->tree_valid) return fail("BVH not built: call build_tree() after load_model()");
    return 0;
}

// entry of the calls that render frames of the film (mpt_render; engines.cpp)
int render_entry(mpt_ctx *c, int nframes) {
    if (!c) return fail("null context");
    if (nframes < 0) return fail("nframes must be >= 0");
    return check_ready(c);
}

// t_scale: 2^-e with 2^e no less than the farthest a ray origin -- a point of the camera's near plane or of a surface, or one of the n
// origins o [n][3] a caller brings (mpt_walk_trace: the finite ones) -- can be from any point of the scene's bounding sphere (mpt_load_model)
void fill_t_scale(const mpt_ctx *c, MptRenderParams &p, const float *o, int n) {
    double reach = c->nfaces > 0 ? 2.0 * c->scene_rad : 1.0;
    for (int corner = 0; corner < 4 && c->nfaces > 0; corner++) {
        const double x = (corner & 1) ? 1.0 : -1.0, y = (corner & 2) ? 1.0 : -1.0;
        const float *M = c->v2w;
        const double a3 = M[12] * x + M[13] * y - M[14] + M[15];
        double d2 = 0;
        for (int k = 0; k < 3; k++) {
            const double o = (M[4 * k] * x + M[4 * k + 1] * y - M[4 * k + 2] + M[4 * k + 3]) / a3;
            d2 += (o - c->scene_cen[k]) * (o - c->scene_cen[k]);
        }
        if (std::isfinite(d2)) reach = std::max(reach, std::sqrt(d2) + c->scene_rad);
    }
    for (int r = 0; r < n && c->nfaces > 0; r++) {
        double d2 = 0;
        for (int k = 0; k < 3; k++) d2 += ((double)o[3 * (size_t)r + k] - c->scene_cen[k]) * ((double)o[3 * (size_t)r + k] - c->scene_cen[k]);
        if (std::isfinite(d2)) reach = std::max(reach, std::sqrt(d2) + c->scene_rad);
    }
    int e = 0;
    std::frexp(std::min(std::max(reach * 1.001, 1e-30), 1e30), &e);       // reach * 1.001 <= 2^e
    p.t_scale = (float)std::ldexp(1.0, -e);
    p.t_unscale = (float)std::ldexp(1.0, e);
}

int fill_params(mpt_ctx *c, MptRenderParams &p, int nframes) {
    if (check_ready(c)) return 1;
    // the production kernels address a frame's Sobol row and a triangle's shading record by 32-bit offsets from a scalar base, and
    // multiply frame x dimension in 24 bits (lane_draws, shade_rec_load)
    if ((long long)nframes * c->sdim >= (1ll << 30) || nframes >= (1 << 24) || c->sdim >= (1 << 24))
        return fail("%d frames of %d Sobol dimensions in one launch exceed the kernels' 32-bit row offsets", nframes, c->sdim);
    if (c->nfaces >= (1 << 26)) return fail("%d faces exceed the kernels' 32-bit record offsets", c->nfaces);
    memset(&p, 0, sizeof p);
    p.nx = c->nx; p.ny = c->ny; p.x0 = c->x0; p.x1 = c->x1;
    p.nframes = nframes; p.n = c->nfaces;
    p.sobol_inv_dim = 1.0f / (float)c->sdim;
    p.sobol_dim = c->sdim;
    share_extent(c, MPT_TILE, nullptr, &p.tiles_x);
    p.stripe_w = c->stripe_w ? c->stripe_w : (1 << 30);
    p.stripe_pitch = c->stripe_w ? c->stripe_w * c->stripe_mod : (1 << 30);
    p.tiles_y = (c->ny + MPT_TILE - 1) / MPT_TILE;
    p.ntiles = p.tiles_x * p.tiles_y;
    fill_t_scale(c, p, nullptr, 0);
    p.wnode = c->wnode; p.qnode = c->qnode; p.nwide = c->wide_nodes; p.stack_spill = nullptr;
    p.snode = c->nodes.snode; p.fnode = c->nodes.fnode; p.tgeo = c->tris.tgeo; p.tshade = c->tris.tshade; p.tfast = c->tfast;
    p.skip_dark = c->opt.skip_dark >= 0 ? c->opt.skip_dark : (c->opt.mode == MPT_MODE_FAST ? 1 : 0);
    p.P = c->sP;
    p.film0 = c->fb.film[0]; p.film1 = c->fb.film[1]; p.film2 = c->fb.film[2];
    p.counters = c->d_counters;
    p.lane_hist = c->opt.lane_hist;
    p.watchdog = c->watchdog.dev;
    return fill_scene_params(c, p);
}

// ------------------------------------------------------------------ mpt_flush, step by step
// where a batch runs: its slot of the ring, the stream of its render kernel and the stream its points are prepared on
struct BatchSlot {
    bool fast;         // fast build: this batch runs on its own stream; strict build: everything stays on the main stream
    int k;
    hipStream_t rs;    // the render
    hipStream_t ss;    // fast build: the Sobol points and the zeroed queue heads of this batch are prepared on the aux
                       // stream (never behind a render kernel), the render itself goes to the slot's own
};

// step 1 (fast build): how many launches share the chip and how many ring slots they rotate through
static int ring_policy(mpt_ctx *c, int B) {
    // A launch ends with a drain of about one path latency (~0.4 ms on MI355X for depth-5 paths)
    // in which its lanes run empty one by one; a persistent workgroup leaves only when its
    // slowest lane has.  A launch that owns every CU pays that on every CU.  Small launches
    // therefore take 1/G of the CUs each and G of them are resident at once, in different
    // phases: the drain then idles 1/G of the chip.  (Measured, 1/8 film slab of 512x512x32:
    // 1.03 ms per step with G=1, 0.78 with G=2, 0.73 with G=4; whole film: 4.69 / 4.62 / 4.84.)
    long long cols = 0;
    share_extent(c, 1, &cols, nullptr);
    const double per_lane = (double)B * cols * c->ny / ((double)c->num_cus * 1024.0);
    int div = c->opt.grid_div > 0 ? c->opt.grid_div : (per_lane >= 24.0 ? 1 : per_lane >= 6.0 ? 2 : 4);
    int depth = c->opt.pipe_depth > 0 ? c->opt.pipe_depth : (div == 1 ? 2 : std::min(div + 2, (int)MPT_MAX_PIPE));
    if (depth != c->cur_depth) {
        // slots are reused round-robin: let everything in flight finish before the ring changes size
        if (wait_all(c)) return 1;
        c->flip = 0;
    }
    c->cur_depth = depth; c->cur_div = div;
    return 0;
}

// step 2: the batch's Sobol points (p.P) and, if they were made ahead of time, its zeroed queue heads (*use_spec).  A batch
// without tiles (p.ntiles == 0: an empty share) only moves the sampler.
static int batch_points(mpt_ctx *c, MptRenderParams &p, const BatchSlot &s, int B, bool *use_spec) {
    MptRingSlot &slot = c->ring[s.k];
    if (s.fast) {
        if (c->main_dirty) {       // uploads / resets / option changes enqueued on the main stream come first
            HIP_TRY(hipEventRecord(c->ev_main, c->stream));
            c->main_dirty = false;
        }
        HIP_TRY(hipStreamWaitEvent(s.ss, c->ev_main, 0));
        HIP_TRY(hipStreamWaitEvent(s.ss, slot.rendered, 0));   // the batch that last read the slot's points and queue heads
        HIP_TRY(hipStreamWaitEvent(s.rs, c->ev_main, 0));
        p.P = slot.points;
    }
    // the points (and zeroed queue heads) of this batch may have been prepared when the previous one was launched
    *use_spec = s.fast && p.ntiles != 0 && c->spec.valid && c->spec.slot == s.k && c->spec.B == B && c->spec.time == c->stime;
    c->spec.valid = false;
    if (p.ntiles == 0) {
        if (sobol_advance(c, B, 0, s.ss, s.fast ? slot.points.p : nullptr)) return 1;
        if (s.fast) { HIP_TRY(hipEventRecord(slot.ready, s.ss)); HIP_TRY(hipStreamWaitEvent(c->stream, slot.ready, 0)); }
        return 0;
    }
    if (*use_spec) {
        // the points AND the state this batch leaves behind were computed when the previous batch was launched: the sampler moves by
        // a swap of two pointers -- no kernel at launch time (round 3 ran an X-only update here, whose 83 small workgroups took
        // CUs just when the persistent render workgroups wanted them: half the workgroups of a 1/8-share launch started 35 us late)
        c->sX.swap(c->spec.X);
        c->stime = (int32_t)((uint32_t)c->stime + (uint32_t)B);
    } else if (sobol_advance(c, B, B, s.ss, s.fast ? slot.points.p : nullptr)) return 1;
    return 0;
}

// step 3a: which kernel serves the scene, and the dynamic LDS it asks for (lds_layout.h: the layout, the fit rule and the choice)
static MptKernelChoice choose_kernel(const mpt_ctx *c) {
    MptKernelFacts f;
    f.fast = c->opt.mode == MPT_MODE_FAST;
    f.use_lds = c->opt.lds; f.lds_wide = c->opt.lds_wide; f.use_wide = c->opt.wide;
    f.nfaces = c->nfaces;
    f.wide_nodes = c->wide_nodes; f.wide_stack = c->wide_stack; f.have_wnode = c->wnode != nullptr;
    f.max_mtlid = c->max_mtlid; f.max_materials = c->caps.max_materials;
    f.fast_depth = c->fast_depth;
    return mpt_choose_kernel(&f);
}

// step 3b: the work items of the launch -- (tile, chunk of frames) -- into p; returns the columns of this context's share, padded
// to whole work-item tiles
static int work_items(const mpt_ctx *c, MptRenderParams &p, int B, bool fast) {
    int chunk = B, nchunks = 1;
    const int tw = 1 << c->opt.tile_w_shift, th = 1 << c->opt.tile_h_shift;
    int tile_cols = 0;
    share_extent(c, tw, nullptr, &tile_cols);
    const int tiles8 = tile_cols * ((c->ny + th - 1) / th);
    if (fast) {
        chunk = c->opt.chunk;
        if (chunk <= 0) {
            // Work items are (8x8 tile, chunk of frames).  Persistent waves refill from the queue the moment their
            // pool drains, so small items cost one returning atomic each and nothing else, and the launch ends
            // with what the last items hold: one frame of a tile (64 samples = one generation of paths per wave)
            // measured best on MI355X -- 512x512x32: 4.56 ms per launch against 4.67 (2 frames) and 5.07 (4);
            // 32-sample items (8x4 tiles) lose again (4.70) because a wave then starts half empty.
            chunk = 1;
        }
        chunk = std::min(chunk, B);
        nchunks = (B + chunk - 1) / chunk;
    }
    p.chunk = chunk; p.nchunks = nchunks;
    p.nitems = tiles8 * nchunks;
    p.tile_w_shift = c->opt.tile_w_shift; p.tile_h_shift = c->opt.tile_h_shift;
    return tile_cols * tw;
}

// Grow a per-slot buffer of the ring to `need` elements -- every slot of the ring at once: an allocation synchronises the
// device, so it must not happen again on the second, third, ... batch of a run.  zero: fresh memory is zeroed on the main
// stream; *grown: a slot was replaced.
template <class T>
static int grow_ring(mpt_ctx *c, DevBuf<T> MptRingSlot::*member, size_t need, bool zero, bool *grown) {
    for (int q = 0; q < c->cur_depth; q++)
        if (DevBuf<T> &buf = c->ring[q].*member; need > buf.cap) {
            HIP_TRY(hipDeviceSynchronize());
            if (buf.reserve(need, grown)) return 1;
            if (zero) HIP_TRY(hipMemsetAsync(buf, 0, need * sizeof(T), c->stream));
        }
    return 0;
}

// step 4 (fast build): the sample slab of the ring's slots, this batch's queue heads, and what its render stream waits for
static int slab_and_queue_heads(mpt_ctx *c, MptRenderParams &p, const BatchSlot &s, int B, int ccols, bool use_spec) {
    MptRingSlot &slot = c->ring[s.k];
    // one float4 per sample: [frame][pixel]; the combine pass sums frames in order
    // ... of this context's share only: its columns packed side by side, padded to whole work-item tiles
    p.partial_stride = ccols * c->ny;
    const size_t need = (size_t)B * (size_t)ccols * c->ny;
    // the w of a slab entry is its ready flag for the tail finalisation (the launch's tag): fresh memory must not
    // hold one by accident -- and it does: the allocator hands back the slab of an earlier context, whose first
    // finalising launch used the very tag this context's first one will use
    bool zeroed = false;
    if (grow_ring(c, &MptRingSlot::slab, need, true, &zeroed)) return 1;
    // ... and the zeros must be there before any launch of the ring writes or reads the slab: the render streams are not
    // ordered behind the stream that zeroes, and a memset may return before it is done.  (Seen in the full GPU test run as a
    // 2048 x 2048 film with single samples of an earlier test's render in it: its 2 GiB slabs take a millisecond to zero.)
    if (zeroed) HIP_TRY(hipStreamSynchronize(c->stream));
    p.partial = slot.slab;
    p.work_counter = slot.heads;
    if (!use_spec) {
        HIP_TRY(hipMemsetAsync(slot.heads, 0, MPT_QUEUE_WORDS * sizeof(unsigned int), s.ss));   // 8 queue heads + the finalisation's tile counter
        HIP_TRY(hipEventRecord(slot.ready, s.ss));
    }
    HIP_TRY(hipStreamWaitEvent(s.rs, slot.ready, 0));
    HIP_TRY(hipStreamWaitEvent(s.rs, slot.consumed, 0));   // combine of the batch that last used this slab
    return 0;
}

// step 5: is the ring idle, and how many CUs does this launch take (c->last_div: the share)
static int launch_share(mpt_ctx *c, bool fast, bool *ring_idle, int *launch_cus) {
    // Persistent workgroups hold their CUs for a whole launch, and the launches of the ring keep every CU taken
    // all the time: a foreign kernel -- RCCL's send/recv kernel of the film gather -- waits for a launch to end
    // (measured with mpt_probe_kernel on MI355X: median 0.13-0.47 ms, up to 2.2 ms beside a 1/8 share's launches,
    // 4.2 ms beside whole-film launches, against 12 us on an idle GPU).  Leaving CUs out of every launch does NOT
    // change that while launches overlap -- the workgroups of the next launch in the ring take any free CU at
    // once (same waits measured with 2 CUs left out) -- so "reserve_cus" defaults to 0 and the gather of batch i
    // simply completes one launch late; nothing waits for it but the read-back, and a step that ends with a
    // read-back (bench.py's `value`) has no other launch in flight when its gather starts.
    const int reserve = std::max(c->opt.reserve_cus, 0);
    const int usable_cus = std::max(c->num_cus - reserve, 1);
    // A launch that finds the ring idle has no other launch to share the chip with -- a step that ends with a
    // read-back (bench.py's `value`, an interactive frame) is one launch at a time -- so it takes every CU; 1/G of
    // them would only make it G times longer.  Launches issued while others are still in flight take 1/G each.
    int launch_div = std::max(c->cur_div, 1);
    *ring_idle = fast;
    if (fast && ((launch_div > 1 && c->opt.grid_div <= 0) || c->opt.finalise)) {
        for (int q = 0; q < c->cur_depth && *ring_idle; q++) {
            hipError_t st = hipEventQuery(c->ring[q].rendered);
            if (st == hipErrorNotReady) *ring_idle = false;
            else if (st != hipSuccess) HIP_TRY(st);
        }
    }
    if (fast && launch_div > 1 && c->opt.grid_div <= 0 && *ring_idle) launch_div = 1;
    c->last_div = launch_div;
    *launch_cus = std::max(usable_cus / launch_div, 1);   // G launches never claim more than usable_cus
    return 0;
}

// step 6: what depends on launch_cus -- the spill strips of the 4-wide gather kernel (*wide_blocks: its workgroups), the lanes
// per workgroup of the LDS-resident kernels (*lds_block), the timeline buffer
static int size_launch_buffers(mpt_ctx *c, MptRenderParams &p, int k, int kernel, int launch_cus, int *wide_blocks, int *lds_block) {
    *wide_blocks = 0;
    if (kernel == MPT_KERNEL_WIDE) {
        HIP_TRY(mpt_wide_blocks(launch_cus, c->opt.count, c->opt.wide_quant, wide_blocks));
        const size_t need_spill = (size_t)*wide_blocks * MPT_BLOCK * 128;   // >= SpillStack::SPILL entries per lane (128 - LDS levels)
        // one strip PER SLOT: the launches of different slots overlap, and a strip is indexed by block and lane only
        bool grown = false;
        if (grow_ring(c, &MptRingSlot::spill, need_spill, false, &grown)) return 1;
        p.stack_spill = c->ring[k].spill;
    }
    const bool lds_kernel = kernel == MPT_KERNEL_LDS || kernel == MPT_KERNEL_LDS4;
    // Lanes per persistent workgroup of the LDS-resident kernel.  A launch that gives a lane fewer than six samples (an eighth
    // of the benchmark film: four) is over before a steady state forms: its length is a few path latencies, and a path is
    // faster with three waves per SIMD than with four (MI355X, 1/8 share: 0.78 ms at 768 lanes against 0.84 at 1024; from a
    // quarter share upwards 1024 is as good or better).  Same film either way.
    // (The kernel over the 4-wide nodes is fastest with 1024 lanes at every size: solo launch of a 1/8 share 0.49 ms against 0.53
    // at 768, 0.64 at 512; whole film 2.59 / 2.97 / 3.94.)
    *lds_block = c->opt.lds_block ? c->opt.lds_block : 1024;
    if (kernel == MPT_KERNEL_LDS && c->opt.lds_block == 0 &&
        ((long long)p.nitems * p.chunk << (c->opt.tile_w_shift + c->opt.tile_h_shift)) < 6ll * launch_cus * 1024) *lds_block = 768;
    p.timeline = nullptr;
    if (c->opt.timeline && lds_kernel) {
        const int waves = launch_cus * (*lds_block / 64);
        if (waves != c->timeline_waves) {
            HIP_TRY(hipDeviceSynchronize());
            c->d_timeline.release();
            if (c->d_timeline.reserve((size_t)waves * MPT_TIMELINE_WORDS)) return 1;
            HIP_TRY(hipMemsetAsync(c->d_timeline, 0, (size_t)waves * MPT_TIMELINE_WORDS * sizeof(unsigned long long), c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->timeline_waves = waves;
        }
        p.timeline = c->d_timeline;
    }
    return 0;
}

// step 7: number the launch and, if it finalises its tiles itself (fin), give it its slab tag, order it behind the main stream's
// work on the film and tell it where the early image goes
// Tail finalisation: a launch that has the chip to itself -- a step that ends with a read-back, an interactive frame -- adds
// its frames to the film, resolves and writes the image out by itself, in the shadow of its own drain (finalise_tiles).  A
// launch issued while another is in flight keeps the combine pass on the main stream: two launches must not add to the same
// film pixels at the same time, and the main stream is what orders them.
static int setup_finalisation(mpt_ctx *c, MptRenderParams &p, const BatchSlot &s, bool fin) {
    c->launch_seq++;
    p.fin_counter = nullptr; p.image_out = nullptr; p.slab_tag = MPT_TAG_COMBINE;
    c->film_version++;                           // this batch changes pass 0, whoever adds it
    c->last_finalised = fin ? 1 : 0;
    if (!fin) return 0;
    // the 16-bit tag both halves of every sample entry of this launch carry (film_ops.h): never 0 (fresh memory) or 1 (a launch
    // that keeps the combine pass).  When the tags come round again no entry of any slab may still carry an old one: every slab
    // is zeroed -- behind whatever still reads one (the ring is idle here, so only a combine pass of an earlier batch on the main
    // stream can be pending: round-4 ADVICE), and in front of this launch AND of every later one: the next pipelined launch runs
    // on another stream and writes another slab, which nothing would order behind that slab's memset, so the host waits for the
    // memsets here (round-5 ADVICE; a wrap comes once in 65 534 launches)
    const unsigned phase = c->launch_seq % (unsigned)MPT_TAG_PERIOD, epoch = c->launch_seq / (unsigned)MPT_TAG_PERIOD;
    if (epoch != c->tag_epoch) {             // (told by the epoch, not by phase == 0: the launch with that number may have kept the combine pass)
        c->tag_epoch = epoch;
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (auto &slot : c->ring)
            if (slot.slab) HIP_TRY(hipMemsetAsync(slot.slab, 0, slot.slab.cap * sizeof(MptVec4), s.rs));
        HIP_TRY(hipStreamSynchronize(s.rs));
        c->tag_wraps++;
    }
    p.fin_counter = c->ring[s.k].heads + 8 * MPT_QUEUE_STRIDE;
    p.slab_tag = (unsigned)MPT_TAG_FIRST + phase;
    // everything the main stream still has to do to the film (an earlier batch's combine, a clear, a gather) comes first --
    // nothing, when the stream is idle (a step that ended with a read-back): then the event pair (8 us of API calls in front of
    // the launch, HIP trace of bench.py) is left out
    const hipError_t main_busy = hipStreamQuery(c->stream);
    if (main_busy == hipErrorNotReady) {
        HIP_TRY(hipEventRecord(c->ev_film, c->stream));
        HIP_TRY(hipStreamWaitEvent(s.rs, c->ev_film, 0));
    } else if (main_busy != hipSuccess) HIP_TRY(main_busy);
    // the resolved image as well, if the caller has said where get_image() will want it and this share is the whole film
    const size_t img_bytes = (size_t)c->nx * c->ny * sizeof(MptVec4);
    if (c->early.hint && c->opt.finalise == 1 && c->x0 == 0 && c->x1 == c->nx && c->stripe_w == 0 &&
        (p.image_out = (MptVec4 *)caller_alias(c, c->early.hint, img_bytes)) != nullptr) {
        c->early.ptr = c->early.hint; c->early.version = c->film_version; c->early.stream = s.rs;
    }
    return 0;
}

// step 8: the launch, between the two events of its timer
static int launch_render(mpt_ctx *c, const MptRenderParams &p, const BatchSlot &s, MptKernelChoice kc, int launch_cus, int lds_block,
                         int wide_blocks) {
    // SHADE compiled for what the scene uses: the LDS-resident 4-wide kernel has a plain instantiation, every other kernel the generic code
    const int shade_feat = kc.kernel == MPT_KERNEL_LDS4 ? shade_feat_instantiation(scene_feat_now(c), c->opt.shade_spec) : MPT_FEAT_GENERIC;
    // ... and the plain one a lean variant, for a scene none of whose materials has sheen or subsurface
    const int shade_lean = kc.kernel == MPT_KERNEL_LDS4 ? shade_lean_instantiation(shade_feat, scene_lean_now(c), c->lean_on) : 0;
    MptTimedSpan span(c->render_timer, s.rs);
    HIP_TRY(span.begun);
    switch (kc.kernel) {
    case MPT_KERNEL_LDS4: HIP_TRY(mpt_launch_render_lds4(&p, launch_cus, lds_block, (size_t)kc.lds_bytes, c->opt.count, shade_feat, shade_lean, s.rs)); break;
    case MPT_KERNEL_LDS: HIP_TRY(mpt_launch_render_lds(&p, launch_cus, lds_block, (size_t)kc.lds_bytes, c->opt.count, s.rs)); break;
    case MPT_KERNEL_WIDE: HIP_TRY(mpt_launch_render_wide(&p, wide_blocks, c->opt.count, c->opt.wide_quant, s.rs)); break;
    default:    // MPT_KERNEL_GATHER: the binary tree, in either build (strict: a workgroup per tile; fast: persistent workgroups on the launch's CUs)
        HIP_TRY(MPT_LAUNCHER(c, mpt_launch_render)(&p, s.fast ? launch_cus : p.ntiles, gather_stack_levels(c), c->opt.count, s.rs));
    }
    c->last_shade_feat = shade_feat;
    c->last_shade_lean = shade_lean;
    c->last_kernel = kc.kernel;
    HIP_TRY(span.end());
    return 0;
}

// step 9 (fast build), behind the launch: the main stream is ordered after it, the combine pass, the next batch's points
static int behind_launch(mpt_ctx *c, const MptRenderParams &p, const BatchSlot &s, int B, bool fin) {
    MptRingSlot &slot = c->ring[s.k];
    // everything later on the main stream (combine, gather, resolve, read-backs, scene changes) is
    // ordered after this render; the next batch, on the other stream, is not
    HIP_TRY(hipEventRecord(slot.rendered, s.rs));
    HIP_TRY(hipStreamWaitEvent(c->stream, slot.rendered, 0));
    if (!fin)
        HIP_TRY(mpt_launch_combine(c->fb.film[0], slot.slab, c->ny, c->x0, c->x1, p.stripe_w, p.stripe_pitch,
                                   p.partial_stride / std::max(c->ny, 1), B, c->stream));
    HIP_TRY(hipEventRecord(slot.consumed, c->stream));      // (a finalising launch has consumed its slab itself)
    // Ahead of time, on the aux stream: the Sobol points and zeroed queue heads of the NEXT batch, assuming it
    // has as many frames as this one and uses the next ring slot (the sampler's future is deterministic; its
    // state X moves only when that batch is really launched).  Takes 25 us of Sobol kernel + memset off the
    // head of every step.
    const int k2 = c->flip % c->cur_depth;
    if (k2 != s.k) {
        MptRingSlot &next = c->ring[k2];
        HIP_TRY(hipStreamWaitEvent(s.ss, next.rendered, 0));   // the batch that last read that slot's points and queue heads
        HIP_TRY(mpt_launch_sobol_update(c->sX, c->spec.X, c->sV, next.points, c->sdim, c->srows, c->stime, B, B, 1, s.ss));
        HIP_TRY(hipMemsetAsync(next.heads, 0, MPT_QUEUE_WORDS * sizeof(unsigned int), s.ss));
        HIP_TRY(hipEventRecord(next.ready, s.ss));
        c->spec.valid = true; c->spec.slot = k2; c->spec.B = B; c->spec.time = c->stime;
    }
    return 0;
}

extern "C" int mpt_flush(mpt_ctx *c) {
    if (!c) return fail("null context");
    if (c->mlt.pending && mlt_flush(c)) return 1;    // engines.cpp (its iterations and PathEngine frames are never pending together)
    if (c->pending == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const int B = c->pending;
    c->pending = 0;
    MptRenderParams p;
    if (fill_params(c, p, B)) return 1;
    const bool fast = c->opt.mode == MPT_MODE_FAST;
    if (fast && ring_policy(c, B)) return 1;                                               // 1
    BatchSlot s;
    s.fast = fast;
    s.k = fast ? (c->flip++ % c->cur_depth) : 0;
    s.rs = fast ? c->ring[s.k].stream : c->stream;
    s.ss = fast ? c->aux : c->stream;
    bool use_spec = false;
    if (batch_points(c, p, s, B, &use_spec)) return 1;                                     // 2
    if (p.ntiles == 0) return 0;                     // nothing to render: the sampler has moved
    const MptKernelChoice kc = choose_kernel(c);                                           // 3
    p.lds_nmats = c->max_mtlid + 1;                  // (render_kernel_lds4: the material records it keeps in LDS)
    const int ccols = work_items(c, p, B, fast);
    if (fast && slab_and_queue_heads(c, p, s, B, ccols, use_spec)) return 1;               // 4
    bool ring_idle = false;
    int launch_cus = 0, wide_blocks = 0, lds_block = 0;
    if (launch_share(c, fast, &ring_idle, &launch_cus)) return 1;                          // 5
    if (size_launch_buffers(c, p, s.k, kc.kernel, launch_cus, &wide_blocks, &lds_block)) return 1;   // 6
    const bool fin = fast && c->opt.finalise && ring_idle && p.nitems > 0;
    if (setup_finalisation(c, p, s, fin)) return 1;                                        // 7
    if (launch_render(c, p, s, kc, launch_cus, lds_block, wide_blocks)) return 1;          // 8
    return fast ? behind_launch(c, p, s, B, fin) : 0;                                      // 9
}

extern "C" int mpt_render(mpt_ctx *c, int nframes) {                           // path.py:75-77
    if (render_entry(c, nframes)) return 1;           // fail at the call, not at the deferred launch
    if (c->mlt.pending && mlt_flush(c)) return 1;     // the film sum follows call order: iterations of engines.cpp's chains enqueued before go first
    while (nframes > 0) {
        int room = c->opt.batch - c->pending;
        int take = std::min(room, nframes);
        c->pending += take;
        nframes -= take;
        if (c->pending >= c->opt.batch && mpt_flush(c)) return 1;
    }
    return 0;
}

// The read-out of an engine's launch timer: what is enqueued is launched, the main stream (and, for launches recorded on them, the
// aux and render streams) waited for, and the launches' segments summed: ms0, and ms1 where a launch has two.
int timer_readout(mpt_ctx *c, MptLaunchTimer &timer, double *ms0, double *ms1, int *launches, bool render_streams) {
    if (mpt_flush(c)) return 1;
    if (wait_all(c, render_streams)) return 1;
    double seg[2] = { 0, 0 };
    if (timer.drain(seg, launches)) return 1;
    if (ms0) *ms0 = seg[0];
    if (ms1) *ms1 = seg[1];
    return 0;
}

// a persistent render kernel that had to be stopped by its watchdog leaves a flag behind (in host-pinned
// memory: no copy to read it); call after the streams have been synchronised
int check_watchdog(mpt_ctx *c) {
    // read and re-arm: the failure is reported once, by the first read-back after it (the film holds
    // incomplete sums until the caller clears it)
    if (__atomic_exchange_n(c->watchdog.host.p, 0u, __ATOMIC_ACQ_REL))
        return fail("render kernel stopped by its watchdog (scheduler made no progress): film is incomplete");
    return 0;
}

extern "C" int mpt_synchronize(mpt_ctx *c) {                                   // worker.py:17-18
    if (use_ro(c)) return 1;
    if (mpt_flush(c)) return 1;
    if (wait_all(c)) return 1;
    return check_watchdog(c);
}

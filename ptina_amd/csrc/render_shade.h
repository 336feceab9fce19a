// render_shade.h -- production build of render_kernel.hip (its only includer; after render_lane.h): SHADE, the prepared primary
// rays, the work queues and trace_stream, the wave's scheduling loop.
#pragma once

// path.py:31-62 for one bounce.  On entry L.to / L.prd are the path ray r.o / r.d and
// (L.hidx >= 0, L.tbest, L.hidx, L.hu, L.hv) the closest hit.  shade_core is the bounce itself; what follows it --
// a shadow ray from hitpos towards the sampled light, or the next bounce from hitpos -- is the caller's (trace_stream).
enum { SH_END = 0, SH_BOUNCE = 1, SH_SHADOW = 2 };
// Diagnostic build -DMPT_X_STAMPS=2 (counting kernels): shader-clock cycles (units of 16) of the segments of SHADE, added by the
// first active lane into the pl_* counters: lights hit | geometry + material (waits for the gathers) | light sample |
// BSDF eval + MIS | BSDF sample | ray start
#if MPT_X_STAMPS == 2
#define MPT_SEG_BEGIN unsigned long long seg_t = 0; if (COUNT) { __builtin_amdgcn_sched_barrier(0); seg_t = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#define MPT_SEG(field) if (COUNT) { __builtin_amdgcn_sched_barrier(0); const unsigned long long seg_n = __builtin_amdgcn_s_memtime(); \
        const unsigned long long seg_m = __ballot(true); \
        const bool seg_first = __builtin_amdgcn_mbcnt_hi((unsigned)(seg_m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)seg_m, 0u)) == 0; \
        cnt.field += seg_first ? (unsigned)((seg_n - seg_t) >> 4) : 0u; seg_t = seg_n; __builtin_amdgcn_sched_barrier(0); }
#else
#define MPT_SEG_BEGIN
#define MPT_SEG(field)
#endif   // path over (miss: world light added) | next bounce from hitpos | shadow ray first
// FEAT: the scene's feature mask the kernel is compiled for (shade_feat.h; wave-uniform by construction: the host picks it per launch)
// LEAN: the lean variant of the plain instantiation (shade_feat.h shade_lean_scene: no material has sheen or subsurface)
template <bool COUNT, int FEAT, bool LEAN, class WALK>
DEV int shade_core(const MptRenderParams &p, const WALK &w, LaneState &L, Cnt &cnt, V3 &hitpos, V3 &sdir, float &sdis) {
    V3 ro = L.to, rd = L.prd;
    const bool was_hit = L.hidx >= 0;
    float hdepth = was_hit ? (WALK::T_SCALED ? L.tbest * p.t_unscale : L.tbest) : MPT_INF;
    // everything the stage gathers from L2 is asked for first: the shading record of the triangle and the six
    // Sobol numbers of the bounce (path.py:48,58: light triple, then BSDF triple) -- one round trip, under the
    // light tests, instead of three in a row
    // (the LDS-resident kernels: no initialisers -- both are read by lanes with a hit only, and "= {}" was 21 v_mov_b32 per stage; the
    //  gather kernels keep them: without, their register allocation spills 16 bytes more and loses 2 %)
    ShadeRec rec;
    float u[6];
    if constexpr (!WALK::LDS_RESIDENT) { rec = ShadeRec{}; for (int k = 0; k < 6; k++) u[k] = 0.0f; }
    MPT_SEG_BEGIN
    const int hslot = WALK::ODD_IDS ? (L.hidx >> 4) : L.hidx;
    if (was_hit) {
        rec = shade_rec_load<WALK::LDS_RESIDENT>(p, hslot);
        lane_draws<6, WALK::LDS_RESIDENT>(p, L, u);
    }
    MPT_SEG(pl_trips)            // (the entry of the stage -- reloads of what the traversal loop had parked -- and the issue of its gathers)
    LightHit lit = lights_hit<FEAT>(p, ro, rd);
    if (lit.hit && (!was_hit || lit.dis < hdepth)) {
        float mis = power_heuristic(L.last_brdf_pdf, lit.pdf);
        L.result = L.result + L.throughput * (lit.color * mis);
    }
    hitpos = ro; sdir = v3s(0.0f); sdis = 0.0f;
    MPT_SEG(pl_local)
    if (!was_hit) {
        L.result = L.result + L.throughput * world_at<FEAT>(p, rd);
        L.depth = 5;                                                         // break, path.py:39
        return SH_END;
    }
    L.navoid = WALK::ODD_IDS ? L.hidx : ~L.hidx;
    Hit hit; hit.hit = 1; hit.depth = hdepth; hit.index = hslot; hit.u = L.hu; hit.v = L.hv;
    V3 normal; Disney mat;
    get_geometries_rec<FEAT>(p, w, rec, hit, ro, rd, &hitpos, &normal, mat);
    if (COUNT) { cnt.n_shade++; cnt.n_draws += 6; }
    float sign = -dot(rd, normal);                                           // path.py:44-46 (never negative)
    if (sign < 0.0f) normal = -normal;
    MPT_SEG(pl_batches)

    LightSample li = lights_sample<FEAT>(p, hitpos, v3(u[0], u[1], u[2]));
    bool want_shadow = any_gt0(li.color);
    MPT_SEG(pl_batch_lanes)
    L.direct = v3s(0.0f);
    if (want_shadow) {
        // evaluated before the visibility is known; dropped if the shadow ray hits (path.py:50-56)
        V3 brdf_clr = disney_brdf<FEAT, LEAN>(mat, normal, sign, -rd, li.dir);
        float brdf_pdf = vavg(brdf_clr);
        float mis = power_heuristic(li.pdf, brdf_pdf);
        V3 direct_li = li.color * mis * brdf_clr * dot_or_zero(normal, li.dir);
        L.direct = L.throughput * direct_li;
    }
    MPT_SEG(pl_prim)
    BsdfSample brdf = disney_bounce<FEAT, LEAN>(mat, normal, sign, -rd, v3(u[3], u[4], u[5]));
    L.throughput = L.throughput * brdf.color;
    L.prd = brdf.outdir;
    L.last_brdf_pdf = brdf.pdf;
    MPT_SEG(pl_tidle)
    // A shadow ray decides whether `direct` is added (path.py:50-56).  When direct is exactly zero -- the light is behind the
    // surface (cos = 0), a black lobe, a dead throughput -- adding it or not is the same bits, so the ray is not traced:
    // an exact elimination (x + 0 == x; a NaN is != 0 and still takes the ray).  On the benchmark scene that is every
    // surface that faces away from the light: 3.5 % of all rays, 8 % of the node fetches (they are the long ones), -5 % time.
    // Option "skip_dark" = 0 traces them like the reference does.  In the strict build (no contraction) the two settings give the
    // same film bit for bit (tested); in this build a handful of pixels may differ in the last bits: -ffp-contract=fast is
    // free to fuse the multiply-adds of the two paths' ray set-up differently.
    if (want_shadow && p.n >= 2 && (p.skip_dark == 0 || any_ne0(L.direct))) {
        sdir = li.dir; sdis = li.dis;
        return SH_SHADOW;
    }
    if (want_shadow && p.n < 2) { L.result = L.result + L.direct; if (COUNT) cnt.rays++; }   // no geometry to occlude
    return SH_BOUNCE;
}

// do_render up to the camera ray, path.py:82-90, in two halves.  A wave prepares the primary rays of the next 64
// samples of its work item with all lanes on (lane l: sample base + l) and keeps them in eight registers; a lane
// whose path has ended fetches the ray of the sample it is handed with ds_bpermute.  Lanes finish a few at a time
// (a NEW pass found 6 of 64 lanes waiting on average), so the hash, the two Sobol loads and the camera
// transform ran at a tenth of the vector width when every lane prepared its own.
struct PrimaryPool {
    V3 ro, rd;
    int rng_i, rng_k;          // the pixel's proxy after the two jitter draws; rng_k < 0: no such pixel (tile past the edge)
};
DEV void pool_prepare(const MptRenderParams &p, PrimaryPool &pp, bool inside, int i, int j, int frame) {
    pp.ro = v3s(0.0f); pp.rd = v3s(0.0f); pp.rng_i = 0; pp.rng_k = -1;
    if (inside) {
        LaneState T;
        T.frame = frame;
        T.rng_i = wanghash2(i, j);                                           // path.py:72-73
        T.rng_k = reduce_mod_dim(T.rng_i, p.sobol_dim, p.sobol_inv_dim);
        float jit[2];
        lane_draws<2>(p, T, jit);                                            // random2: dx then dy, path.py:87
        float x = m_div((float)i + jit[0], (float)p.nx) * 2.0f - 1.0f;
        float y = m_div((float)j + jit[1], (float)p.ny) * 2.0f - 1.0f;
        camera_generate(p, x, y, &pp.ro, &pp.rd);
        pp.rng_i = T.rng_i; pp.rng_k = T.rng_k;
    }
}
DEV float lane_from(float v, int byte_lane) { return __int_as_float(__builtin_amdgcn_ds_bpermute(byte_lane, __float_as_int(v))); }
DEV int lane_from(int v, int byte_lane) { return __builtin_amdgcn_ds_bpermute(byte_lane, v); }

#ifndef MPT_PREF_NODE
#define MPT_PREF_NODE 1     // a NODE step when nodes * MPT_PREF_NODE >= leaves * MPT_PREF_LEAF, else a LEAF step
#define MPT_PREF_LEAF 1
#endif
#ifndef MPT_LEAVE_A
#define MPT_LEAVE_A 2    // leave traversal mode when traversing * A < waiting * B
#define MPT_LEAVE_B 1
#endif
// Diagnostic build (-DMPT_X_STAMPS=1, counting kernels only): the shader-clock cycles each wave spends in each
// stage, accumulated into the counters named in MPT_STAMP_END instead of their usual meaning (tools/gpu_diag.py stamps)
#if MPT_X_STAMPS
#define MPT_STAMP_BEGIN unsigned long long stamp_t0 = 0; if (COUNT) { __builtin_amdgcn_sched_barrier(0); stamp_t0 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#define MPT_STAMP_END(acc) if (COUNT) { __builtin_amdgcn_sched_barrier(0); acc += __builtin_amdgcn_s_memtime() - stamp_t0; __builtin_amdgcn_sched_barrier(0); }
#else
#define MPT_STAMP_BEGIN
#define MPT_STAMP_END(acc)
#endif
// diagnostics (counting kernels, option "lane_hist"): one issued stage -- how many lanes took part, and whose (depth, ray kind) they were
DEV void lane_hist_add(const MptRenderParams &p, int stage, bool part, int depth, int shadow) {
    unsigned long long *h = p.counters + MPT_HIST_BASE;
    const bool l0 = (threadIdx.x & 63) == 0;
    const int n = (int)__builtin_popcountll(__ballot(part));
    if (l0) atomicAdd(h + stage * 65 + n, 1ull);
    for (int d = 0; d < 6; d++)
        for (int k = 0; k < 2; k++) {
            const int c = (int)__builtin_popcountll(__ballot(part && min(depth, 5) == d && (shadow != 0) == (k != 0)));
            if (l0 && c) atomicAdd(h + 3 * 65 + (stage * 6 + d) * 2 + k, (unsigned long long)c);
        }
}
// diagnostics: a NODE stage's lane-steps by the bucket of the node's number (0 | 1 | 2-3 | 4-7 | ...): the 4-wide nodes are numbered
// breadth first, so "number < N" is "the top of the tree" -- what share of the fetches a cache of the top N records would serve
DEV void node_id_hist_add(const MptRenderParams &p, bool part, int id) {
    unsigned long long *h = p.counters + MPT_HIST_BASE + 3 * 65 + 3 * 6 * 2;
    const int b = id <= 0 ? 0 : 32 - __builtin_clz((unsigned)id);
    for (int k = 0; k < 24; k++) {
        const int c = (int)__builtin_popcountll(__ballot(part && b == k));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(h + k, (unsigned long long)c);
    }
}
DEV int wave_count(bool pred) { return (int)__builtin_popcountll(__ballot(pred)); }
DEV int wave_count32(bool pred) {            // a count that stays on the scalar unit when compared
    unsigned long long m = __ballot(pred);
    int n;                                   // one s_bcnt1_i32_b64, written out: the compiler's own 64-bit popcount ends up compared on the VALU, and
    asm("s_bcnt1_i32_b64 %0, %1" : "=s"(n) : "s"(m) : "scc");     // two 32-bit ones are three scalar instructions in the chain in front of every step
    return n;                                // (MI355X: 2.462 / 2.464 / 2.463 ms per launch -> 2.449 / 2.453 / 2.460; the gather kernels +0.8 %)
}

// Work items = (8x8 pixel tile, chunk of frames), tile-major, split into 8 contiguous ranges with
// one counter each.  A wave starts on the range of its XCD (blocks b, b+8, ... share an XCD) and
// moves on to the next range when one runs dry, so neighbouring tiles are traced by CUs behind the
// same L2 for as long as there is local work; every wave leaves when all eight ranges are exhausted.
// (Round 4, measured and taken out again -- profiles/r04_ab_experiments.json: a tapered end of launch, the younger waves of a SIMD
//  leaving the last items to the older.  Told by a look at the eight heads it made the launch 2.1-2.7 x slower -- which is how the
//  heads' shared cache line was found, mpt_types.h MPT_QUEUE_STRIDE -- and told by the pull's own result, free of any memory
//  access, 1-2 % slower: the end of a launch wants every wave it can get.  Also: the pull's atomic issued 8 / 16 / 32 samples ahead
//  of need: 2.89 / 2.89 / 2.92 against 2.88 ms -- its round trip is already hidden behind the wave's other lanes.)
struct WorkQueue {
    unsigned int *ctr;
    int nitems, q0, qoff;
    DEV int pull() {           // wave-uniform; -1 = no work left anywhere
        const int lane = threadIdx.x & 63;
        while (qoff < 8) {
            int q = (q0 + qoff) & 7;
            int lo = (int)(((long long)nitems * q) >> 3), hi = (int)(((long long)nitems * (q + 1)) >> 3);
            int k = 0;
            if (lane == 0) k = (int)atomicAdd(ctr + q * MPT_QUEUE_STRIDE, 1u);
            k = __builtin_amdgcn_readfirstlane(k);
            if (lo + k < hi) return lo + k;
            qoff++;
        }
        return -1;
    }
};

// One issued LEAF step of the traversal loop for the lanes that are ready for it: its counter, the optional histogram, the step.
// (The NODE body is still written out at its two places in trace_stream: as a function of its own it compiled to the same
//  instructions in another order in the binary LDS kernel.)
template <bool COUNT, class WALK>
DEV void step_leaf(const MptRenderParams &p, const WALK &w, typename WALK::Lifo &stk, LaneState &L, Cnt &cnt) {
    if (COUNT && (threadIdx.x & 63) == 0) cnt.it_leaf++;
    if (COUNT && p.lane_hist) lane_hist_add(p, 1, L.st == ST_LEAF, L.depth, L.shadow);
    if (L.st == ST_LEAF) stage_leaf<COUNT>(w, stk, L, cnt);
}

template <bool COUNT, int FEAT, bool LEAN = false, class WALK>
DEV void trace_stream(const MptRenderParams &p, const WALK &w, typename WALK::Lifo stk, WorkQueue wq, Cnt &cnt,
                      unsigned long long *tl = nullptr) {
    // work-item tiles are 2^tw_shift x 2^th_shift pixels (8x8 by default; smaller tiles shorten the
    // end-of-launch skew between waves at the price of primary-ray coherence)
    const int tws = p.tile_w_shift, ths = p.tile_h_shift, tps = tws + ths;
    const int t8y = (p.ny + (1 << ths) - 1) >> ths;
    int S = 0, next = 0;                            // wave-uniform: current pool = 64*frames samples; next unassigned
    int ti = 0, tj = 0, f0 = 0, tx_cur = 0;
    int ndead = 0;                                  // wave-uniform: lanes that have left for good
    int deferred = 0;                               // wave-uniform: lanes whose SHADE the last pass put off (MPT_SHADE_MIN)
    bool more = true;
    PrimaryPool pool;                               // lane l: primary ray of sample pool_base + l of the current item
    pool.ro = v3s(0.0f); pool.rd = v3s(0.0f); pool.rng_i = 0; pool.rng_k = -1;
    int pool_base = -64;
#if MPT_X_STAMPS
    unsigned long long acc_node = 0, acc_leaf = 0, acc_sdone = 0, acc_shade = 0, acc_new = 0;
    const unsigned long long stamp_start = __builtin_amdgcn_s_memtime();
#endif
    LaneState L;
    L.st = ST_NEW;
    L.sp = 0; L.curr = 0; L.shadow = 0;
    L.result = v3s(0.0f); L.throughput = v3s(0.0f); L.prd = v3s(0.0f); L.direct = v3s(0.0f);
    L.to = v3s(0.0f); L.td = v3s(0.0f); L.inv = v3s(0.0f); L.oinv = v3s(0.0f);
    L.offx = 0; L.offy = 0; L.offz = 0;
    L.tbest = 0.0f; L.hidx = -1; L.hu = 0.0f; L.hv = 0.0f; L.last_brdf_pdf = 0.0f;
    L.navoid = 0; L.depth = 0; L.rng_i = 0; L.rng_k = 0; L.pix = 0; L.frame = 0;
    // Every pass of this loop retires at least one stage for at least one lane, so it ends when the
    // queues are empty.  The pass counter is a watchdog only: a scheduling bug must not be able to keep
    // a persistent wave (and with it the GPU) spinning -- the host turns the flag into an error.
    for (unsigned guard = 0;; guard++) {
        if (guard > (1u << 26)) {
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(p.watchdog, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        // ---- traversal mode: tight loop while the lanes that are traversing outnumber the waiting ones
        for (;;) {
            // The decision in front of every step is a chain VALU compare -> scalar count -> scalar compare ->
            // branch that a wave cannot overlap with anything of its own (stamped: a fifth of its cycles went
            // there), so it is kept short: two ballots, counts in 32-bit scalar registers (a 64-bit popcount makes
            // the compiler compare on the VALU), the waiting lanes by subtraction, one branch per condition.
            const int cn = wave_count32(L.st == ST_NODE);
            const int cl = wave_count32(L.st == ST_LEAF);
            const int trav = cn + cl;
            if (trav == 0) break;
            // leave when the waiting lanes (DONE or NEW: everything alive that is not traversing) outnumber the
            // traversing ones 2 : 1 (best of the ratios tried on MI355X)
            if (trav * MPT_LEAVE_A < (64 - ndead - trav - deferred) * MPT_LEAVE_B) break;
            MPT_STAMP_BEGIN
            if (cn * MPT_PREF_NODE >= cl * MPT_PREF_LEAF) {
                if (COUNT && (threadIdx.x & 63) == 0) cnt.it_node++;
                if (COUNT && p.lane_hist) lane_hist_add(p, 0, L.st == ST_NODE, L.depth, L.shadow);
                if constexpr (!WALK::ODD_IDS) { if (COUNT && p.lane_hist) node_id_hist_add(p, L.st == ST_NODE, L.curr); }
                if (L.st == ST_NODE) {
                    if constexpr (WALK::WIDE) stage_node4<COUNT>(w, stk, L, cnt);
                    else stage_node<COUNT>(w, stk, L, cnt);
                }
                // further steps for the lanes that are still at a node, without counting again: the three ballots
                // and the decision chain in front of every step cost a wave about as many cycles as half a step.
                // (Measured and not kept, tools/scratch/r05_node_prefetch_attempt.patch: the second step's node record asked for
                //  the moment the first knows where the lane goes, before its pushes and the ballot in between: +1.6 % per launch.)
#pragma unroll
                for (int rep = 0; rep < WALK::NODE_REP; rep++) {
                    if (__ballot(L.st == ST_NODE) == 0ull) break;
                    if (COUNT && (threadIdx.x & 63) == 0) cnt.it_node++;
                    if (COUNT && p.lane_hist) lane_hist_add(p, 0, L.st == ST_NODE, L.depth, L.shadow);
                    if constexpr (!WALK::ODD_IDS) { if (COUNT && p.lane_hist) node_id_hist_add(p, L.st == ST_NODE, L.curr); }
                    if (L.st == ST_NODE) {
                        if constexpr (WALK::WIDE) stage_node4<COUNT>(w, stk, L, cnt);
                        else stage_node<COUNT>(w, stk, L, cnt);
                    }
                }
                MPT_STAMP_END(acc_node)
            } else {
                step_leaf<COUNT>(p, w, stk, L, cnt);
#pragma unroll
                for (int rep = 0; rep < WALK::LEAF_REP; rep++) {
                    if (__ballot(L.st == ST_LEAF) == 0ull) break;
                    step_leaf<COUNT>(p, w, stk, L, cnt);
                }
                MPT_STAMP_END(acc_leaf)
            }
        }
        // ---- shading mode
        bool shade_now = wave_count(L.st == ST_DONE && !L.shadow) != 0;
        if constexpr (WALK::SHADE_MIN > 0) {
            // SHADE costs a wave the same whatever the number of lanes in it (8 400 cycles; a NODE step 575): with fewer than
            // SHADE_MIN lanes waiting for it, and other lanes still traversing, the pass serves the cheap stages only and the
            // lanes wait for company (they are left out of the traversal loop's leave test meanwhile).  LDS-resident kernel:
            // SHADE at 36 lanes instead of 26, 3.18 -> 3.06 ms; the gather kernels, where a step costs three times as much and
            // an idle lane with it, lose 5-14 % and keep SHADE_MIN = 0.
            const int ns = wave_count(L.st == ST_DONE && !L.shadow);
            const int ntrav = wave_count(L.st == ST_NODE || L.st == ST_LEAF);
            shade_now = ns != 0 && (ns >= WALK::SHADE_MIN || ns * 2 >= 64 - ndead || ntrav == 0);
            deferred = shade_now ? 0 : ns;
        }
        if (shade_now) {
            if (COUNT && (threadIdx.x & 63) == 0) cnt.it_shade++;
            if (COUNT && p.lane_hist) lane_hist_add(p, 2, L.st == ST_DONE && !L.shadow, L.depth, 0);
            MPT_STAMP_BEGIN
            if (L.st == ST_DONE && !L.shadow) {
                V3 hitpos, sdir;
                float sdis;
                const int nk = shade_core<COUNT, FEAT, LEAN>(p, w, L, cnt, hitpos, sdir, sdis);
                L.to = hitpos;
                if (nk == SH_SHADOW) { L.td = sdir; L.tbest = sdis; L.st = ST_SHADOW; }
                else L.st = ST_BOUNCE;                                       // SH_END: depth is 5, the sample is stored below
            }
            MPT_STAMP_END(acc_shade)
        }
        {
            MPT_STAMP_BEGIN
            // a shadow ray has finished: the candidate direct light is added if nothing was hit (path.py:51,56); the next
            // bounce starts from hitpos (= the shadow ray's origin, still in L.to), path.py:60
            if (L.st == ST_DONE && L.shadow) {
                if (L.hidx < 0) L.result = L.result + L.direct;
                L.st = ST_BOUNCE;
            }
            if (L.st == ST_BOUNCE && !path_continues(L)) lane_store_sample(p, L);   // path.py:25,93: these lanes take a new sample below
            MPT_STAMP_END(acc_sdone)
        }
        MPT_STAMP_BEGIN
        unsigned long long m_new = __ballot(L.st == ST_NEW);
        if (m_new != 0ull) {
            if (next >= S && more) {                // pool drained: fetch the next work item right away,
                int item = wq.pull();               // while the other lanes are still busy (no per-item tail)
                if (item < 0) {
                    more = false;
                    if (tl && (threadIdx.x & 63) == 0) tl[2] = wall_clock64();
                } else {
                    int tile = item / p.nchunks, chunk = item - tile * p.nchunks;
                    int tx = tile / t8y, ty = tile - tx * t8y;
                    int tps_x = p.stripe_w >> tws, st = tx / tps_x;      // stripe of this tile column
                    ti = p.x0 + st * p.stripe_pitch + ((tx - st * tps_x) << tws); tj = ty << ths; tx_cur = tx;
                    f0 = chunk * p.chunk;
                    S = (min(f0 + p.chunk, p.nframes) - f0) << tps;
                    next = 0; pool_base = -64;
                }
            }
            if (next < S) {
                if (COUNT && (threadIdx.x & 63) == 0) cnt.it_new++;
                const int lane = threadIdx.x & 63;
                if (next >= pool_base + 64) {       // wave-uniform: the pool is used up (or belongs to the last item)
                    pool_base = next;
                    const int smp = pool_base + lane;
                    const int q = smp & ((1 << tps) - 1);
                    const int i = ti + (q >> ths), j = tj + (q & ((1 << ths) - 1));
                    pool_prepare(p, pool, smp < S && i < p.x1 && j < p.ny, i, j, f0 + (smp >> tps));
                }
                // idle lanes take the next consecutive samples (neighbouring pixels of one frame)
                const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m_new >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_new, 0u));
                const int smp = next + rank;
                const int pool_end = min(S, pool_base + 64);
                const int src = ((smp - pool_base) & 63) << 2;                 // every lane fetches: bpermute reads active lanes only
                V3 ro = v3(lane_from(pool.ro.x, src), lane_from(pool.ro.y, src), lane_from(pool.ro.z, src));
                V3 rd = v3(lane_from(pool.rd.x, src), lane_from(pool.rd.y, src), lane_from(pool.rd.z, src));
                const int rng_i = lane_from(pool.rng_i, src), rng_k = lane_from(pool.rng_k, src);
                if (L.st == ST_NEW && smp < pool_end && rng_k >= 0) {
                    const int q = smp & ((1 << tps) - 1);
                    L.frame = f0 + (smp >> tps);
                    // slot in this launch's sample slab: the columns of the share packed side by side
                    L.pix = ((tx_cur << tws) + (q >> ths)) * p.ny + (tj + (q & ((1 << ths) - 1)));
                    L.rng_i = rng_i; L.rng_k = rng_k; L.prd = rd;
                    L.navoid = 0; L.depth = 0;
                    L.result = v3s(0.0f); L.throughput = v3s(1.0f); L.last_brdf_pdf = 0.0f;
                    if (COUNT) { cnt.samples++; cnt.n_draws += 2; }
                    L.to = ro;
                    L.st = ST_BOUNCE;
                    if (!path_continues(L)) lane_store_sample(p, L);          // (a camera ray of zero length: path.py:25)
                }
                // NEW lanes beyond the pool's end keep waiting: the next pass prepares the next 64 samples
                next = min(next + (int)__builtin_popcountll(m_new), pool_end);
            } else if (!more) {
                if (L.st == ST_NEW) L.st = ST_DEAD;  // nothing left anywhere: those lanes are done
                ndead += (int)__builtin_popcountll(m_new);
            }
        }
        MPT_STAMP_END(acc_new)
        {
            MPT_STAMP_BEGIN
            if (L.st == ST_BOUNCE || L.st == ST_SHADOW) lane_begin_ray<COUNT, WALK>(p, L, stk, cnt);
            MPT_STAMP_END(acc_sdone)
        }
        if (ndead == 64) break;
    }
#if MPT_X_STAMPS
    if (COUNT) {       // the stage cycles (in units of 256) replace the work counters of this diagnostic build
        const bool l0 = (threadIdx.x & 63) == 0;
        const unsigned long long total = __builtin_amdgcn_s_memtime() - stamp_start;
        cnt.n_box = l0 ? (unsigned)(acc_node >> 8) : 0u; cnt.n_tri = l0 ? (unsigned)(acc_leaf >> 8) : 0u;
        cnt.n_draws = l0 ? (unsigned)(acc_sdone >> 8) : 0u; cnt.n_shade = l0 ? (unsigned)(acc_shade >> 8) : 0u;
        cnt.bounces = l0 ? (unsigned)(acc_new >> 8) : 0u; cnt.n_node = l0 ? (unsigned)(total >> 8) : 0u;
    }
#endif
}

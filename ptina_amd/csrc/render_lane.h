// render_lane.h -- production build of render_kernel.hip (its only includer): the per-lane state of the in-wave state machine
// and the three traversal steps (NODE, NODE over 4-wide records, LEAF).
#pragma once

// Production build: a WAVE owns an 8x8 pixel tile x the frames [f0, f1) = a pool of 64*(f1-f0)
// samples, and runs them as an in-wave state machine.  Measured on MI355X, the straightforward
// "each lane loops over its own path" megakernel is VALU-issue bound at ~14 % lane utilisation
// (SQ_THREAD_CYCLES_VALU / 64 / SQ_ACTIVE_INST_VALU): traversal trip counts, leaf tests and
// shading all diverge.  Here every lane carries a small state and the wave alternates between
//   traversal mode: a tight loop that runs ONE step per iteration for the lanes that are ready for
//       it -- NODE (two child-box tests, near child next, far child pushed) or LEAF (one triangle
//       test), whichever has more lanes -- for as long as most live lanes are traversing;
//   shading mode: lanes whose shadow ray finished add their direct light and start the next bounce;
//       lanes whose closest-hit query finished run SHADE (emitters, miss -> world, material, light
//       sample + BSDF eval, BSDF sample: the whole bounce); then NEW hands the idle lanes the next
//       samples of the pool (ballot + mbcnt compaction) and makes camera rays.
// A bounce issues its shadow ray first and keeps the next ray's direction and the candidate direct
// light C = throughput * mis * li * f * cos in registers; when the shadow traversal ends, C is
// added iff nothing was hit and the closest-hit traversal of the next bounce starts at once, so
// there is one shading stage per bounce and the order of additions into `result` is the
// reference's (path.py:31-56).  Rays, samples and sums do not depend on the schedule: each sample's
// radiance goes to p.partial[frame][column of the share][y] and the combine pass adds frames in order.
enum { ST_NODE = 0, ST_LEAF = 1, ST_DONE = 2, ST_NEW = 3, ST_DEAD = 4,     // DONE: this lane's ray is finished
       // inside one shading pass only: the lane's next ray starts in the pass's common block, from L.to --
       // a closest-hit ray along L.prd (head of the path_trace loop first) | a shadow ray along L.td up to L.tbest
       ST_BOUNCE = 5, ST_SHADOW = 6 };

// Per-lane state: live across the whole loop, so every word costs a VGPR for the kernel's lifetime.
struct LaneState {
    int st;
    // path, path.py:19-23
    V3 result, throughput;
    float last_brdf_pdf;
    int navoid, depth, rng_i;  // navoid: the id a node record holds for the triangle the ray left from (~slot; 0 = none:
                               // id 0 is the root, which is nobody's child)
    int rng_k;                 // rng_i reduced into [0, dim): the Sobol dimension of the lane's next draw
    int pix, frame;
    V3 prd;                    // closest ray: the path direction r.d; shadow ray: the NEXT bounce direction
    V3 direct;                 // shadow ray in flight: candidate direct light, added if unoccluded
    // ray being traversed (closest: the path ray; shadow: hitpos -> light)
    V3 to, td, inv, oinv;
    int offx, offy, offz;      // byte offset of the entry planes of each axis in a node record (binary LDS kernel: WALK::PLANE_OFF)
    float tbest;               // closest: best depth so far; shadow: li.dis, moved up one float where WALK::LDS_RESIDENT; x t_scale while traversed (T_SCALED)
    int curr, sp, hidx;        // hidx: leaf slot of the hit so far, -1 = none (closest) / any occluder found (shadow); in the 4-wide LDS kernel
                               // curr / hidx hold ids as its LDS node records do (LdsWalk4::ODD_IDS) and sp is the LDS address of the
                               // lane's top stack entry (LdsWalk4::SP_ADDR), everywhere else a level
    float hu, hv;
    int shadow;                // 1: the ray in flight is a shadow ray.  An int in a VGPR on purpose: as a bool the
                               // compiler keeps it in a scalar lane mask and re-merges that mask (s_andn2 / s_and /
                               // s_or) around every divergent region of the traversal loop
};

DEV Rng lane_rng(const MptRenderParams &p, const LaneState &L) {
    Rng r; r.dim = p.sobol_dim; r.P = p.P + (size_t)L.frame * p.sobol_dim; r.i = L.rng_i; return r;
}

// Python's floor-mod of the proxy counter by the table size (sobol.py:123), without an integer division:
// an estimate of the quotient from the float reciprocal, then the remainder is put right exactly
DEV int reduce_mod_dim(int h, int dim, float inv_dim) {
    // the float estimate is off by |h| / dim * 2^-23 at most: below one for tables of >= 1024 dimensions (the
    // reference's has 21201); smaller ones take the division (wave-uniform branch)
    if (dim < 1024) return pymod(h, dim);
    int q = (int)floorf((float)h * inv_dim);                       // within +-1 of floor(h / dim)
    int r = (int)((unsigned)h - (unsigned)q * (unsigned)dim);      // exact modulo 2^32, and the true remainder is small
    if (r < 0) r += dim;
    if (r < 0) r += dim;
    if (r >= dim) r -= dim;
    if (r >= dim) r -= dim;
    return r;
}

// N consecutive draws of the lane's Sobol proxy (sobol.py:121-125).  The proxy's counter is an i32
// that the reference reduces mod dim (floor-mod) at every draw; unless the counter is about to wrap
// (probability ~N/2^32 per pixel) the N indices are k, k+1, ... with one wrap at dim: the lane carries k
// along with the counter, so a draw costs a load and a compare.  The wrapping case takes the literal path.
template <int N, bool OFF32 = false>
DEV void lane_draws(const MptRenderParams &p, LaneState &L, float *out) {
    // OFF32 (WALK::LDS_RESIDENT): the frame's row as a 32-bit word offset from the scalar base (frames x dim stays below 2^30,
    // fill_params checks) instead of 64-bit arithmetic per lane; the gather kernels keep the long form (pt_device.h shade_rec_load)
#define MPT_ROW(k_) (OFF32 ? (const float *)((const char *)p.P + ((__umul24((unsigned)L.frame, (unsigned)p.sobol_dim) + (unsigned)(k_)) << 2)) \
                           : p.P + (size_t)L.frame * p.sobol_dim + (k_))
    const float *P = MPT_ROW(0);
    const int dim = p.sobol_dim;
    if (L.rng_i <= 0x7fffffff - N && L.rng_k + N <= dim) {
        // the N numbers are consecutive words (no wrap at dim inside them): two 16-byte gathers (any 4-byte
        // alignment) instead of six -- a gather instruction costs the big scenes the same whatever its width
        struct __attribute__((packed, aligned(4))) W4 { float a, b, c, d; };
        struct __attribute__((packed, aligned(4))) W2 { float a, b; };
        const float *q = MPT_ROW(L.rng_k);
        static_assert(N == 2 || N == 6, "lane_draws: two (jitter) or six (light + BSDF triples) numbers");
        if constexpr (N == 6) {
            const W4 v = *(const W4 *)q;
            int k2 = L.rng_k + 2;
            asm("" : "+v"(k2));                                              // (or the compiler turns it into two 4-byte gathers)
            const W4 w = *(const W4 *)MPT_ROW(k2);                           // overlaps the first: no read past the six
            out[0] = v.a; out[1] = v.b; out[2] = v.c; out[3] = v.d; out[4] = w.c; out[5] = w.d;
        } else {
            const W2 w = *(const W2 *)q;
            out[0] = w.a; out[1] = w.b;
        }
        const int k = L.rng_k + N;
        L.rng_k = k == dim ? 0 : k;
        L.rng_i += N;
    } else if (L.rng_i <= 0x7fffffff - N) {
        int k = L.rng_k;
#pragma unroll
        for (int t = 0; t < N; t++) {
            out[t] = P[k];
            k = (k + 1 == dim) ? 0 : k + 1;
        }
        L.rng_k = k;
        L.rng_i += N;
    } else {
        Rng rng = lane_rng(p, L);
#pragma unroll
        for (int t = 0; t < N; t++) out[t] = rng_random(rng);
        L.rng_i = rng.i;
        L.rng_k = pymod(L.rng_i, dim);
    }
#undef MPT_ROW
}

// One sample's radiance into the launch's slab, path.py:93 (the combine pass or the tail finalisation adds the frames in order).
// The entry is two self-validating 8-byte granules (film_ops.h: slab_pack), each written by ONE relaxed agent-scope 64-bit atomic
// store -- single-copy atomic by the language's memory model; on gfx950 a `global_store_dwordx2 ... sc1`, i.e. write-through: it
// leaves this XCD's L2 at once, where a finishing wave of any other XCD can see it.  A half that carries the launch's tag carries
// its data, so the data is the flag: nothing to order, no fence and no read-modify-write in the shading pass (the guide's R2 form:
// cdna_hip_programming.md Guideline 16, Pitfall 8 "ONE aligned 8-B store").  Every launch stores that way, finalising or not: a
// wave-uniform choice between two store flavours in the shading pass cost the whole kernel 4 % (it is short of scalar registers).
// Measured (MI355X, same box, three alternations, profiles/r05_ab_experiments.json): 2.603-2.613 ms per launch against 2.582-2.584
// with the same entry behind ONE 16-byte sc1 store (round 4's shape, whose halves are only observed to land together): the
// second store instruction costs 0.9 %, and buys a hand-off that rests on nothing but 64-bit atomicity.
DEV void store_sample(const MptRenderParams &p, int frame, int pix, V3 radiance) {
    MptVec4 *dst = p.partial + ((size_t)frame * (size_t)p.partial_stride + pix);
    const mpt_u4 v = slab_pack(radiance.x, radiance.y, radiance.z, p.slab_tag);
    unsigned long long *d64 = (unsigned long long *)dst;
    __hip_atomic_store(d64, ((unsigned long long)v.y << 32) | v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d64 + 1, ((unsigned long long)v.w << 32) | v.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the bottom entry of every ray's LIFO is a sentinel, so "pop" never needs an emptiness test:
// popping the sentinel means the traversal is over
template <class WALK>
DEV int classify(int v) {      // what a popped / chosen entry means for the lane's state
    if constexpr (WALK::ODD_IDS) return v & 3;      // node ids are multiples of 16 (ST_NODE == 0), leaf ids 16 * slot + 1 (ST_LEAF == 1), the sentinel is 2 (ST_DONE)
    else return v == WALK::SENTINEL ? ST_DONE : (v < 0 ? ST_LEAF : ST_NODE);
}

template <bool COUNT, class WALK>
DEV void lane_start_ray(LaneState &L, typename WALK::Lifo &stk, V3 o, V3 d, float tmax, bool shadow, Cnt &cnt) {
    L.to = o; L.td = d;
    L.inv = ray_inv(d);                       // (1 / d, finite for a component that is +-0: pt_device.h)
    if constexpr (WALK::T_SCALED) { L.inv = L.inv * stk.ts; tmax *= stk.ts; }
    L.oinv = o * L.inv;
    // which of an axis' two planes the ray enters through: offset of that plane in the node record
    if constexpr (WALK::PLANE_OFF != 0) {     // (the 4-wide gather kernels read the signs off L.inv in the step: three registers less to carry)
        L.offx = __float_as_int(L.inv.x) < 0 ? WALK::PLANE_OFF : 0;
        L.offy = __float_as_int(L.inv.y) < 0 ? WALK::PLANE_OFF : 0;
        L.offz = __float_as_int(L.inv.z) < 0 ? WALK::PLANE_OFF : 0;
    }
    // a shadow ray takes any occluder with depth <= li.dis (path.py:51), a closest-hit ray a strictly nearer hit (lbvh.py:331): with
    // the shadow ray's bound moved up to the next float the LEAF step asks both the same question, depth < tbest (the
    // LDS-resident kernels, -0.5 %; the gather kernels lose 1-2 % with it and keep the two tests)
    if constexpr (WALK::LDS_RESIDENT) {
        if (shadow) { const int b = __float_as_int(tmax); tmax = __int_as_float(b + (b < 0x7f800000 ? 1 : 0)); }
    }
    L.tbest = tmax; L.shadow = shadow ? 1 : 0; L.hidx = -1; L.hu = 0.0f; L.hv = 0.0f;
    stk.sp = 0;
    stk.push(WALK::SENTINEL);
    L.curr = 0;
    if constexpr (WALK::SP_ADDR) L.sp = stk.sp_at(1) - WALK::SP_BIAS; else L.sp = 1;
    if (COUNT) cnt.rays++;
    L.st = ST_NODE;
}

// The loop head alone (path.py:25): a lane about to bounce whose path is over stores its sample and waits for a new one
DEV bool path_continues(const LaneState &L) { return L.depth < 5 && any_gt0(L.throughput) && any_ne0(L.prd); }
DEV void lane_store_sample(const MptRenderParams &p, LaneState &L) {
    store_sample(p, L.frame, L.pix, L.result);                              // path.py:93, summed by combine
    L.st = ST_NEW;
}
// The one place of a shading pass where rays start: the lanes whose shadow ray just ended, the lanes that
// shaded and the lanes that took a new sample all come here, so the direction set-up (a normalisation, three reciprocals,
// the stack reset) is issued once per pass at the width of all of them, not three times at a third each
template <bool COUNT, class WALK>
DEV void lane_begin_ray(const MptRenderParams &p, LaneState &L, typename WALK::Lifo &stk, Cnt &cnt) {
    const bool sh = L.st == ST_SHADOW;
    const V3 n = normalized_unfused(L.prd);
    if (!sh) {
        L.depth += 1;
        if (COUNT) cnt.bounces++;
        L.prd = n;
    }
    const V3 d = sh ? L.td : n;
    lane_start_ray<COUNT, WALK>(L, stk, L.to, d, sh ? L.tbest : MPT_INF, sh, cnt);
    // lbvh.py:218,319: with fewer than two faces the root box is never written: no hit
    if (!sh && p.n < 2) L.st = ST_DONE;
}

// Traversal steps touch only (curr, sp, st) and, for leaves, the hit record: everything a finished
// ray triggers happens later, in shading mode, so the traversal loop carries no other live updates.
// They are written with two flat conditionals each (push / pop) instead of nested ones: on this
// code the nested form cost more scalar exec-mask bookkeeping than the box arithmetic itself.
// (Measured in-process A/B on MI355X and not kept: the twelve plane distances as six v_pk_fma_f32 --
//  5 % slower, packed f32 is not double-rate here; filtering the origin triangle in the leaf stage
//  instead of here -- within noise; per-stage instead of ratio scheduler thresholds -- within +-1 %.)
template <bool COUNT, class WALK>
DEV void stage_node(const WALK &w, typename WALK::Lifo &stk, LaneState &L, Cnt &cnt) {
    int id0, id1;
    float tn0, tn1;
    bool h0, h1;
    if (COUNT) { cnt.n_node++; cnt.n_box += 2; }
    int spec = 0;
    if constexpr (WALK::PEEK) spec = stk.peek(L.sp - 1);      // (the sentinel sits at level 0: sp >= 1 while a ray is traversed)
    if constexpr (WALK::PLANE_OFF != 0) {
        mpt_f2 nx, fx, ny, fy, nz, fz, ids;
        w.node_planes(L.curr, L.offx, L.offy, L.offz, nx, fx, ny, fy, nz, fz, ids);
        id0 = __float_as_int(ids.x); id1 = __float_as_int(ids.y);
        tn0 = fmaxf(fmaxf(__builtin_fmaf(nx.x, L.inv.x, -L.oinv.x), __builtin_fmaf(ny.x, L.inv.y, -L.oinv.y)),
                    fmaxf(__builtin_fmaf(nz.x, L.inv.z, -L.oinv.z), 0.0f));
        tn1 = fmaxf(fmaxf(__builtin_fmaf(nx.y, L.inv.x, -L.oinv.x), __builtin_fmaf(ny.y, L.inv.y, -L.oinv.y)),
                    fmaxf(__builtin_fmaf(nz.y, L.inv.z, -L.oinv.z), 0.0f));
        float tf0 = fminf(fminf(__builtin_fmaf(fx.x, L.inv.x, -L.oinv.x), __builtin_fmaf(fy.x, L.inv.y, -L.oinv.y)),
                          fminf(__builtin_fmaf(fz.x, L.inv.z, -L.oinv.z), L.tbest));
        float tf1 = fminf(fminf(__builtin_fmaf(fx.y, L.inv.x, -L.oinv.x), __builtin_fmaf(fy.y, L.inv.y, -L.oinv.y)),
                          fminf(__builtin_fmaf(fz.y, L.inv.z, -L.oinv.z), L.tbest));
        h0 = tn0 <= tf0; h1 = tn1 <= tf1;
    } else {
        MptVec4 a, b, c, d;
        w.node(L.curr, a, b, c, d);
        id0 = __float_as_int(d.x); id1 = __float_as_int(d.y);
        h0 = box_fast(a.x, b.x, c.x, a.z, b.z, c.z, L.inv, L.oinv, L.tbest, &tn0);
        h1 = box_fast(a.y, b.y, c.y, a.w, b.w, c.w, L.inv, L.oinv, L.tbest, &tn1);
    }
    // a leaf that is the triangle the ray left from is never tested (lbvh.py:329)
    h0 = h0 && (id0 != L.navoid);
    h1 = h1 && (id1 != L.navoid);
    bool swap = tn1 < tn0;
    int nearid = swap ? id1 : id0, farid = swap ? id0 : id1;
    int next = h0 ? (h1 ? nearid : id0) : id1;
    if constexpr (WALK::PEEK) {
        // the entry a pop would return was asked for with the node record (spec, below the function's head): a step that
        // pops does not wait a second LDS round trip behind the box tests.  Push (both hit) and pop (both missed) exclude
        // each other, and a push goes to level sp, not sp - 1
        int sp = L.sp;
        if (h0 && h1) { stk.sp = sp; stk.push(farid); sp++; }
        if (!(h0 || h1)) { next = spec; sp--; }
        L.sp = sp;
    } else {
        stk.sp = L.sp;
        if (h0 && h1) stk.push(farid);
        if (!(h0 || h1)) next = stk.pop();
        L.sp = stk.sp;
    }
    L.curr = next;
    L.st = classify<WALK>(next);
}

// min(a, b, c, tbest) of a slab test's exit side.  Written as the two instructions themselves: through fminf the compiler first
// quiets a signalling NaN its analysis cannot rule out in tbest (a register carried round the loop) -- one v_max_f32 tbest, tbest
// per step, and min / max issue at half the rate of an FMA on gfx950.  The instructions return the same bits as fminf for every
// input that is not a signalling NaN, and nothing in the kernel makes one.  MI355X, same box, alternated three times
// (profiles/r05_ab_experiments.json): 2.593 / 2.566 / 2.554 ms per launch -> 2.560 / 2.537 / 2.526.  (The 8-bit step of the
// gather kernels, which wait for their gathers as much as for the issue port, did not move with it: C4 1547 / 1543 against 1546 / 1549.)
DEV float exit_min(float a, float b, float c, float tbest) {
    float m, r;
    asm("v_min_f32 %0, %1, %2" : "=v"(m) : "v"(c), "v"(tbest));
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(m));
    return r;
}

// The same step through a 4-wide node: four slab tests (planes picked by the ray's direction signs) on one 128-B
// record, the children that are hit sorted
// by entry distance (a five-comparator network on (distance bits, id) pairs; a miss sorts last), the nearest
// taken next and the others pushed farthest first.
template <bool COUNT, class WALK>
DEV void stage_node4(const WALK &w, typename WALK::Lifo &stk, LaneState &L, Cnt &cnt) {
    typedef typename WALK::Lifo LIFO;
    int id0, id1, id2, id3;
    float t0, t1, t2, t3;
    bool h0, h1, h2, h3;
    if (COUNT) { cnt.n_node++; cnt.n_box += 4; }
    // the entry a step without a hit pops is asked for together with the node record: some lane of the wave pops in nearly every
    // step, and the wave then waited a second LDS round trip behind the sort (pushes go above the top entry, never onto it)
    int spec = 0;
    if constexpr (WALK::SP_ADDR) spec = LIFO::ld(L.sp - WALK::SP_STEP + WALK::SP_BIAS);
    if constexpr (WALK::QUANT) {
        MptVec4 ra, rb, rc, idv;
        w.node4q(L.curr, ra, rb, rc, idv);
        id0 = __float_as_int(idv.x); id1 = __float_as_int(idv.y); id2 = __float_as_int(idv.z); id3 = __float_as_int(idv.w);
        // plane = origin + q * scale, so its distance along the ray is q * (scale * inv) + (origin * inv - o * inv)
        const float sx = ra.w * L.inv.x, sy = rb.x * L.inv.y, sz = rb.y * L.inv.z;
        const float bx = __builtin_fmaf(ra.x, L.inv.x, -L.oinv.x), by = __builtin_fmaf(ra.y, L.inv.y, -L.oinv.y),
                    bz = __builtin_fmaf(ra.z, L.inv.z, -L.oinv.z);
        const unsigned lox = (unsigned)__float_as_int(rb.z), hix = (unsigned)__float_as_int(rb.w);
        const unsigned loy = (unsigned)__float_as_int(rc.x), hiy = (unsigned)__float_as_int(rc.y);
        const unsigned loz = (unsigned)__float_as_int(rc.z), hiz = (unsigned)__float_as_int(rc.w);
        // entry planes: the low ones for a ray going up the axis, the high ones for one going down (L.off*: per-ray flags)
        const bool dnx = __float_as_int(L.inv.x) < 0, dny = __float_as_int(L.inv.y) < 0, dnz = __float_as_int(L.inv.z) < 0;
        const unsigned nxq = dnx ? hix : lox, fxq = dnx ? lox : hix;
        const unsigned nyq = dny ? hiy : loy, fyq = dny ? loy : hiy;
        const unsigned nzq = dnz ? hiz : loz, fzq = dnz ? loz : hiz;
#define MPT_UB(w, c) ((float)(((w) >> (8 * (c))) & 0xffu))
#define MPT_QSLAB(c, tn, h)                                                                                            \
        tn = fmaxf(fmaxf(__builtin_fmaf(MPT_UB(nxq, c), sx, bx), __builtin_fmaf(MPT_UB(nyq, c), sy, by)),               \
                   fmaxf(__builtin_fmaf(MPT_UB(nzq, c), sz, bz), 0.0f));                                                 \
        h = tn <= fminf(fminf(__builtin_fmaf(MPT_UB(fxq, c), sx, bx), __builtin_fmaf(MPT_UB(fyq, c), sy, by)),          \
                        fminf(__builtin_fmaf(MPT_UB(fzq, c), sz, bz), L.tbest));
        MPT_QSLAB(0, t0, h0) MPT_QSLAB(1, t1, h1) MPT_QSLAB(2, t2, h2) MPT_QSLAB(3, t3, h3)
#undef MPT_QSLAB
#undef MPT_UB
    } else {
        MptVec4 nx, fx, ny, fy, nz, fz, idv;
        w.node4(L.curr, __float_as_int(L.inv.x) < 0 ? 16 : 0, __float_as_int(L.inv.y) < 0 ? 16 : 0, __float_as_int(L.inv.z) < 0 ? 16 : 0,
                 nx, fx, ny, fy, nz, fz, idv);
        id0 = __float_as_int(idv.x); id1 = __float_as_int(idv.y); id2 = __float_as_int(idv.z); id3 = __float_as_int(idv.w);
#define MPT_SLAB(c, tn, h)                                                                                              \
        tn = fmaxf(fmaxf(__builtin_fmaf(nx.c, L.inv.x, -L.oinv.x), __builtin_fmaf(ny.c, L.inv.y, -L.oinv.y)),            \
                   WALK::T_SCALED ? __builtin_amdgcn_fmed3f(__builtin_fmaf(nz.c, L.inv.z, -L.oinv.z), 0.0f, 1.0f)       \
                                   : fmaxf(__builtin_fmaf(nz.c, L.inv.z, -L.oinv.z), 0.0f));                             \
        h = tn <= exit_min(__builtin_fmaf(fx.c, L.inv.x, -L.oinv.x), __builtin_fmaf(fy.c, L.inv.y, -L.oinv.y),          \
                           __builtin_fmaf(fz.c, L.inv.z, -L.oinv.z), L.tbest);
        MPT_SLAB(x, t0, h0) MPT_SLAB(y, t1, h1) MPT_SLAB(z, t2, h2) MPT_SLAB(w, t3, h3)
#undef MPT_SLAB
    }
    // entry distances are >= 0, so their bit patterns order like the values; a miss (or the triangle the ray
    // left from, lbvh.py:329) gets the largest key
    const unsigned MISS = 0xffffffffu;
    unsigned k0, k1, k2, k3;
    if constexpr (WALK::IDS16) {
        // 16-bit ids (the LDS-resident kernel): the upper half of the distance's bits over the id is ONE word that sorts with
        // v_min_u32 / v_max_u32 -- ten instructions instead of the 25 of five compare-and-swaps on (key, id) pairs; distances that
        // agree in their first 8 mantissa bits are met in id order, which costs a step now and then and never a hit (the
        // order only decides what is looked at first)
        k0 = h0 ? __builtin_amdgcn_perm((unsigned)__float_as_int(t0), (unsigned)id0, 0x07060100u) : MISS;
        k1 = h1 ? __builtin_amdgcn_perm((unsigned)__float_as_int(t1), (unsigned)id1, 0x07060100u) : MISS;
        k2 = h2 ? __builtin_amdgcn_perm((unsigned)__float_as_int(t2), (unsigned)id2, 0x07060100u) : MISS;
        k3 = h3 ? __builtin_amdgcn_perm((unsigned)__float_as_int(t3), (unsigned)id3, 0x07060100u) : MISS;
        const unsigned a0 = min(k0, k1), a1 = max(k0, k1), b0 = min(k2, k3), b1 = max(k2, k3);
        const unsigned m0 = max(a0, b0), m1 = min(a1, b1);
        k0 = min(a0, b0); k3 = max(a1, b1); k1 = min(m0, m1); k2 = max(m0, m1);    // (measured and not kept: without this fifth
        // comparator -- the middle pair in whatever order the network leaves it -- the step is two instructions shorter and the launch 1.8 % longer)
        id0 = (int)(k0 & 0xffffu);                                                           // (ODD_IDS: unsigned)
        id1 = (int)k1; id2 = (int)k2; id3 = (int)k3;                                         // (the pushes store the low halves)
    } else {
        k0 = h0 ? (unsigned)__float_as_int(t0) : MISS;
        k1 = h1 ? (unsigned)__float_as_int(t1) : MISS;
        k2 = h2 ? (unsigned)__float_as_int(t2) : MISS;
        k3 = h3 ? (unsigned)__float_as_int(t3) : MISS;
#define MPT_CSWAP(ka, ia, kb, ib) { bool sw = kb < ka; unsigned tk = sw ? kb : ka; kb = sw ? ka : kb; ka = tk; \
                                    int ti_ = sw ? ib : ia; ib = sw ? ia : ib; ia = ti_; }
        MPT_CSWAP(k0, id0, k1, id1) MPT_CSWAP(k2, id2, k3, id3) MPT_CSWAP(k0, id0, k2, id2) MPT_CSWAP(k1, id1, k3, id3)
        MPT_CSWAP(k1, id1, k2, id2)
#undef MPT_CSWAP
    }
    int next = id0;
    // The three pushes are plain stores at a running index -- a store that is not wanted lands on the slot the next one overwrites --
    // instead of three divergent regions with a spill test each: always where the stack holds every level the tree can ask for in
    // LDS (SP_ADDR: an address has no spilled form), else while no lane of the wave is within three entries of the LDS part of its
    // stack (the rule, not the exception)
    if constexpr (WALK::SP_ADDR) {                                                    // (sp: the address of the top entry)
        int sp = L.sp;
        LIFO::st(sp + WALK::SP_BIAS, id3); sp += k3 != MISS ? WALK::SP_STEP : 0;
        LIFO::st(sp + WALK::SP_BIAS, id2); sp += k2 != MISS ? WALK::SP_STEP : 0;
        LIFO::st(sp + WALK::SP_BIAS, id1); sp += k1 != MISS ? WALK::SP_STEP : 0;
        if (k0 == MISS) { sp -= WALK::SP_STEP; next = spec; }
        L.sp = sp;
    } else if (__ballot(L.sp > WALK::CAP - 3) == 0ull) {
        int sp = L.sp;
        stk.stack[sp * MPT_BLOCK] = id3; sp += k3 != MISS ? 1 : 0;
        stk.stack[sp * MPT_BLOCK] = id2; sp += k2 != MISS ? 1 : 0;
        stk.stack[sp * MPT_BLOCK] = id1; sp += k1 != MISS ? 1 : 0;
        if (k0 == MISS) { sp--; next = stk.stack[sp * MPT_BLOCK]; }                     // sorted: then nothing was pushed
        L.sp = sp;
    } else {
        stk.sp = L.sp;
        if (k3 != MISS) stk.push(id3);
        if (k2 != MISS) stk.push(id2);
        if (k1 != MISS) stk.push(id1);
        if (k0 == MISS) next = stk.pop();
        L.sp = stk.sp;
    }
    L.curr = next;
    L.st = classify<WALK>(next);
}

template <bool COUNT, class WALK>
DEV void stage_leaf(const WALK &w, typename WALK::Lifo &stk, LaneState &L, Cnt &cnt) {
    int slot = WALK::ODD_IDS ? L.curr : ~L.curr;      // (ODD_IDS: the leaf's id stands for the slot until a shading pass needs it)
    bool stop = false;
    // (the counters count the reference's work: it never tests the triangle a ray left from, lbvh.py:329)
    if (COUNT) cnt.n_tri += (WALK::WIDE && L.curr == L.navoid) ? 0u : 1u;
    int spec = 0;
    if constexpr (WALK::SP_ADDR) spec = WALK::Lifo::ld(L.sp - WALK::SP_STEP + WALK::SP_BIAS);
    else if constexpr (WALK::PEEK) spec = stk.peek(L.sp - 1);      // a leaf step always pops: asked for with the triangle record
    MptVec4 g0, g1, g2;
    w.tri(slot, g0, g1, g2);
    float dd, su, sv;
    bool hit = tri_test_fast(g0, g1, g2, L.to, L.td, &dd, &su, &sv);
    if constexpr (WALK::T_SCALED) dd *= stk.ts;                            // (L.tbest is held scaled while the ray is traversed)
    if constexpr (WALK::WIDE) hit = hit && L.curr != L.navoid;              // the triangle the ray left from (lbvh.py:329): the 4-wide NODE step let it through
    if constexpr (WALK::LDS_RESIDENT) {
        if (hit && dd < L.tbest) {                                          // lbvh.py:331; path.py:51 (lane_start_ray)
            L.tbest = dd; L.hidx = slot; L.hu = su; L.hv = sv;
            stop = L.shadow != 0;
        }
    } else if (hit) {
        if (L.shadow) {
            if (dd <= L.tbest) { L.hidx = slot; stop = true; }              // path.py:51: any occluder within li.dis
        } else if (dd < L.tbest) {                                          // lbvh.py:331
            L.tbest = dd; L.hidx = slot; L.hu = su; L.hv = sv;
        }
    }
    int next;
    if constexpr (WALK::SP_ADDR) {
        next = spec; L.sp = L.sp - WALK::SP_STEP;
    } else if constexpr (WALK::PEEK) {
        next = spec; L.sp = L.sp - 1;
    } else {
        stk.sp = L.sp;
        next = stk.pop();
        L.sp = stk.sp;
    }
    L.curr = next;
    L.st = stop ? ST_DONE : classify<WALK>(next);
}

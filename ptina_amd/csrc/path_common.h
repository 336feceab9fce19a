// path_common.h -- one path of the unidirectional integrator (do_render + path_trace, engine/path.py:18-93) and the
// per-lane tracer each build walks it with.  Shared by the PathEngine kernels (render_kernel.hip) and the Metropolis chain
// kernel (mlt_kernel.hip): one definition of the path, so that a chain's path and a PathEngine sample given the same
// draws are the same path.  Also here: the brute-force engine's loop body (brute_step, engine/brute.py:29-60; brute_kernel.hip)
// and the 16x16-tile pixel mapping of the one-lane-per-pixel kernels; the name of a build's kernels and launchers (MPT_SUFFIX) and the
// launch of a kernel of the shape they share (launch_by_stack).
// Included once per translation unit; MPT_STRICT selects the build.
#pragma once
#include "pt_device.h"

// what both builds define carries the build in its name: mpt_launch_brute_strict / mpt_launch_brute_fast (miptina_ctx.h MPT_DUAL_LAUNCHER)
#if MPT_STRICT
#define MPT_SUFFIX(x) x##_strict
#else
#define MPT_SUFFIX(x) x##_fast
#endif

// ---------------------------------------------------------------- one lane per pixel of a 16x16 tile (strict render, preview, brute)
DEV int xcd_remap(int b, int nb) {
    // blocks are dealt round-robin over the 8 XCDs: give XCD k the k-th contiguous run of work
    int q = nb >> 3, r = nb & 7;
    int xcd = b & 7, k = b >> 3;
    return xcd * q + (xcd < r ? xcd : r) + k;
}

DEV bool tile_pixel(const MptRenderParams &p, int tile, int *pi, int *pj) {
    int tx = tile / p.tiles_y, ty = tile - tx * p.tiles_y;
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int tps_x = p.stripe_w / MPT_TILE, st = tx / tps_x;                       // stripe of this tile column
    int i = p.x0 + st * p.stripe_pitch + (tx - st * tps_x) * MPT_TILE + (wave >> 1) * 8 + (lane >> 3);
    int j = ty * MPT_TILE + (wave & 1) * 8 + (lane & 7);
    *pi = i; *pj = j;
    return i < p.x1 && j < p.ny;
}


#if MPT_STRICT
struct StrictTracer {
    const MptRenderParams *p;
    int *lds;
    template <bool COUNT>
    DEV Hit closest(V3 ro, V3 rd, int avoid, Cnt &cnt) const { return bvh_closest<COUNT>(*p, lds, ro, rd, avoid, cnt); }
    template <bool COUNT>
    DEV bool occluded(V3 ro, V3 rd, int avoid, float dis, Cnt &cnt) const {
        return bvh_occluded<COUNT>(*p, lds, ro, rd, avoid, dis, cnt);
    }
};
typedef StrictTracer BlockTracer;
DEV BlockTracer make_block_tracer(const MptRenderParams &p, int *lds) {
    BlockTracer t; t.p = &p; t.lds = lds; return t;
}
#else
typedef Tracer<GatherWalk> BlockTracer;
DEV BlockTracer make_block_tracer(const MptRenderParams &p, int *lds) {
    BlockTracer t;
    t.w.fnode = p.fnode; t.w.tgeo = p.tfast;
    t.st.stack = lds; t.st.sp = 0;
    t.n = p.n;
    return t;
}
#endif

// ---------------------------------------------------------------- one path = do_render + path_trace (path.py:18-93)
struct PathState {
    Rng rng;
    V3 ro, rd, result, throughput;
    float last_brdf_pdf;
    int avoid, depth;
};

// do_render up to the camera ray, path.py:82-90, for pixel (i, j) and batch frame f
template <bool COUNT>
DEV void path_begin(const MptRenderParams &p, PathState &s, int i, int j, int f, Cnt &cnt) {
    s.rng.dim = p.sobol_dim;
    s.rng.P = p.P + (size_t)f * p.sobol_dim;
    s.rng.i = wanghash2(i, j);                                               // path.py:72-73
    float dx = rng_random(s.rng), dy = rng_random(s.rng);
    float x = m_div((float)i + dx, (float)p.nx) * 2.0f - 1.0f;
    float y = m_div((float)j + dy, (float)p.ny) * 2.0f - 1.0f;
    camera_generate(p, x, y, &s.ro, &s.rd);
    s.avoid = -1; s.depth = 0;
    s.result = v3s(0.0f); s.throughput = v3s(1.0f); s.last_brdf_pdf = 0.0f;
    if (COUNT) { cnt.samples++; cnt.n_draws += 2; }
}

// do_render's camera ray for a path whose draws are all given (the Metropolis engine, mltpath.py:66-68): the proxy reads
// the chain's vector X from dim 0 in order, and the first two draws ARE the screen position, X[0] * 2 - 1 and X[1] * 2 - 1
template <bool COUNT>
DEV void path_begin_vec(const MptRenderParams &p, PathState &s, const float *X, Cnt &cnt) {
    s.rng.dim = 32;
    s.rng.P = X;
    s.rng.i = 0;
    float x = rng_random(s.rng) * 2.0f - 1.0f;
    float y = rng_random(s.rng) * 2.0f - 1.0f;
    camera_generate(p, x, y, &s.ro, &s.rd);
    s.avoid = -1; s.depth = 0;
    s.result = v3s(0.0f); s.throughput = v3s(1.0f); s.last_brdf_pdf = 0.0f;
    if (COUNT) { cnt.samples++; cnt.n_draws += 2; }
}

// one iteration of the path_trace loop, path.py:25-62; returns true when the path has ended
template <bool COUNT, class TR>
DEV bool path_step(const MptRenderParams &p, const TR &tr, PathState &s, Cnt &cnt) {
    if (!(s.depth < 5 && any_gt0(s.throughput) && any_ne0(s.rd))) return true;   // loop head, path.py:25
    s.depth += 1;
    if (COUNT) cnt.bounces++;

    s.rd = normalized(s.rd);
    Hit hit = tr.template closest<COUNT>(s.ro, s.rd, s.avoid, cnt);

    LightHit lit = lights_hit(p, s.ro, s.rd);
    if (lit.hit && (hit.hit == 0 || lit.dis < hit.depth)) {
        float mis = power_heuristic(s.last_brdf_pdf, lit.pdf);
        s.result = s.result + s.throughput * (lit.color * mis);
    }

    if (hit.hit == 0) {
        s.result = s.result + s.throughput * world_at(p, s.rd);
        return true;                                                         // break, path.py:39
    }
    s.avoid = hit.index;
    V3 hitpos, normal; Disney material;
    get_geometries(p, hit, s.ro, s.rd, &hitpos, &normal, material);
    if (COUNT) { cnt.n_shade++; cnt.n_draws += 6; }

    float sign = -dot(s.rd, normal);                                         // path.py:44-46 (never negative)
    if (sign < 0.0f) normal = -normal;

    LightSample li = lights_sample(p, hitpos, random3(s.rng));
    if (any_gt0(li.color)) {
        // (the candidate is a pure function of the bounce: evaluated before the shadow ray so that option "skip_dark" can
        //  leave out a ray whose candidate is exactly zero; the reference traces first and evaluates if unoccluded -- same values)
        V3 brdf_clr = disney_brdf(material, normal, sign, -s.rd, li.dir);
        float brdf_pdf = vavg(brdf_clr);
        float mis = power_heuristic(li.pdf, brdf_pdf);
        V3 direct_li = li.color * mis * brdf_clr * dot_or_zero(normal, li.dir);
        V3 direct = s.throughput * direct_li;
        if (p.skip_dark == 0 || any_ne0(direct))
            if (!tr.template occluded<COUNT>(hitpos, li.dir, s.avoid, li.dis, cnt))
                s.result = s.result + direct;
    }

    BsdfSample brdf = disney_bounce(material, normal, sign, -s.rd, random3(s.rng));
    s.throughput = s.throughput * brdf.color;
    s.ro = hitpos;
    s.rd = brdf.outdir;
    s.last_brdf_pdf = brdf.pdf;
    return false;
}

// one iteration of BruteEngine.trace's loop, brute.py:35-58; returns true when the path has ended.  path_trace without light
// sampling: no LightPool().sample, no shadow ray, no MIS weight (a light counts only when a bounce ray hits it), ONE random3
// per bounce, and the loop head compares the throughput with eps = 1e-6 (common.py:32) and does not look at r.d.
// PathState's last_brdf_pdf is not used.
template <bool COUNT, class TR>
DEV bool brute_step(const MptRenderParams &p, const TR &tr, PathState &s, Cnt &cnt) {
    const float eps = 1e-6f;
    if (!(s.depth < 5 && (s.throughput.x > eps || s.throughput.y > eps || s.throughput.z > eps))) return true;   // brute.py:35
    s.depth += 1;
    if (COUNT) cnt.bounces++;

    s.rd = normalized(s.rd);
    Hit hit = tr.template closest<COUNT>(s.ro, s.rd, s.avoid, cnt);

    LightHit lit = lights_hit(p, s.ro, s.rd);
    if (lit.hit && (hit.hit == 0 || lit.dis < hit.depth))
        s.result = s.result + s.throughput * lit.color;                      // brute.py:41-43

    if (hit.hit == 0) {
        s.result = s.result + s.throughput * world_at(p, s.rd);
        return true;                                                         // break, brute.py:47
    }
    s.avoid = hit.index;
    V3 hitpos, normal; Disney material;
    get_geometries(p, hit, s.ro, s.rd, &hitpos, &normal, material);
    if (COUNT) { cnt.n_shade++; cnt.n_draws += 3; }

    float sign = -dot(s.rd, normal);                                         // brute.py:52-54
    if (sign < 0.0f) normal = -normal;

    BsdfSample brdf = disney_bounce(material, normal, sign, -s.rd, random3(s.rng));
    s.throughput = s.throughput * brdf.color;
    s.ro = hitpos;
    s.rd = brdf.outdir;
    return false;
}

// ---------------------------------------------------------------- host side: the launch of a block-tracer kernel
// The kernels that walk through make_block_tracer are `template <int STACK>` with `__shared__ int s_stack[STACK * MPT_BLOCK]` and
// have two instantiations each, 32 and 64 levels; `stack` is what the tree asks for (lds_layout.h mpt_gather_stack_levels).
// Which of the two serves it: 0 or 1
static int stack_instantiation(int stack) { return stack <= 32 ? 0 : 1; }

// `grid` workgroups of MPT_BLOCK lanes of K32 or K64, the same kernel's <32> and <64>
template <auto K32, auto K64, class... A>
static hipError_t launch_by_stack(int stack, unsigned grid, hipStream_t stream, const A &...args) {
    static const decltype(K32) variants[2] = { K32, K64 };
    hipLaunchKernelGGL(variants[stack_instantiation(stack)], dim3(grid), dim3(MPT_BLOCK), 0, stream, args...);
    return hipGetLastError();
}

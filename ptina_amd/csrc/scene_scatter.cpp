// scene_scatter.cpp -- scatters behind mpt_scatter_* (DESIGN.md section 3.21): instances of a mesh placed over a surface object of
// the table on the device.  The table of scatters beside scene_compose.cpp's object table; the arenas of the surfaces' weights,
// shares and scans and of the instances' sticky records; and the steps of mpt_compose: scatter_ready (its refusals, before anything
// changes), scatter_mark (behind subdiv_step: which scatters select and which place, their instances flagged for the composition)
// and scatter_step (behind the upload of the object table, which would overwrite matrices written earlier, and before
// compose_kernel: the launches of scatter.hip).  The rule itself is scatter_rule.h's, which mpt_scatter_rule evaluates on the host.

#include "miptina_ctx.h"
#include <cstddef>

static_assert(sizeof(mpt_scatter_point) == sizeof(MptScatterPoint) && offsetof(mpt_scatter_point, sy) == offsetof(MptScatterPoint, sy),
              "include/miptina.h and mpt_types.h hold the sticky record alike");

// the parameters as a scatter keeps them: checked, `up` at unit length.  Words of a refusal go to why (always terminated)
static int scatter_params_of(const mpt_scatter_params *in, mpt_scatter_params *out, char *why, size_t why_size) {
    why[0] = 0;
    if (!in) { snprintf(why, why_size, "null parameters"); return 1; }
    *out = *in;
    if (!std::isfinite(in->smin) || !std::isfinite(in->smax)) { snprintf(why, why_size, "the scale range is not finite"); return 1; }
    if (in->smin > in->smax) { snprintf(why, why_size, "the scale range is empty: smin %g above smax %g", in->smin, in->smax); return 1; }
    if (in->align != MPT_SCATTER_ALIGN_NORMAL && in->align != MPT_SCATTER_ALIGN_UP) { snprintf(why, why_size, "align %d outside [0, 1]", in->align); return 1; }
    if (!std::isfinite(in->up[0]) || !std::isfinite(in->up[1]) || !std::isfinite(in->up[2])) { snprintf(why, why_size, "up is not finite"); return 1; }
    mpt_scatter_normalise(in->up, out->up);
    if (!std::isfinite(out->up[0]) || !std::isfinite(out->up[1]) || !std::isfinite(out->up[2])) {
        snprintf(why, why_size, "up (%g, %g, %g) has no direction", in->up[0], in->up[1], in->up[2]);
        return 1;
    }
    out->random_yaw = in->random_yaw != 0;
    return 0;
}

extern "C" int mpt_scatter_rule(const double *corners, const uint32_t *q, int64_t nfaces, const mpt_scatter_params *params, uint64_t seed, int64_t first,
                                int64_t count, mpt_scatter_point *points, double *worlds) {
    mpt_scatter_params par;
    char why[160];
    if (nfaces < 1 || nfaces > MPT_SUBDIV_MAX_FACES || count < 0 || first < 0 || !corners || !q || scatter_params_of(params, &par, why, sizeof why)) return 1;
    std::vector<uint64_t> cdf((size_t)nfaces + 1);
    uint64_t at = 0;
    for (int64_t g = 0; g < nfaces; g++) { cdf[(size_t)g] = at; at += q[g]; }
    cdf[(size_t)nfaces] = at;
    if (at == 0) return 2;
    const uint64_t key = mpt_scatter_mix(seed);
    for (int64_t k = 0; k < count; k++) {
        MptScatterPoint r;
        mpt_scatter_select(cdf.data(), nfaces, key, (uint64_t)(first + k), par.smin, par.smax, par.random_yaw, &r);
        if (points) memcpy(points + k, &r, sizeof r);
        const double *P = corners + (size_t)r.face * 9;
        if (worlds) mpt_scatter_place(P, P + 3, P + 6, r, par.align, par.up, worlds + (size_t)k * 16);
    }
    return 0;
}

// ---------------------------------------------------------------- what scene_compose.cpp tells the table
void scatter_scene_cleared(mpt_ctx *c) {
    auto &sc = c->scatter;
    sc.rows.clear();
    sc.faces_used = sc.points_used = 0;
    sc.space.states_used = 0;
}

// ---------------------------------------------------------------- the scatters
static int check_scatter(const mpt_ctx *c, int id, const char *who) {
    if (id < 0 || (size_t)id >= c->scatter.rows.size()) return fail("%s: unknown scatter %d (%zu scatters)", who, id, c->scatter.rows.size());
    return 0;
}

// the parameters of a scatter over surface object `surf`, checked against the context as well
static int check_params(mpt_ctx *c, const char *who, int surf, const mpt_scatter_params *in, mpt_scatter_params *out) {
    char why[160];
    if (scatter_params_of(in, out, why, sizeof why)) return fail("%s: %s", who, why);
    if (in->density_image < -1 || in->density_image >= c->caps.max_textures)
        return fail("%s: density image %d outside [-1, %d)", who, in->density_image, c->caps.max_textures);
    if (in->density_image < 0) return 0;
    if (in->channel < MPT_DISPLACE_R || in->channel > MPT_DISPLACE_MEAN) return fail("%s: channel %d outside [0, 4]", who, in->channel);
    // the uvs the density is sampled at are means of midpoints of the corner uvs of the surface's mesh: admitted with them
    const int mesh = c->compose.rows[surf].mesh;
    std::vector<float> rec;
    if (fetch_mesh(c, mesh, rec)) return 1;
    if (mpt_displace_uv_check_of(rec.data(), c->compose.meshes[mesh].nfaces, why, sizeof why)) return fail("%s: the surface, object %d of mesh %d: %s", who, surf, mesh, why);
    return 0;
}

extern "C" int mpt_scatter_add(mpt_ctx *c, int surface_obj, int mesh_id, int count, uint64_t seed, int mtlid, const mpt_scatter_params *params,
                               int *scatter_id, int *first_obj) {
    if (use(c)) return 1;
    const char *who = "mpt_scatter_add";
    auto &cp = c->compose;
    auto &sc = c->scatter;
    if (surface_obj < 0 || (size_t)surface_obj >= cp.objs.size()) return fail("%s: unknown surface object %d (%zu objects)", who, surface_obj, cp.objs.size());
    if (check_mesh(c, mesh_id, who)) return 1;
    if (cp.rows[surface_obj].scatter >= 0)
        return fail("%s: the surface, object %d, is itself an instance of scatter %d", who, surface_obj, cp.rows[surface_obj].scatter);
    if (count < 1) return fail("%s: count %d is below 1", who, count);
    if (mtlid < -1 || mtlid >= c->caps.max_materials) return fail("%s: material id %d outside [-1, %d)", who, mtlid, c->caps.max_materials);
    if (cp.meshes[mesh_id].deform.ntargets || cp.meshes[mesh_id].deform.njoints)
        return fail("%s: mesh %d carries morph targets or a skin: a deformable mesh has one copy per object and cannot be instanced", who, mesh_id);
    long long total = 0;
    for (const auto &o : cp.objs) total += o.nfaces;
    const int k = subdiv_object_faces(c, mesh_id);
    if (total + (long long)count * k >= c->caps.max_faces)
        return fail("%s: too many faces: %lld with %d instances of mesh %d, room for fewer than %d", who, total + (long long)count * k, count, mesh_id, c->caps.max_faces);
    mpt_ctx::MptScatterRow row;
    if (check_params(c, who, surface_obj, params, &row.par)) return 1;
    row.surf = surface_obj; row.mesh = mesh_id; row.first_obj = (int)cp.objs.size(); row.count = count; row.seed = seed;
    row.faces = cp.objs[surface_obj].nfaces;
    row.face_at = sc.faces_used; row.point_at = sc.points_used;
    sc.faces_used += (size_t)row.faces + 1; sc.points_used += (size_t)count;
    for (int i = 0; i < count; i++) add_object(c, mesh_id, nullptr, mtlid, (int)sc.rows.size());   // (the host's copy of an instance's matrix is a placeholder)
    sc.rows.push_back(row);
    if (scatter_id) *scatter_id = (int)sc.rows.size() - 1;
    if (first_obj) *first_obj = row.first_obj;
    return 0;
}

extern "C" int mpt_scatter_set_params(mpt_ctx *c, int scatter_id, const mpt_scatter_params *params) {
    if (use(c)) return 1;
    if (check_scatter(c, scatter_id, "mpt_scatter_set_params")) return 1;
    auto &row = c->scatter.rows[scatter_id];
    mpt_scatter_params par;
    if (check_params(c, "mpt_scatter_set_params", row.surf, params, &par)) return 1;
    row.par = par; row.select = true;
    return 0;
}

extern "C" int mpt_scatter_rescatter(mpt_ctx *c, int scatter_id, uint64_t seed) {
    if (use(c)) return 1;
    if (check_scatter(c, scatter_id, "mpt_scatter_rescatter")) return 1;
    c->scatter.rows[scatter_id].seed = seed;
    c->scatter.rows[scatter_id].select = true;
    return 0;
}

extern "C" int mpt_scatter_set_spacing(mpt_ctx *c, int scatter_id, double min_distance, int64_t candidates) {
    if (use(c)) return 1;
    const char *who = "mpt_scatter_set_spacing";
    if (check_scatter(c, scatter_id, who)) return 1;
    auto &row = c->scatter.rows[scatter_id];
    if (!std::isfinite(min_distance) || min_distance < 0.0) return fail("%s: scatter %d: the minimum distance %g is negative or not finite", who, scatter_id, min_distance);
    if (min_distance == 0.0) { row.min_distance = 0.0; row.select = true; return 0; }
    if (candidates < row.count || candidates > MPT_SPACE_MAX_CANDIDATES)
        return fail("%s: scatter %d: %lld candidates outside [%d, %lld], its count and 2^24", who, scatter_id, (long long)candidates, row.count,
                    (long long)MPT_SPACE_MAX_CANDIDATES);
    if (candidates != row.candidates) {       // new room for its states (the old room stays behind until the scene is cleared)
        row.state_at = c->scatter.space.states_used;
        c->scatter.space.states_used += (size_t)candidates;
    }
    row.min_distance = min_distance; row.candidates = candidates; row.select = true;
    return 0;
}

// ---------------------------------------------------------------- the elimination of spaced scatters (scatter_space.hip)
// The rows sj of one elimination: their room in the workspace, the launches, the host's looks.  records: the candidates' records
// (rows of a compose) -- explicit points (rows with job < 0) come from host_pos [sum of m][3] instead.  `compact`: the kept records
// go to points and their candidates to index.  rounds and kept (per row, kept only with compact) and st are what it came to.
static int space_eliminate(mpt_ctx *c, std::vector<MptSpaceJob> &sj, const double *host_pos, const MptScatterPoint *records, MptScatterPoint *points,
                           bool compact, std::vector<int32_t> &rounds, std::vector<int64_t> &kept, mpt_scatter_spacing_info &st) {
    auto &sc = c->scatter;
    auto &sp = sc.space;
    const int n = (int)sj.size();
    std::vector<int32_t> ms((size_t)n);
    size_t cands = 0, buckets = 0, states = sp.states_used;
    int32_t most = 0;
    for (int s = 0; s < n; s++) {
        MptSpaceJob &t = sj[s];
        uint32_t nb = 1;
        while ((int64_t)nb < t.m) nb <<= 1;
        t.mask = nb - 1; t.at = (int64_t)cands; t.bucket_at = (int64_t)buckets;
        t.r2 = t.r * t.r;
        cands += (size_t)t.m; buckets += nb;
        states = std::max(states, (size_t)t.state_at + (size_t)t.m);
        ms[s] = t.m; most = std::max(most, t.m);
    }
    std::vector<MptRun> runs((size_t)n);
    int blocks = 0;
    const int nruns = mpt_run_plan_into(ms.data(), nullptr, n, MPT_SCATTER_CHUNK, runs.data(), &blocks);
    if (nruns != n) return fail("a spaced scatter without candidates");
    if (grow_keeping(sp.state, states, sp.state.cap, c->stream)) return 1;
    if (sp.pos.reserve(cands * 3) || sp.items.reserve(cands) || sp.cursor.reserve(buckets) || sp.start.reserve(buckets) ||
        sp.part.reserve((size_t)blocks * 6) || sp.jobs.reserve((size_t)n) || sp.grids.reserve((size_t)n) || sp.runs.reserve((size_t)n)) return 1;
    if ((size_t)n > sp.words_cap) {
        const size_t cap = std::max((size_t)n, 2 * sp.words_cap);
        if (sp.words.create(2 * cap)) return 1;
        sp.words_cap = cap;
    }
    uint32_t *left = sp.words.host, *kept_word = sp.words.host + sp.words_cap;
    for (int s = 0; s < n; s++) left[s] = kept_word[s] = 0;
    HIP_TRY(hipMemcpyAsync(sp.jobs, sj.data(), (size_t)n * sizeof(MptSpaceJob), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(sp.runs, runs.data(), (size_t)n * sizeof(MptRun), hipMemcpyHostToDevice, c->stream));
    if (host_pos) HIP_TRY(hipMemcpyAsync(sp.pos, host_pos, cands * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(sp.cursor, 0, buckets * sizeof(uint32_t), c->stream));
    HIP_TRY(mpt_launch_space_grid(c->compose.bufs.pool, c->compose.bufs.objs, sc.jobs, sp.jobs, sp.runs, nruns, blocks, records, sp.pos, sp.part, sp.grids,
                                  sp.state, sp.cursor, sp.start, sp.items, c->stream));
    st.grid_launches += 5; sc.launches += 5;
    // the rounds, a batch at a time: the lowest undecided candidate decides in every round, so a scatter takes at most m of them
    unsigned done = 0;
    for (bool waits = true; waits;) {
        if ((int64_t)done >= (int64_t)most + MPT_SPACE_BATCH) return fail("the elimination of a spaced scatter did not settle in %u rounds", done);
        HIP_TRY(mpt_launch_space_rounds(sp.jobs, sp.grids, sp.runs, nruns, blocks, sp.pos, sp.start, sp.cursor, sp.items, sp.state, sp.words.dev, done + 1,
                                        MPT_SPACE_BATCH, c->stream));
        done += MPT_SPACE_BATCH;
        st.round_launches += MPT_SPACE_BATCH; sc.launches += MPT_SPACE_BATCH;
        HIP_TRY(hipStreamSynchronize(c->stream));
        st.host_reads++;
        waits = false;
        for (int s = 0; s < n; s++) waits |= left[s] == done;
    }
    rounds.assign((size_t)n, 0); kept.assign((size_t)n, 0);
    for (int s = 0; s < n; s++) { rounds[s] = (int32_t)left[s] + 1; st.rounds = std::max<int64_t>(st.rounds, rounds[s]); }
    if (!compact) return 0;
    HIP_TRY(mpt_launch_space_compact(sp.jobs, sp.runs, nruns, sp.state, records, points, sp.index, sp.words.dev + sp.words_cap, c->stream));
    st.compact_launches += 1; sc.launches += 1;
    HIP_TRY(hipStreamSynchronize(c->stream));
    st.host_reads++;
    for (int s = 0; s < n; s++) { kept[s] = kept_word[s]; st.kept += kept[s]; }
    return 0;
}

// ---------------------------------------------------------------- the steps of mpt_compose
bool scatter_selection_due(const mpt_ctx *c) {
    for (const auto &r : c->scatter.rows)
        if (r.select) return true;
    return false;
}

int scatter_ready(mpt_ctx *c) {
    const auto &sc = c->scatter;
    for (size_t id = 0; id < sc.rows.size(); id++) {
        const auto &r = sc.rows[id];
        // (an object keeps its face count while it exists -- a mesh with an object takes no subdivision level: should a road to
        // another count open, the scatter has to select again in new room, and says so here until it does)
        if (r.faces != c->compose.objs[r.surf].nfaces)
            return fail("mpt_compose: scatter %zu: its surface, object %d, has %d faces and had %d when the scatter was added", id, r.surf,
                        c->compose.objs[r.surf].nfaces, r.faces);
        if (!r.select) continue;
        if (c->compose.objs[r.surf].nfaces < 1) return fail("mpt_compose: scatter %zu: its surface, object %d, has no faces", id, r.surf);
        const int im = r.par.density_image;
        if (im < 0) continue;
        if ((size_t)im >= c->h_images.size())
            return fail("mpt_compose: the density of scatter %zu reads image %d, and %zu images are loaded", id, im, c->h_images.size());
        if (c->h_images[im].nx < 1 || c->h_images[im].ny < 1)
            return fail("mpt_compose: the density of scatter %zu reads image %d, which is empty (%d x %d)", id, im, c->h_images[im].nx, c->h_images[im].ny);
    }
    return 0;
}

void scatter_mark(mpt_ctx *c) {
    auto &cp = c->compose;
    auto &sc = c->scatter;
    const size_t n = sc.rows.size();
    sc.selects.assign(n, 0); sc.places.assign(n, 0);
    for (size_t id = 0; id < n; id++) {
        auto &r = sc.rows[id];
        sc.selects[id] = r.select;
        bool place = r.select || !r.placed || cp.relayout || (cp.rows[r.surf].dirty & mpt_ctx::MPT_OBJ_COMPOSE);
        // a row of an instance that goes up from the host's table (MPT_OBJ_UPLOAD: its material changed, or the copy of its mesh was
        // displaced again -- mpt_mesh_set_displacement_params, a new image generation in subdiv_step) takes the placeholder
        // matrix with it: its scatter places again
        for (int i = 0; i < r.count && !place; i++) place = (cp.rows[r.first_obj + i].dirty & mpt_ctx::MPT_OBJ_UPLOAD) != 0;
        sc.places[id] = place;
        if (!place) continue;
        r.placed = false;
        for (int i = 0; i < r.count; i++) cp.rows[r.first_obj + i].dirty |= mpt_ctx::MPT_OBJ_PLACED;
    }
}

int scatter_step(mpt_ctx *c) {
    auto &cp = c->compose;
    auto &sc = c->scatter;
    auto &st = sc.stats;
    st.selected_scatters = st.placed_scatters = st.placed_instances = 0;
    st.weight_launches = st.scan_launches = st.select_launches = st.place_launches = st.host_fetches = 0;
    sc.space.stats = mpt_scatter_spacing_info{};
    const int n = (int)sc.rows.size();
    if (n == 0) return 0;
    std::vector<int32_t> faces((size_t)n), counts((size_t)n), sel((size_t)n), plc((size_t)n);
    int nsel = 0, nplc = 0;
    for (int j = 0; j < n; j++) {
        const auto &r = sc.rows[j];
        sel[j] = sc.selects[j]; plc[j] = sc.places[j];
        faces[j] = r.faces; counts[j] = r.count;
        nsel += sel[j]; nplc += plc[j];
    }
    if (nplc == 0) return 0;
    // the spaced scatters that select: the selection makes their candidates, behind the sticky records of all, and the elimination
    // picks the instances from them.  Without one the compose takes the plain path, launch for launch
    std::vector<MptSpaceJob> spaced;
    std::vector<int32_t> drawn(counts);                                   // records the selection makes per scatter
    size_t cands = 0;
    for (int j = 0; j < n; j++) {
        const auto &r = sc.rows[j];
        if (!sel[j] || !(r.min_distance > 0.0)) continue;
        MptSpaceJob t{};
        t.job = j; t.m = (int32_t)r.candidates; t.count = r.count; t.r = r.min_distance;
        t.cand_at = (int64_t)(sc.points_used + cands); t.state_at = (int64_t)r.state_at; t.point_at = (int64_t)r.point_at;
        cands += (size_t)r.candidates;
        drawn[j] = t.m;
        spaced.push_back(t);
    }
    const size_t views = spaced.empty() ? 0 : (size_t)n;                  // the selection's views of the jobs: rows n .. 2 n - 1
    std::vector<MptScatterJob> &jobs = sc.h_jobs;
    jobs.assign((size_t)n + views, MptScatterJob{});
    for (int j = 0; j < n; j++) {
        const auto &r = sc.rows[j];
        MptScatterJob &t = jobs[j];
        t.surf_obj = r.surf; t.first_obj = r.first_obj; t.nfaces = r.faces; t.count = r.count;
        t.face_at = (int64_t)r.face_at; t.point_at = (int64_t)r.point_at;
        t.key = mpt_scatter_mix(r.seed);
        t.align = r.par.align; t.random_yaw = r.par.random_yaw;
        t.smin = r.par.smin; t.smax = r.par.smax;
        for (int k = 0; k < 3; k++) t.up[k] = r.par.up[k];
        if (sel[j] && r.par.density_image >= 0) {
            const MptImage &im = c->h_images[r.par.density_image];        // (loaded: scatter_ready)
            t.density = 1; t.channel = r.par.channel; t.nx = im.nx; t.ny = im.ny; t.texel_at = (int64_t)im.base;
        }
    }
    std::vector<MptRun> &runs = sc.h_runs;
    runs.assign((size_t)3 * (size_t)n, MptRun{});
    int nruns[3] = { 0, 0, 0 }, blocks[3] = { 0, 0, 0 };
    nruns[0] = mpt_run_plan_into(faces.data(), sel.data(), n, MPT_SCATTER_CHUNK, runs.data(), &blocks[0]);
    nruns[1] = mpt_run_plan_into(drawn.data(), sel.data(), n, MPT_SCATTER_CHUNK, runs.data() + (size_t)n, &blocks[1]);
    nruns[2] = mpt_run_plan_into(counts.data(), plc.data(), n, MPT_SCATTER_CHUNK, runs.data() + 2 * (size_t)n, &blocks[2]);
    if (nruns[0] < 0 || nruns[1] < 0 || nruns[2] < 0) return fail("too many faces or instances to scatter");
    if (views) {                                                          // a spaced scatter draws m records into its candidates' room
        for (int j = 0; j < n; j++) jobs[(size_t)n + j] = jobs[j];
        for (const MptSpaceJob &t : spaced) { jobs[(size_t)n + t.job].count = t.m; jobs[(size_t)n + t.job].point_at = t.cand_at; }
        for (int r = 0; r < nruns[1]; r++) runs[(size_t)n + r].item += n;
    }
    // room: the arenas keep what they hold (the records and shares of the scatters that stay as they are)
    if (grow_keeping(sc.w, sc.faces_used, sc.w.cap, c->stream) || grow_keeping(sc.q, sc.faces_used, sc.q.cap, c->stream) ||
        grow_keeping(sc.cdf, sc.faces_used, sc.cdf.cap, c->stream) || grow_keeping(sc.points, sc.points_used + cands, sc.points.cap, c->stream)) return 1;
    if (views && grow_keeping(sc.space.index, sc.points_used, sc.space.index.cap, c->stream)) return 1;
    if (sc.jobs.reserve((size_t)n + views) || sc.runs.reserve((size_t)3 * (size_t)n) || sc.wmax.reserve((size_t)n)) return 1;
    if ((size_t)n > sc.wmax_cap) {
        const size_t cap = std::max((size_t)n, 2 * sc.wmax_cap);
        if (sc.wmax_host.create(cap)) return 1;
        sc.wmax_cap = cap;
    }
    if (sc.part.reserve((size_t)std::max(blocks[0], 1)) || sc.bsum.reserve((size_t)std::max(blocks[0], 1))) return 1;
    HIP_TRY(hipMemcpyAsync(sc.jobs, jobs.data(), jobs.size() * sizeof(MptScatterJob), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(sc.runs, runs.data(), runs.size() * sizeof(MptRun), hipMemcpyHostToDevice, c->stream));
    if (nsel > 0) {
        MptTimedSpan span(sc.select_timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(mpt_launch_scatter_weights(cp.bufs.pool, cp.bufs.objs, sc.jobs, sc.runs, nruns[0], blocks[0], c->texels, sc.w, sc.part, sc.wmax,
                                           sc.wmax_host.dev, c->stream));
        st.weight_launches = 1; sc.launches += 2;
        // the one place a compose with scatters waits for the device: a surface without weight is refused before its shares are made
        HIP_TRY(hipStreamSynchronize(c->stream));
        st.host_fetches = 1;
        for (int j = 0; j < n; j++)
            if (sel[j] && !(sc.wmax_host.host[j] > 0.0))
                return fail("mpt_compose: scatter %d: its surface, object %d, has no face with a weight above 0 (area times density)", j, sc.rows[j].surf);
        HIP_TRY(mpt_launch_scatter_scan(sc.jobs, sc.runs, nruns[0], blocks[0], sc.w, sc.wmax, sc.q, sc.cdf, sc.bsum, c->stream));
        st.scan_launches = 3; sc.launches += 3;
        HIP_TRY(mpt_launch_scatter_select(sc.jobs, sc.runs + (size_t)n, nruns[1], blocks[1], sc.cdf, sc.points, c->stream));
        st.select_launches = 1; sc.launches += 1;
        if (!spaced.empty()) {
            auto &ss = sc.space.stats;
            std::vector<int32_t> rounds;
            std::vector<int64_t> kept;
            ss.scatters = (int64_t)spaced.size(); ss.candidates = (int64_t)cands;
            MptTimedSpan inner(sc.space_timer, c->stream);
            HIP_TRY(inner.begun);
            const int rc = space_eliminate(c, spaced, nullptr, sc.points, sc.points, true, rounds, kept, ss);
            st.host_fetches += ss.host_reads;
            if (rc) return 1;
            HIP_TRY(inner.end());
            for (size_t s = 0; s < spaced.size(); s++) {
                auto &r = sc.rows[spaced[s].job];
                r.kept = kept[s]; r.rounds = rounds[s];
                if (kept[s] < r.count)
                    return fail("mpt_compose: scatter %d: %lld of its %lld candidates are kept at the minimum distance %g, fewer than its count %d", spaced[s].job,
                                (long long)kept[s], (long long)r.candidates, r.min_distance, r.count);
            }
        }
        HIP_TRY(span.end());
    }
    {
        MptTimedSpan span(sc.place_timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(mpt_launch_scatter_place(cp.bufs.pool, cp.bufs.objs, sc.jobs, sc.runs + 2 * (size_t)n, nruns[2], blocks[2], sc.points, cp.epoch, c->stream));
        st.place_launches = 1; sc.launches += 1;
        HIP_TRY(span.end());
    }
    for (int j = 0; j < n; j++) {
        auto &r = sc.rows[j];
        if (sel[j]) { r.select = false; st.selected_scatters++; }
        if (plc[j]) { r.placed = true; st.placed_scatters++; st.placed_instances += r.count; }
    }
    return 0;
}

// ---------------------------------------------------------------- read-backs
extern "C" int mpt_scatter_stats(mpt_ctx *c, mpt_scatter_info *out) {
    if (!c || !out) return fail("null argument");
    *out = c->scatter.stats;
    out->scatters = (int64_t)c->scatter.rows.size();
    out->instances = 0;
    for (const auto &r : c->scatter.rows) out->instances += r.count;
    return 0;
}

extern "C" int mpt_scatter_kernel_time(mpt_ctx *c, double *select_ms, double *place_ms, int *launches) {
    if (use_ro(c)) return 1;
    auto &sc = c->scatter;
    double seg[2] = { 0, 0 };
    if (timer_readout(c, sc.select_timer, &seg[0], nullptr, nullptr) || timer_readout(c, sc.place_timer, &seg[1], nullptr, nullptr)) return 1;
    if (select_ms) *select_ms = seg[0];
    if (place_ms) *place_ms = seg[1];
    if (launches) *launches = sc.launches;
    sc.launches = 0;
    return 0;
}

extern "C" int mpt_scatter_get(mpt_ctx *c, int scatter_id, mpt_scatter_point *points, double *worlds, uint32_t *q) {
    if (use_ro(c)) return 1;
    if (check_scatter(c, scatter_id, "mpt_scatter_get")) return 1;
    const auto &sc = c->scatter;
    const auto &r = sc.rows[scatter_id];
    if (!r.placed || r.select) return fail("mpt_scatter_get: scatter %d has not been placed yet: call mpt_compose", scatter_id);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (points) HIP_TRY(hipMemcpy(points, sc.points + r.point_at, (size_t)r.count * sizeof(MptScatterPoint), hipMemcpyDeviceToHost));
    if (worlds)
        HIP_TRY(hipMemcpy2D(worlds, 16 * sizeof(double), (const char *)(c->compose.bufs.objs + r.first_obj) + offsetof(MptComposeObj, world), sizeof(MptComposeObj),
                            16 * sizeof(double), (size_t)r.count, hipMemcpyDeviceToHost));
    if (q) HIP_TRY(hipMemcpy(q, sc.q + r.face_at, (size_t)r.faces * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mpt_scatter_spacing_stats(mpt_ctx *c, mpt_scatter_spacing_info *out) {
    if (!c || !out) return fail("null argument");
    *out = c->scatter.space.stats;
    return 0;
}

extern "C" int mpt_scatter_spacing_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->scatter.space_timer, ms, nullptr, launches);
}

extern "C" int mpt_scatter_get_spacing(mpt_ctx *c, int scatter_id, int64_t *candidates, int64_t *kept, int32_t *rounds, uint8_t *kept_flags, int64_t *index) {
    if (use_ro(c)) return 1;
    const char *who = "mpt_scatter_get_spacing";
    if (check_scatter(c, scatter_id, who)) return 1;
    const auto &sc = c->scatter;
    const auto &r = sc.rows[scatter_id];
    if (!(r.min_distance > 0.0)) return fail("%s: scatter %d is a plain scatter: it has no minimum distance", who, scatter_id);
    if (!r.placed || r.select) return fail("%s: scatter %d has not been placed yet: call mpt_compose", who, scatter_id);
    if (candidates) *candidates = r.candidates;
    if (kept) *kept = r.kept;
    if (rounds) *rounds = r.rounds;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int32_t> tmp((size_t)std::max<int64_t>(r.candidates, r.count));
    if (kept_flags) {
        HIP_TRY(hipMemcpy(tmp.data(), sc.space.state + r.state_at, (size_t)r.candidates * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < r.candidates; j++) kept_flags[j] = tmp[(size_t)j] == MPT_SPACE_KEPT;
    }
    if (index) {
        HIP_TRY(hipMemcpy(tmp.data(), sc.space.index + r.point_at, (size_t)r.count * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < r.count; i++) index[i] = tmp[(size_t)i];
    }
    return 0;
}

static int space_rule_args(const double *points, int64_t n, double r) { return n < 0 || (n > 0 && !points) || !(r >= 0.0); }

extern "C" int mpt_scatter_space_rule(const double *points, int64_t n, double r, uint8_t *kept, int32_t *rounds) {
    if (space_rule_args(points, n, r)) return 1;
    std::vector<uint8_t> flags((size_t)n);
    std::vector<int32_t> t((size_t)n);
    const int32_t took = mpt_scatter_space_of(points, n, r, flags.data(), t.data());
    if (kept && n > 0) memcpy(kept, flags.data(), (size_t)n);
    if (rounds) *rounds = took;
    return 0;
}

extern "C" int mpt_scatter_space_points(mpt_ctx *c, const double *points, int64_t n, double r, uint8_t *kept, int32_t *rounds) {
    if (use_ro(c)) return 1;
    const char *who = "mpt_scatter_space_points";
    if (space_rule_args(points, n, r) || n > MPT_SPACE_MAX_CANDIDATES)
        return fail("%s: bad arguments: %lld points (%s; at most 2^24) at the distance %g", who, (long long)n, points ? "given" : "null", r);
    if (rounds) *rounds = 0;
    if (n == 0) return 0;
    auto &sc = c->scatter;
    std::vector<MptSpaceJob> sj(1);
    sj[0].job = -1; sj[0].m = (int32_t)n; sj[0].r = r; sj[0].state_at = (int64_t)sc.space.states_used;   // behind the states that scatters own
    std::vector<int32_t> took;
    std::vector<int64_t> none;
    mpt_scatter_spacing_info st{};
    const int launched = sc.launches;
    const int rc = space_eliminate(c, sj, points, nullptr, nullptr, false, took, none, st);
    sc.launches = launched;                                               // (mpt_scatter_kernel_time counts the composes' kernels)
    if (rc) return 1;
    if (rounds) *rounds = took[0];
    if (!kept) return 0;
    std::vector<int32_t> state((size_t)n);
    HIP_TRY(hipMemcpy(state.data(), sc.space.state + sj[0].state_at, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < n; j++) kept[j] = state[(size_t)j] == MPT_SPACE_KEPT;
    return 0;
}

// scene_subdiv.cpp -- Loop subdivision behind mpt_mesh_set_subdivision: the meshes' topology blocks on the
// device (subdiv_rule.h makes them, a pure function), the table of subdivided copies beside scene_compose.cpp's object table and
// scene_deform.cpp's poses, the run tables of a compose's launches (mpt_subdiv_plan: run_table.h's rule), and subdiv_step: the part of
// mpt_compose behind deform_step that gives the copies their room in the pool and launches subdiv.hip before compose_kernel.
// A Catmull-Clark mesh (mpt_mesh_set_subdivision_cc) is a row of the same tables and a job of the same
// launches: its block has other rules in it, its job names the table of level-1 quads, and its objects have another face count.
// Texture displacement of the copies lives here too: mpt_mesh_set_displacement and its first-corner table
// (displace_rule.h makes it, a pure function), and displace.hip's launch inside subdiv_step, between the last refine level and the
// normals.

#include "miptina_ctx.h"

extern "C" int mpt_subdiv_plan(const int32_t *items, const int32_t *dirty, int njobs, int32_t *run_job, int64_t *run_block, int cap, int64_t *blocks) {
    return mpt_run_plan_of(items, dirty, njobs, MPT_SUBDIV_CHUNK, run_job, run_block, cap, blocks);
}

// what the topology entry points hand back of an accepted mesh (offsets: 9 words, 11 with the records' rules and number, 12 with the table of level-1 quads)
static int topology_out(const MptSubdivTopo &t, int levels, int64_t *counts, int32_t *offsets, int noffsets, int32_t *words, int64_t cap_words, int64_t *need_words) {
    if (counts)
        for (int l = 0; l <= levels; l++) { counts[3 * l] = t.nv[l]; counts[3 * l + 1] = t.ne[l]; counts[3 * l + 2] = t.nf[l]; }
    if (offsets) {
        for (int l = 0; l <= MPT_SUBDIV_MAX_LEVELS; l++) offsets[l] = l <= levels ? t.rule_at[l] : 0;
        offsets[6] = t.nrule_at; offsets[7] = t.face_at; offsets[8] = (int32_t)t.words.size();
        if (noffsets > 9) { offsets[9] = t.srule_at; offsets[10] = (int32_t)t.nrec; }
        if (noffsets > 11) offsets[11] = t.quad_at;
    }
    if (need_words) *need_words = (int64_t)t.words.size();
    if (words && cap_words >= (int64_t)t.words.size()) memcpy(words, t.words.data(), t.words.size() * sizeof(int32_t));
    return 0;
}

extern "C" int mpt_subdiv_topology(const float *verts, int k, int levels, int64_t *counts, int32_t *offsets, int32_t *words, int64_t cap_words,
                                   int64_t *need_words, char *why, int why_size) {
    MptSubdivTopo t;
    const MptSubdivVerdict v = mpt_subdiv_topology_of(verts, k, levels, t, why, why_size > 0 ? (size_t)why_size : 0);
    if (v != MPT_SUBDIV_OK) return (int)v;
    return topology_out(t, levels, counts, offsets, 9, words, cap_words, need_words);
}

extern "C" int mpt_subdiv_topology_cc(const float *verts, int k, int levels, const int32_t *polys, int m, const float *crease, const uint8_t *corner,
                                      int64_t *counts, int32_t *offsets, int32_t *words, int64_t cap_words, int64_t *need_words, char *why, int why_size) {
    MptSubdivTopoCC t;
    const MptSubdivVerdict v = mpt_subdiv_topology_cc_of(verts, k, levels, polys, m, crease, corner, t, why, why_size > 0 ? (size_t)why_size : 0);
    if (v != MPT_SUBDIV_OK) return (int)v;
    return topology_out(t, levels, counts, offsets, 12, words, cap_words, need_words);
}

extern "C" int mpt_subdiv_topology_creased(const float *verts, int k, int levels, const float *crease, const uint8_t *corner, int64_t *counts, int32_t *offsets,
                                           int32_t *words, int64_t cap_words, int64_t *need_words, char *why, int why_size) {
    MptSubdivTopo t;
    const MptSubdivVerdict v = mpt_subdiv_topology_creased_of(verts, k, levels, crease, corner, t, why, why_size > 0 ? (size_t)why_size : 0);
    if (v != MPT_SUBDIV_OK) return (int)v;
    return topology_out(t, levels, counts, offsets, 11, words, cap_words, need_words);
}

// ---------------------------------------------------------------- what scene_compose.cpp and scene_deform.cpp tell the table
int subdiv_object_faces(const mpt_ctx *c, int mesh_id) {
    const auto &m = c->compose.meshes[mesh_id];
    return m.subdiv.head.levels ? (int)m.subdiv.out_faces : m.nfaces;
}

void subdiv_object_added(mpt_ctx *c, int obj_id) {
    auto &sd = c->subdiv;
    auto &row = c->compose.rows[obj_id];
    auto &m = c->compose.meshes[row.mesh].subdiv;
    if (m.head.levels == 0) return;
    const bool deformable = row.pose >= 0;
    if (deformable || m.job < 0) {
        mpt_ctx::MptSubdivCopy p;
        p.mesh = row.mesh; p.obj = deformable ? obj_id : -1;
        sd.copies.push_back(p);
        if (!deformable) m.job = (int)sd.copies.size() - 1;
    }
    row.copy = deformable ? (int)sd.copies.size() - 1 : m.job;
    sd.room.stale = true;
}

void subdiv_pose_changed(mpt_ctx *c, int obj_id) {
    const int copy = c->compose.rows[obj_id].copy;
    if (copy >= 0) c->subdiv.copies[copy].dirty = true;
}

void subdiv_scene_cleared(mpt_ctx *c, int meshes) {
    auto &sd = c->subdiv;
    sd.copies.clear();
    for (auto &m : c->compose.meshes) m.subdiv.job = -1;
    sd.room.copy_verts = 0; sd.room.stale = true;
    if (meshes) sd.topo_used = 0;
}

// ---------------------------------------------------------------- the meshes' levels
// crease [k][3] and corner [k][3] of the mesh's faces, either may be null.  cc: Catmull-Clark over the m
// polygons polys (null: the triangles), crease and corner then flat over the polygons' corners (section 3.19.2)
static int set_subdivision(mpt_ctx *c, const char *who, int mesh_id, int levels, const float *crease, const uint8_t *corner, bool cc = false,
                           const int32_t *polys = nullptr, int npolys = 0) {
    if (use(c)) return 1;
    auto &sd = c->subdiv;
    auto &cp = c->compose;
    if (check_fresh_mesh(c, mesh_id, who)) return 1;
    auto &m = cp.meshes[mesh_id].subdiv;
    if (m.head.levels) return fail("%s: mesh %d already has a subdivision level", who, mesh_id);
    if (levels < 1 || levels > MPT_SUBDIV_MAX_LEVELS) return fail("%s: levels %d outside [1, %d]", who, levels, MPT_SUBDIV_MAX_LEVELS);
    const int k = cp.meshes[mesh_id].nfaces;
    // the faces an object of the mesh will have: k 4^L, or of m polygons of n_j corners 2 (sum n_j) 4^(L - 1)
    long long out_faces = (long long)k << (2 * levels);
    if (cc) {
        long long corners = 3LL * k;
        if (polys) { corners = 0; for (int j = 0; j < npolys; j++) corners += std::max(polys[j], 0); }
        out_faces = (2 * corners) << (2 * (levels - 1));
    }
    if (out_faces >= c->caps.max_faces) return fail("%s: too many faces: %lld at level %d", who, out_faces, levels);
    std::vector<float> rec;
    if (fetch_mesh(c, mesh_id, rec)) return 1;
    MptSubdivTopoCC t;
    char why[200];
    const MptSubdivVerdict verdict = cc ? mpt_subdiv_topology_cc_of(rec.data(), k, levels, polys, npolys, crease, corner, t, why, sizeof why)
                                        : mpt_subdiv_topology_creased_of(rec.data(), k, levels, crease, corner, t, why, sizeof why);
    if (verdict != MPT_SUBDIV_OK) return fail("%s: mesh %d: %s", who, mesh_id, why);
    const size_t words = t.words.size();
    if (grow_keeping(sd.bufs.topo, sd.topo_used + words, sd.topo_used, c->stream)) return 1;
    if (words > 0) {
        HIP_TRY(hipMemcpyAsync(sd.bufs.topo + sd.topo_used, t.words.data(), words * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    m.head = t;
    if (!t.srule_at) m.head.srule_at = t.nrule_at;       // (an uncreased mesh: the records' rules are the rings')
    m.topo_at = sd.topo_used; m.job = -1;
    m.out_faces = cc ? 2 * t.nf[levels] : t.nf[levels];
    sd.topo_used += words;
    return 0;
}

extern "C" int mpt_mesh_set_subdivision(mpt_ctx *c, int mesh_id, int levels) {
    return set_subdivision(c, "mpt_mesh_set_subdivision", mesh_id, levels, nullptr, nullptr);
}

extern "C" int mpt_mesh_set_subdivision_creased(mpt_ctx *c, int mesh_id, int levels, const float *crease, const uint8_t *corner) {
    return set_subdivision(c, "mpt_mesh_set_subdivision_creased", mesh_id, levels, crease, corner);
}

extern "C" int mpt_mesh_set_subdivision_cc(mpt_ctx *c, int mesh_id, int levels, const int32_t *polys, int m, const float *crease, const uint8_t *corner) {
    return set_subdivision(c, "mpt_mesh_set_subdivision_cc", mesh_id, levels, crease, corner, true, polys, m);
}

// ---------------------------------------------------------------- the meshes' displacements
extern "C" int mpt_displace_corners(const int32_t *faces, int64_t nfaces, int32_t nverts, int32_t *corner) {
    return mpt_displace_corners_of(faces, nfaces, nverts, corner);
}

static int check_displace_params(const char *who, double strength, double midlevel) {
    if (!std::isfinite(strength)) return fail("%s: strength is not finite", who);
    if (!std::isfinite(midlevel)) return fail("%s: midlevel is not finite", who);
    return 0;
}

extern "C" int mpt_mesh_set_displacement(mpt_ctx *c, int mesh_id, int image_id, int mode, int channel, double strength, double midlevel) {
    if (use(c)) return 1;
    const char *who = "mpt_mesh_set_displacement";
    auto &sd = c->subdiv;
    auto &cp = c->compose;
    if (check_mesh(c, mesh_id, who)) return 1;
    auto &m = cp.meshes[mesh_id].subdiv;
    if (m.head.levels == 0) return fail("%s: displacement needs a subdivided mesh: mesh %d has no subdivision level", who, mesh_id);
    if (check_fresh_mesh(c, mesh_id, who)) return 1;
    if (m.displaced) return fail("%s: mesh %d already has a displacement", who, mesh_id);
    if (mode != MPT_DISPLACE_NORMAL && mode != MPT_DISPLACE_VECTOR) return fail("%s: mode %d outside [0, 1]", who, mode);
    if (channel < MPT_DISPLACE_R || channel > MPT_DISPLACE_MEAN) return fail("%s: channel %d outside [0, 4]", who, channel);
    if (image_id < 0) return fail("%s: image id %d is negative", who, image_id);
    if (check_displace_params(who, strength, midlevel)) return 1;
    const int k = cp.meshes[mesh_id].nfaces;
    const int64_t nf = m.out_faces, nv = m.head.nv[m.head.levels];
    std::vector<float> rec;
    std::vector<int32_t> faces((size_t)nf * 3), corner((size_t)nv);
    if (fetch_mesh(c, mesh_id, rec)) return 1;
    if (k > 0) HIP_TRY(hipMemcpy(faces.data(), sd.bufs.topo + m.topo_at + (size_t)m.head.face_at, faces.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    char why[200];
    if (mpt_displace_uv_check_of(rec.data(), k, why, sizeof why)) return fail("%s: mesh %d: %s", who, mesh_id, why);
    if (m.head.srule_at != m.head.nrule_at && nf > 0) {  // a creased mesh's face table indexes records: back to their vertices
        std::vector<int32_t> vert((size_t)m.head.nrec);
        HIP_TRY(hipMemcpy(vert.data(), sd.bufs.topo + m.topo_at + (size_t)m.head.srule_at + (size_t)m.head.nrec * 2, vert.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (auto &f : faces) f = vert[(size_t)f];
    }
    if (mpt_displace_corners_of(faces.data(), nf, (int32_t)nv, corner.data())) return fail("%s: mesh %d: its topology names no first corner for every vertex", who, mesh_id);
    if (grow_keeping(sd.bufs.topo, sd.topo_used + corner.size(), sd.topo_used, c->stream)) return 1;
    if (nv > 0) {
        HIP_TRY(hipMemcpyAsync(sd.bufs.topo + sd.topo_used, corner.data(), corner.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    m.displaced = true; m.image = image_id; m.mode = mode; m.channel = channel; m.strength = strength; m.midlevel = midlevel;
    m.corner_at = sd.topo_used;
    sd.topo_used += corner.size();
    return 0;
}

extern "C" int mpt_mesh_set_displacement_params(mpt_ctx *c, int mesh_id, double strength, double midlevel) {
    if (use(c)) return 1;
    const char *who = "mpt_mesh_set_displacement_params";
    if (check_mesh(c, mesh_id, who)) return 1;
    auto &m = c->compose.meshes[mesh_id].subdiv;
    if (!m.displaced) return fail("%s: mesh %d has no displacement", who, mesh_id);
    if (check_displace_params(who, strength, midlevel)) return 1;
    m.strength = strength; m.midlevel = midlevel;
    // every copy of the mesh is displaced again, and every object that reads one is composed again (a rigid mesh's share one copy)
    for (auto &row : c->compose.rows) {
        if (row.copy < 0 || row.mesh != mesh_id) continue;
        c->subdiv.copies[row.copy].dirty = true;
        row.dirty = mpt_ctx::MPT_OBJ_UPLOAD;
    }
    return 0;
}

// ---------------------------------------------------------------- the step of mpt_compose
// the doubles of a copy's workspace: the positions of levels 1..L (each level from an even offset), then the last level's records,
// one per vertex or, of a creased mesh, per sector, then -- a displaced copy -- the displaced positions of the last level
static size_t work_layout(const mpt_ctx::MptSubdivMesh &m, MptSubdivJob *job) {
    const MptSubdivHead &h = m.head;
    size_t at = 0;
    for (int l = 1; l <= h.levels; l++) {
        if (job) job->pos_at[l] = (int32_t)at;
        at += ((size_t)h.nv[l] * 3 + 1) & ~(size_t)1;
    }
    if (job) job->vrec_at = (int32_t)at;
    at += (size_t)h.nrec * 4;
    if (job) job->npos_at = job->pos_at[h.levels];
    if (!m.displaced) return at;
    if (job) job->pos_at[0] = job->npos_at = (int32_t)at;
    return at + (((size_t)h.nv[h.levels] * 3 + 1) & ~(size_t)1);
}

// the part of a job that is the block's header (a mesh's row keeps it normalised: set_subdivision)
static void job_head(const MptSubdivHead &h, MptSubdivJob &t) {
    t.levels = h.levels;
    for (int l = 0; l <= h.levels; l++) { t.nv[l] = (int32_t)h.nv[l]; t.rule_at[l] = h.rule_at[l]; }
    t.nrule_at = h.nrule_at; t.face_at = h.face_at;
    t.srule_at = h.srule_at; t.nrec = (int32_t)h.nrec;
    t.rule_at[0] = h.quad_at;                             // (the record has no word to spare: MptSubdivJob)
}

// does the next subdiv_step write this copy?  (`all`: a relayout writes every copy)
static bool copy_is_dirty(const mpt_ctx *c, const mpt_ctx::MptSubdivCopy &p, bool all) {
    return all || p.dirty || (c->compose.meshes[p.mesh].subdiv.displaced && p.image_gen != c->image_gen);
}

// The first thing mpt_compose asks, before anything is queued or changed: the image of every displaced copy that the step below
// will write is loaded.  (A copy it will not write was displaced at this image generation: its image is there.)
int subdiv_images_ready(mpt_ctx *c) {
    const auto &sd = c->subdiv;
    const bool all = c->compose.relayout || sd.room.stale || c->deform.room.stale;
    for (const auto &p : sd.copies) {
        const auto &m = c->compose.meshes[p.mesh].subdiv;
        if (!m.displaced || m.head.nv[m.head.levels] == 0 || !copy_is_dirty(c, p, all)) continue;
        if ((size_t)m.image >= c->h_images.size())
            return fail("mpt_compose: the displacement of mesh %d reads image %d, and %zu images are loaded", p.mesh, m.image, c->h_images.size());
        const MptImage &im = c->h_images[m.image];
        if (im.nx < 1 || im.ny < 1) return fail("mpt_compose: the displacement of mesh %d reads image %d, which is empty (%d x %d)", p.mesh, m.image, im.nx, im.ny);
    }
    return 0;
}

// Called with deform_step's launch (if any) queued.  At a relayout (objects added or dropped, or the copies lost their room) the
// copies are laid out behind the meshes and the deformed copies, the pool grows to hold them, the objects' mesh_vert is pointed at
// them -- mpt_compose then uploads the whole table -- and every copy is subdivided; else the copies of the objects whose pose
// changed.  Nothing here waits for the device, except a pool that has to grow.
int subdiv_step(mpt_ctx *c) {
    auto &cp = c->compose;
    auto &sd = c->subdiv;
    auto &df = c->deform;
    sd.stats.refined_copies = sd.stats.refined_faces = 0;
    sd.displaced_copies = sd.displaced_verts = 0;
    const int n = (int)sd.copies.size();
    if (n == 0) { sd.stats.copy_verts = 0; return 0; }
    const bool all = cp.relayout || sd.room.stale;
    if (all) {
        // (behind the deformed copies, which the pool keeps as it grows: a pool that grows here waits for the deform launch)
        const size_t base = cp.pool_verts + df.room.copy_verts;
        if (lay_copies(c, sd.room, sd.copies, base, [&](const auto &p) { return (size_t)subdiv_object_faces(c, p.mesh) * 3; }, "subdivided")) return 1;
        size_t work = 0;
        for (auto &p : sd.copies) {
            p.work_at = work;
            work += work_layout(cp.meshes[p.mesh].subdiv, nullptr);
        }
        if (sd.bufs.work.reserve(std::max(work, (size_t)2)) || sd.bufs.reserve_tables((size_t)n)) return 1;
        for (size_t o = 0; o < cp.rows.size(); o++)
            if (cp.rows[o].copy >= 0) cp.objs[o].mesh_vert = (int32_t)sd.copies[cp.rows[o].copy].copy_vert;
        sd.room.stale = false;
    }
    sd.stats.copy_verts = (int64_t)sd.room.copy_verts;
    std::vector<MptSubdivJob> &jobs = sd.h_jobs;
    jobs.assign((size_t)n, MptSubdivJob{});
    std::vector<MptDisplaceJob> &djobs = sd.h_djobs;
    djobs.assign((size_t)n, MptDisplaceJob{});
    std::vector<int32_t> dirty((size_t)n), displace((size_t)n);
    int lmax = 0, ndirty = 0, ndisplaced = 0, any_cc = 0;                // (any_cc: a dirty copy is of a Catmull-Clark mesh)
    for (int j = 0; j < n; j++) {
        const auto &p = sd.copies[j];
        const auto &m = c->compose.meshes[p.mesh].subdiv;
        MptSubdivJob &t = jobs[j];
        t.src_vert = p.obj >= 0 ? (int32_t)df.poses[cp.rows[p.obj].pose].copy_vert : (int32_t)cp.meshes[p.mesh].vert;
        t.dst_vert = (int32_t)p.copy_vert;
        t.nfaces = subdiv_object_faces(c, p.mesh);
        t.topo_at = (int64_t)m.topo_at; t.work_at = (int64_t)p.work_at;
        job_head(m.head, t);
        work_layout(m, &t);
        dirty[j] = copy_is_dirty(c, p, all);
        if (!dirty[j] || t.nfaces == 0) continue;
        ndirty++; lmax = std::max(lmax, m.head.levels); any_cc |= m.head.quad_at != 0;
        sd.stats.refined_copies++; sd.stats.refined_faces += t.nfaces;
        if (!m.displaced) continue;
        const MptImage &im = c->h_images[m.image];            // (loaded: subdiv_images_ready)
        djobs[j] = { m.mode, m.channel, im.nx, im.ny, (int64_t)im.base, (int64_t)m.corner_at, m.strength, m.midlevel };
        displace[j] = 1; ndisplaced++;
        sd.displaced_copies++; sd.displaced_verts += t.nv[m.head.levels];
    }
    // a copy displaced again because the images changed: the objects that read it are composed again
    for (auto &row : cp.rows)
        if (row.copy >= 0 && displace[row.copy]) row.dirty = mpt_ctx::MPT_OBJ_UPLOAD;
    for (int j = 0; j < n; j++) {
        sd.copies[j].dirty = false;
        if (displace[j]) sd.copies[j].image_gen = c->image_gen;
    }
    if (ndirty == 0) return 0;
    // the run tables: launch t = 0 .. lmax - 1 refines to level t + 1, then the normals, then the records; behind them the
    // displacement's, over the displaced copies among the dirty ones (it is launched between the last refine level and the normals)
    const int ntables = lmax + 2 + (ndisplaced ? 1 : 0);
    std::vector<MptRun> &runs = sd.h_runs;
    runs.assign((size_t)ntables * (size_t)n, MptRun{});
    std::vector<int> nruns((size_t)ntables), blocks((size_t)ntables);
    std::vector<int32_t> items((size_t)n);
    for (int t = 0; t < ntables; t++) {
        for (int j = 0; j < n; j++)
            items[j] = t < lmax ? (jobs[j].levels > t ? jobs[j].nv[t + 1] : 0) : t == lmax ? jobs[j].nrec : t == lmax + 1 ? jobs[j].nfaces
                     : displace[j] ? jobs[j].nv[jobs[j].levels] : 0;
        nruns[t] = mpt_run_plan_into(items.data(), dirty.data(), n, MPT_SUBDIV_CHUNK, runs.data() + (size_t)t * (size_t)n, &blocks[t]);
        if (nruns[t] < 0) return fail("too many faces to subdivide");
    }
    HIP_TRY(hipMemcpyAsync(sd.bufs.jobs, jobs.data(), (size_t)n * sizeof(MptSubdivJob), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(sd.bufs.runs, runs.data(), runs.size() * sizeof(MptRun), hipMemcpyHostToDevice, c->stream));
    if (ndisplaced) HIP_TRY(hipMemcpyAsync(sd.bufs.djobs, djobs.data(), (size_t)n * sizeof(MptDisplaceJob), hipMemcpyHostToDevice, c->stream));
    {
        MptTimedSpan span(sd.refine_timer, c->stream);
        HIP_TRY(span.begun);
        for (int t = 0; t < lmax; t++) {
            HIP_TRY(mpt_launch_subdiv_refine(cp.bufs.pool, sd.bufs.jobs, sd.bufs.runs + (size_t)t * (size_t)n, nruns[t], blocks[t], t + 1, any_cc, sd.bufs.topo,
                                             sd.bufs.work, c->stream));
            sd.launches++;
        }
        HIP_TRY(span.end());
    }
    if (ndisplaced && nruns[lmax + 2] > 0) {
        MptTimedSpan span(sd.displace_timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(mpt_launch_displace(cp.bufs.pool, sd.bufs.jobs, sd.bufs.djobs, sd.bufs.runs + (size_t)(lmax + 2) * (size_t)n, nruns[lmax + 2], blocks[lmax + 2],
                                    sd.bufs.topo, c->texels, sd.bufs.work, c->stream));
        sd.displace_launches++;
        HIP_TRY(span.end());
    }
    {
        MptTimedSpan span(sd.normal_timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(mpt_launch_subdiv_normals(sd.bufs.jobs, sd.bufs.runs + (size_t)lmax * (size_t)n, nruns[lmax], blocks[lmax], sd.bufs.topo, sd.bufs.work,
                                          c->stream));
        sd.launches++;
        HIP_TRY(span.end());
    }
    {
        MptTimedSpan span(sd.emit_timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(mpt_launch_subdiv_emit(cp.bufs.pool, sd.bufs.jobs, sd.bufs.runs + (size_t)(lmax + 1) * (size_t)n, nruns[lmax + 1], blocks[lmax + 1],
                                       sd.bufs.topo, sd.bufs.work, c->stream));
        sd.launches++;
        HIP_TRY(span.end());
    }
    return 0;
}

// ---------------------------------------------------------------- read-backs
extern "C" int mpt_get_subdivided(mpt_ctx *c, int obj_id, float *verts, int cap_faces) {
    if (use_ro(c)) return 1;
    auto &sd = c->subdiv;
    if (check_object(c, obj_id, "mpt_get_subdivided")) return 1;
    const int copy = c->compose.rows[obj_id].copy;
    if (copy < 0) return fail("mpt_get_subdivided: the mesh of object %d has no subdivision level", obj_id);
    const auto &p = sd.copies[copy];
    const int k = subdiv_object_faces(c, p.mesh);
    return read_copy(c, p.copy_vert, sd.room.stale, k, obj_id, verts, cap_faces, "mpt_get_subdivided", "subdivided", "subdivided mesh");
}

extern "C" int mpt_subdiv_stats(mpt_ctx *c, mpt_subdiv_info *out) {
    if (!c || !out) return fail("null argument");
    *out = c->subdiv.stats;
    out->subdivided_objects = 0;
    for (const auto &row : c->compose.rows) out->subdivided_objects += row.copy >= 0;
    out->copies = (int64_t)c->subdiv.copies.size();
    out->copy_verts = (int64_t)c->subdiv.room.copy_verts;
    return 0;
}

extern "C" int mpt_subdiv_kernel_time(mpt_ctx *c, double *refine_ms, double *normals_ms, double *records_ms, int *launches) {
    if (use_ro(c)) return 1;
    auto &sd = c->subdiv;
    double seg[3] = { 0, 0, 0 };
    if (timer_readout(c, sd.refine_timer, &seg[0], nullptr, nullptr) || timer_readout(c, sd.normal_timer, &seg[1], nullptr, nullptr) ||
        timer_readout(c, sd.emit_timer, &seg[2], nullptr, nullptr)) return 1;
    if (refine_ms) *refine_ms = seg[0];
    if (normals_ms) *normals_ms = seg[1];
    if (records_ms) *records_ms = seg[2];
    if (launches) *launches = sd.launches;
    sd.launches = 0;
    return 0;
}

extern "C" int mpt_displace_stats(mpt_ctx *c, mpt_displace_info *out) {
    if (!c || !out) return fail("null argument");
    const auto &sd = c->subdiv;
    *out = mpt_displace_info{};
    for (const auto &m : c->compose.meshes) out->displaced_meshes += m.subdiv.displaced;
    for (const auto &p : sd.copies) out->copies += c->compose.meshes[p.mesh].subdiv.displaced;
    out->displaced_copies = sd.displaced_copies;
    out->displaced_verts = sd.displaced_verts;
    out->image_generation = (int64_t)c->image_gen;
    return 0;
}

extern "C" int mpt_displace_kernel_time(mpt_ctx *c, double *displace_ms, int *launches) {
    if (use_ro(c)) return 1;
    auto &sd = c->subdiv;
    double ms = 0;
    if (timer_readout(c, sd.displace_timer, &ms, nullptr, nullptr)) return 1;
    if (displace_ms) *displace_ms = ms;
    if (launches) *launches = sd.displace_launches;
    sd.displace_launches = 0;
    return 0;
}

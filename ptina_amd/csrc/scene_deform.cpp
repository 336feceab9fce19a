// scene_deform.cpp -- mesh deformation behind mpt_mesh_set_morph / mpt_mesh_set_skin / mpt_object_set_morph_weights /
// mpt_object_set_joints: the meshes' deltas and skins and the objects' poses on the device, the deform
// table beside scene_compose.cpp's object table, the run table of a launch (mpt_deform_plan: run_table.h's rule), and deform_step:
// the part of mpt_compose that gives the deformed copies their room in the pool and launches deform.hip before compose_kernel.

#include "miptina_ctx.h"

extern "C" int mpt_deform_plan(const int32_t *corners, const int32_t *dirty, int nobj, int32_t *run_obj, int64_t *run_block, int cap, int64_t *blocks) {
    return mpt_run_plan_of(corners, dirty, nobj, MPT_DEFORM_CHUNK, run_obj, run_block, cap, blocks);
}

extern "C" int mpt_skin_check(const uint16_t *joints, const float *weights, int64_t ncorners, int njoints, char *why, int why_size) {
    return (int)mpt_skin_rule(joints, weights, ncorners, njoints, why, why_size > 0 ? (size_t)why_size : 0);
}

// ---------------------------------------------------------------- what scene_compose.cpp tells the table
void deform_object_added(mpt_ctx *c, int obj_id) {
    auto &df = c->deform;
    auto &row = c->compose.rows[obj_id];
    const auto &m = c->compose.meshes[row.mesh].deform;
    if (m.ntargets == 0 && m.njoints == 0) return;
    mpt_ctx::MptDeformPose p;
    p.obj = obj_id; p.mesh = row.mesh;
    p.pose.assign((size_t)m.ntargets + (size_t)m.njoints * 12, 0.0);
    for (int j = 0; j < m.njoints; j++)
        for (int r = 0; r < 3; r++) p.pose[(size_t)m.ntargets + (size_t)j * 12 + 4 * r + r] = 1.0;
    row.pose = (int)df.poses.size();
    df.poses.push_back(std::move(p));
    df.room.stale = true;
}

void deform_scene_cleared(mpt_ctx *c, int meshes) {
    auto &df = c->deform;
    df.poses.clear();
    df.room.copy_verts = 0; df.room.stale = true;
    if (meshes) { df.deltas_used = 0; df.skin_used = 0; }
}

// ---------------------------------------------------------------- the meshes' targets and skins
extern "C" int mpt_mesh_set_morph(mpt_ctx *c, int mesh_id, const float *deltas, int T) {
    if (use(c)) return 1;
    if (check_fresh_mesh(c, mesh_id, "mpt_mesh_set_morph")) return 1;
    auto &df = c->deform;
    auto &m = c->compose.meshes[mesh_id];
    if (m.deform.ntargets) return fail("mpt_mesh_set_morph: mesh %d already has morph targets", mesh_id);
    if (T < 1 || T > MPT_DEFORM_MAX_TARGETS) return fail("mpt_mesh_set_morph: T %d outside [1, %d]", T, MPT_DEFORM_MAX_TARGETS);
    const size_t corners = (size_t)m.nfaces * 3, floats = (size_t)T * corners * 6;
    if (floats > 0 && !deltas) return fail("mpt_mesh_set_morph: null deltas");
    for (size_t k = 0; k < floats; k++)
        if (!std::isfinite(deltas[k]))
            return fail("mpt_mesh_set_morph: deltas[%zu][%zu][%zu] is not finite", k / (corners * 6), k / 6 % corners, k % 6);
    if (grow_keeping(df.bufs.deltas, df.deltas_used + floats, df.deltas_used, c->stream)) return 1;
    if (floats > 0) {
        HIP_TRY(hipMemcpyAsync(df.bufs.deltas + df.deltas_used, deltas, floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));      // the caller's array is borrowed for the call
    }
    m.deform.ntargets = T; m.deform.delta_at = df.deltas_used;
    df.deltas_used += floats;
    return 0;
}

extern "C" int mpt_mesh_set_skin(mpt_ctx *c, int mesh_id, const uint16_t *joints, const float *weights, int njoints) {
    if (use(c)) return 1;
    if (check_fresh_mesh(c, mesh_id, "mpt_mesh_set_skin")) return 1;
    auto &df = c->deform;
    auto &m = c->compose.meshes[mesh_id];
    if (m.deform.njoints) return fail("mpt_mesh_set_skin: mesh %d already has a skin", mesh_id);
    const size_t corners = (size_t)m.nfaces * 3;
    char why[160];
    if (mpt_skin_rule(joints, weights, (int64_t)corners, njoints, why, sizeof why) != MPT_SKIN_OK) return fail("mpt_mesh_set_skin: %s", why);
    if (grow_keeping(df.bufs.joints, (df.skin_used + corners) * 4, df.skin_used * 4, c->stream) ||
        grow_keeping(df.bufs.weights, (df.skin_used + corners) * 4, df.skin_used * 4, c->stream)) return 1;
    if (corners > 0) {
        HIP_TRY(hipMemcpyAsync(df.bufs.joints + df.skin_used * 4, joints, corners * 4 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(df.bufs.weights + df.skin_used * 4, weights, corners * 4 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    m.deform.njoints = njoints; m.deform.skin_at = df.skin_used;
    df.skin_used += corners;
    return 0;
}

// ---------------------------------------------------------------- the objects' poses
// the entry check of the calls that name an object: refuses an unknown one; *pose is the object's pose, null for an object that
// is not deformable (the caller words that refusal: what its mesh lacks)
static int pose_of(mpt_ctx *c, int obj_id, const char *who, mpt_ctx::MptDeformPose **pose) {
    if (check_object(c, obj_id, who)) return 1;
    const int row = c->compose.rows[obj_id].pose;
    *pose = row < 0 ? nullptr : &c->deform.poses[row];
    return 0;
}

extern "C" int mpt_object_set_morph_weights(mpt_ctx *c, int obj_id, const double *w, int n) {
    if (use(c)) return 1;
    mpt_ctx::MptDeformPose *p = nullptr;
    if (pose_of(c, obj_id, "mpt_object_set_morph_weights", &p)) return 1;
    const int T = p ? c->compose.meshes[p->mesh].deform.ntargets : 0;
    if (T == 0) return fail("mpt_object_set_morph_weights: the mesh of object %d has no morph targets", obj_id);
    if (n != T) return fail("mpt_object_set_morph_weights: n %d, the mesh of object %d has %d morph targets", n, obj_id, T);
    if (!w) return fail("mpt_object_set_morph_weights: null w");
    if (p->clip >= 0) return fail("mpt_object_set_morph_weights: object %d is bound to clip %d, which gives its pose: unbind it first (mpt_object_set_animation with clip -1)", obj_id, p->clip);
    for (int t = 0; t < T; t++)
        if (!std::isfinite(w[t])) return fail("mpt_object_set_morph_weights: w[%d] is not finite", t);
    memcpy(p->pose.data(), w, (size_t)T * sizeof(double));
    p->dirty = true;
    c->compose.rows[obj_id].dirty = mpt_ctx::MPT_OBJ_UPLOAD;
    subdiv_pose_changed(c, obj_id);
    return 0;
}

extern "C" int mpt_object_set_joints(mpt_ctx *c, int obj_id, const double *mats, int n) {
    if (use(c)) return 1;
    mpt_ctx::MptDeformPose *p = nullptr;
    if (pose_of(c, obj_id, "mpt_object_set_joints", &p)) return 1;
    const int nj = p ? c->compose.meshes[p->mesh].deform.njoints : 0, T = nj ? c->compose.meshes[p->mesh].deform.ntargets : 0;
    if (nj == 0) return fail("mpt_object_set_joints: the mesh of object %d has no skin", obj_id);
    if (n != nj) return fail("mpt_object_set_joints: n %d, the skin of the mesh of object %d has %d joints", n, obj_id, nj);
    if (!mats) return fail("mpt_object_set_joints: null mats");
    if (p->clip >= 0) return fail("mpt_object_set_joints: object %d is bound to clip %d, which gives its pose: unbind it first (mpt_object_set_animation with clip -1)", obj_id, p->clip);
    static const double bottom[4] = { 0, 0, 0, 1 };
    for (int j = 0; j < nj; j++) {
        for (int k = 0; k < 16; k++)
            if (!std::isfinite(mats[16 * j + k])) return fail("mpt_object_set_joints: mats[%d][%d] is not finite", j, k);
        for (int k = 0; k < 4; k++)
            if (!(mats[16 * j + 12 + k] == bottom[k])) return fail("mpt_object_set_joints: the bottom row of mats[%d] is not 0 0 0 1 (not affine)", j);
    }
    for (int j = 0; j < nj; j++) memcpy(p->pose.data() + T + (size_t)j * 12, mats + 16 * j, 12 * sizeof(double));
    p->dirty = true;
    c->compose.rows[obj_id].dirty = mpt_ctx::MPT_OBJ_UPLOAD;
    subdiv_pose_changed(c, obj_id);
    return 0;
}

// ---------------------------------------------------------------- the step of mpt_compose
// Called with the stream idle, after mpt_compose's own refusals and before it uploads the object table.  At a relayout (objects
// added or dropped, or the copies lost their room) the copies are laid out behind the meshes, the pool grows to hold them, the
// objects' mesh_vert is pointed at them -- mpt_compose then uploads the whole table -- and every deformable object is deformed;
// else the objects whose pose changed.  Nothing here waits for the device: the uploads read the poses and the tables the context
// keeps (h_objs, h_runs), which are next written by the next call, behind mpt_compose's closing synchronise.
// An object bound to a clip (scene_anim.cpp) has no pose to upload: anim_step evaluates the poses of all such objects on the device,
// in one launch between the uploads and the deform kernel.
int deform_step(mpt_ctx *c) {
    auto &cp = c->compose;
    auto &df = c->deform;
    c->anim.stats.evaluated_objects = 0; c->anim.evaluated_blended = 0;
    df.stats.deformed_objects = df.stats.deformed_corners = 0;
    df.stats.deformable_objects = (int64_t)df.poses.size();
    const int np = (int)df.poses.size();
    if (np == 0) { df.stats.copy_verts = 0; return 0; }
    const bool all = cp.relayout || df.room.stale;
    if (all) {
        if (lay_copies(c, df.room, df.poses, cp.pool_verts, [&](const auto &p) { return (size_t)cp.meshes[p.mesh].nfaces * 3; }, "deformed")) return 1;
        size_t pose_at = 0;
        for (auto &p : df.poses) {
            cp.objs[p.obj].mesh_vert = (int32_t)p.copy_vert;
            p.pose_at = pose_at;
            pose_at += p.pose.size();
        }
        if (df.bufs.pose.reserve(pose_at) || df.bufs.reserve_tables((size_t)np)) return 1;
        df.room.stale = false;
    }
    df.stats.copy_verts = (int64_t)df.room.copy_verts;
    std::vector<MptDeformObj> &table = df.h_objs;
    table.resize((size_t)np);
    std::vector<int32_t> corners((size_t)np), dirty((size_t)np);
    for (int k = 0; k < np; k++) {
        const auto &p = df.poses[k];
        const auto &m = cp.meshes[p.mesh].deform;
        MptDeformObj &t = table[k];
        t = MptDeformObj{};
        t.src_vert = (int32_t)cp.meshes[p.mesh].vert; t.dst_vert = (int32_t)p.copy_vert; t.nverts = cp.meshes[p.mesh].nfaces * 3;
        t.ntargets = m.ntargets; t.njoints = m.njoints;
        t.delta_at = (int64_t)m.delta_at; t.skin_at = (int64_t)m.skin_at; t.pose_at = (int64_t)p.pose_at;
        corners[k] = t.nverts; dirty[k] = all || p.dirty;
    }
    df.h_runs.resize((size_t)np);
    int blocks = 0;
    const int nruns = mpt_run_plan_into(corners.data(), dirty.data(), np, MPT_DEFORM_CHUNK, df.h_runs.data(), &blocks);
    if (nruns < 0) return fail("too many corners to deform");
    std::vector<int> bound;
    for (int k = 0; k < np; k++) {
        auto &p = df.poses[k];
        if (!dirty[k]) continue;
        df.stats.deformed_objects++; df.stats.deformed_corners += corners[k];
        if (p.clip >= 0) { bound.push_back(k); continue; }
        if (!p.pose.empty())
            HIP_TRY(hipMemcpyAsync(df.bufs.pose + p.pose_at, p.pose.data(), p.pose.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    if (!bound.empty() && anim_step(c, bound)) return 1;
    if (nruns > 0) {
        HIP_TRY(hipMemcpyAsync(df.bufs.objs, table.data(), (size_t)np * sizeof(MptDeformObj), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(df.bufs.runs, df.h_runs.data(), (size_t)nruns * sizeof(MptRun), hipMemcpyHostToDevice, c->stream));
        MptTimedSpan span(df.timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(mpt_launch_deform(cp.bufs.pool, df.bufs.objs, df.bufs.runs, nruns, blocks, df.bufs.deltas, df.bufs.joints, df.bufs.weights,
                                  df.bufs.pose, c->stream));
        HIP_TRY(span.end());
    }
    for (auto &p : df.poses) p.dirty = false;
    return 0;
}

// ---------------------------------------------------------------- read-backs
extern "C" int mpt_get_deformed(mpt_ctx *c, int obj_id, float *verts, int cap_faces) {
    if (use_ro(c)) return 1;
    mpt_ctx::MptDeformPose *p = nullptr;
    if (pose_of(c, obj_id, "mpt_get_deformed", &p)) return 1;
    if (!p) return fail("mpt_get_deformed: the mesh of object %d has neither morph targets nor a skin", obj_id);
    return read_copy(c, p->copy_vert, c->deform.room.stale, c->compose.meshes[p->mesh].nfaces, obj_id, verts, cap_faces, "mpt_get_deformed", "deformed", "mesh");
}

extern "C" int mpt_deform_stats(mpt_ctx *c, mpt_deform_info *out) {
    if (!c || !out) return fail("null argument");
    *out = c->deform.stats;
    out->deformable_objects = (int64_t)c->deform.poses.size();
    out->copy_verts = (int64_t)c->deform.room.copy_verts;
    return 0;
}

extern "C" int mpt_deform_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->deform.timer, ms, nullptr, launches);
}

// scene_anim.cpp -- keyframe animation behind mpt_mesh_set_skeleton / mpt_mesh_add_clip / mpt_object_set_animation / mpt_scene_set_time
// (DESIGN.md section 3.17.1): the meshes' skeletons and clips in arenas on the device, the objects' bindings beside their poses
// (scene_deform.cpp's table), and anim_step: the part of deform_step that evaluates the bound objects' poses with anim.hip where it
// would upload them.  The rule itself is anim_rule.h's; the C ABI has it whole as mpt_anim_rule and a clip's validation as
// mpt_clip_check (no context, no GPU).

#include "miptina_ctx.h"

extern "C" int mpt_clip_check(int njoints, int ntargets, int ntracks, const int32_t *tracks, const float *times, int64_t ntimes, const float *values,
                              int64_t nvalues, char *why, int why_size) {
    return (int)mpt_clip_rule(njoints, ntargets, ntracks, tracks, times, ntimes, values, nvalues, why, why_size > 0 ? (size_t)why_size : 0);
}

extern "C" int mpt_anim_rule(int njoints, int ntargets, const int32_t *parents, const double *rest, const double *inverse_bind, int ntracks,
                             const int32_t *tracks, const float *times, int64_t ntimes, const float *values, int64_t nvalues, double offset, double speed,
                             int loop, double t, double *pose) {
    if (njoints < 0 || ntargets < 0 || ntargets > MPT_DEFORM_MAX_TARGETS || !pose) return 201;
    if (njoints > 0) {
        const MptSkeletonVerdict v = mpt_skeleton_rule(njoints, parents, rest, inverse_bind, nullptr, 0);
        if (v != MPT_SKELETON_OK) return 200 + (int)v;
    }
    const MptClipVerdict v = mpt_clip_rule(njoints, ntargets, ntracks, tracks, times, ntimes, values, nvalues, nullptr, 0);
    if (v != MPT_CLIP_OK) return 100 + (int)v;
    std::vector<MptAnimTrack> tr((size_t)ntracks);
    double t0, t1;
    mpt_anim_tracks(ntargets, ntracks, tracks, times, tr.data(), &t0, &t1);
    const double tau = mpt_anim_local_time(t, offset, speed, loop, t0, t1);
    mpt_anim_pose(njoints, ntargets, parents, rest, inverse_bind, ntracks, tr.data(), times, values, tau, pose);
    return 0;
}

// ---------------------------------------------------------------- what scene_compose.cpp tells the table
void anim_scene_cleared(mpt_ctx *c, int meshes) {
    auto &an = c->anim;                                  // (the bindings went with deform.poses)
    if (!meshes) return;
    an.clips.clear();
    an.joints_used = an.tracks_used = an.times_used = an.values_used = 0;
    an.skeletons = 0;
}

// ---------------------------------------------------------------- the meshes' skeletons and clips
// n more elements behind the first `used` of an arena; the caller's array is borrowed for the call
template <class T>
static int append(mpt_ctx *c, DevBuf<T> &buf, size_t used, const T *src, size_t n) {
    if (n == 0) return 0;
    if (grow_keeping(buf, used + n, used, c->stream)) return 1;
    HIP_TRY(hipMemcpyAsync(buf + used, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mpt_mesh_set_skeleton(mpt_ctx *c, int mesh_id, int njoints, const int32_t *parents, const double *rest, const double *inverse_bind) {
    if (use(c)) return 1;
    if (check_fresh_mesh(c, mesh_id, "mpt_mesh_set_skeleton")) return 1;
    auto &an = c->anim;
    auto &m = c->compose.meshes[mesh_id].deform;
    if (m.skeleton) return fail("mpt_mesh_set_skeleton: mesh %d already has a skeleton", mesh_id);
    if (m.njoints == 0) return fail("mpt_mesh_set_skeleton: mesh %d has no skin: mpt_mesh_set_skin comes first", mesh_id);
    if (njoints != m.njoints) return fail("mpt_mesh_set_skeleton: njoints %d, the skin of mesh %d has %d joints", njoints, mesh_id, m.njoints);
    char why[200];
    if (mpt_skeleton_rule(njoints, parents, rest, inverse_bind, why, sizeof why) != MPT_SKELETON_OK) return fail("mpt_mesh_set_skeleton: %s", why);
    std::vector<int32_t> depth((size_t)njoints);
    const int levels = mpt_anim_depths(njoints, parents, depth.data());
    const size_t at = an.joints_used, n = (size_t)njoints;
    if (append(c, an.bufs.parents, at, parents, n) || append(c, an.bufs.depths, at, depth.data(), n) ||
        append(c, an.bufs.rest, at * MPT_ANIM_REST, rest, n * MPT_ANIM_REST) || append(c, an.bufs.inverse_bind, at * 12, inverse_bind, n * 12)) return 1;
    m.skeleton = true; m.joint_at = at; m.levels = levels;
    an.joints_used += n; an.skeletons++;
    return 0;
}

extern "C" int mpt_mesh_add_clip(mpt_ctx *c, int mesh_id, int ntracks, const int32_t *tracks, const float *times, int64_t ntimes, const float *values,
                                 int64_t nvalues, int *clip_id) {
    if (use(c)) return 1;
    if (check_fresh_mesh(c, mesh_id, "mpt_mesh_add_clip")) return 1;
    if (!clip_id) return fail("mpt_mesh_add_clip: null clip_id");
    auto &an = c->anim;
    const auto &m = c->compose.meshes[mesh_id].deform;
    if (m.ntargets == 0 && m.njoints == 0) return fail("mpt_mesh_add_clip: mesh %d has neither morph targets nor a skin", mesh_id);
    if (m.njoints > 0 && !m.skeleton) return fail("mpt_mesh_add_clip: mesh %d has a skin and no skeleton: mpt_mesh_set_skeleton comes first", mesh_id);
    char why[200];
    if (mpt_clip_rule(m.njoints, m.ntargets, ntracks, tracks, times, ntimes, values, nvalues, why, sizeof why) != MPT_CLIP_OK)
        return fail("mpt_mesh_add_clip: %s", why);
    mpt_ctx::MptAnimClip clip;
    clip.mesh = mesh_id; clip.ntracks = ntracks; clip.track_at = an.tracks_used;
    std::vector<MptAnimTrack> tr((size_t)ntracks);
    mpt_anim_tracks(m.ntargets, ntracks, tracks, times, tr.data(), &clip.t0, &clip.t1);
    for (auto &r : tr) { r.time_at += (int64_t)an.times_used; r.value_at += (int64_t)an.values_used; }
    if (append(c, an.bufs.tracks, an.tracks_used, tr.data(), tr.size()) || append(c, an.bufs.times, an.times_used, times, (size_t)ntimes) ||
        append(c, an.bufs.values, an.values_used, values, (size_t)nvalues)) return 1;
    an.tracks_used += tr.size(); an.times_used += (size_t)ntimes; an.values_used += (size_t)nvalues;
    *clip_id = (int)an.clips.size();
    an.clips.push_back(clip);
    return 0;
}

// ---------------------------------------------------------------- the objects' bindings and the scene's time
// what mpt_object_set_joints does to one object: the next mpt_compose writes its pose, deforms it and composes it again
static void pose_changed(mpt_ctx *c, mpt_ctx::MptDeformPose &p) {
    p.dirty = true;
    c->compose.rows[p.obj].dirty = mpt_ctx::MPT_OBJ_UPLOAD;
    subdiv_pose_changed(c, p.obj);
}

extern "C" int mpt_object_set_animation(mpt_ctx *c, int obj_id, int clip_id, double offset, double speed, int loop) {
    if (use(c)) return 1;
    if (check_object(c, obj_id, "mpt_object_set_animation")) return 1;
    const int row = c->compose.rows[obj_id].pose;
    if (row < 0) return fail("mpt_object_set_animation: the mesh of object %d has neither morph targets nor a skin", obj_id);
    auto &p = c->deform.poses[row];
    if (clip_id == -1) {
        if (p.clip < 0) return 0;
        p.clip = -1;
        pose_changed(c, p);
        return 0;
    }
    const auto &clips = c->anim.clips;
    if (clip_id < 0 || (size_t)clip_id >= clips.size()) return fail("mpt_object_set_animation: unknown clip %d (%zu clips)", clip_id, clips.size());
    if (clips[clip_id].mesh != p.mesh)
        return fail("mpt_object_set_animation: clip %d is a clip of mesh %d, object %d an object of mesh %d", clip_id, clips[clip_id].mesh, obj_id, p.mesh);
    if (!std::isfinite(offset)) return fail("mpt_object_set_animation: offset is not finite");
    if (!std::isfinite(speed)) return fail("mpt_object_set_animation: speed is not finite");
    p.clip = clip_id; p.offset = offset; p.speed = speed; p.loop = loop != 0;
    pose_changed(c, p);
    return 0;
}

extern "C" int mpt_scene_set_time(mpt_ctx *c, double t) {
    if (use(c)) return 1;
    if (!std::isfinite(t)) return fail("mpt_scene_set_time: t is not finite");
    if (memcmp(&t, &c->anim.time, sizeof t) == 0) return 0;          // the same time again: nothing changed
    c->anim.time = t;
    for (auto &p : c->deform.poses)
        if (p.clip >= 0) pose_changed(c, p);
    return 0;
}

// ---------------------------------------------------------------- the step of deform_step
// rows: the rows of deform.poses whose object is bound and whose pose this mpt_compose writes.  One launch for all of them, queued on
// the stream behind the unbound objects' uploads and in front of the deform kernel; nothing waits for the device
int anim_step(mpt_ctx *c, const std::vector<int> &rows) {
    auto &an = c->anim;
    an.stats.evaluated_objects = (int64_t)rows.size();
    if (rows.empty()) return 0;
    an.h_objs.resize(rows.size());
    for (size_t k = 0; k < rows.size(); k++) {
        const auto &p = c->deform.poses[rows[k]];
        const auto &m = c->compose.meshes[p.mesh].deform;
        const auto &clip = an.clips[p.clip];
        MptAnimObj &o = an.h_objs[k];
        o = MptAnimObj{};
        o.njoints = m.njoints; o.ntargets = m.ntargets; o.ntracks = clip.ntracks; o.loop = p.loop; o.levels = m.levels;
        o.joint_at = (int64_t)m.joint_at; o.track_at = (int64_t)clip.track_at; o.pose_at = (int64_t)p.pose_at;
        o.offset = p.offset; o.speed = p.speed; o.t0 = clip.t0; o.t1 = clip.t1;
    }
    if (an.bufs.objs.reserve(rows.size())) return 1;
    HIP_TRY(hipMemcpyAsync(an.bufs.objs, an.h_objs.data(), rows.size() * sizeof(MptAnimObj), hipMemcpyHostToDevice, c->stream));
    MptTimedSpan span(an.timer, c->stream);
    HIP_TRY(span.begun);
    HIP_TRY(mpt_launch_anim(an.bufs.objs, (int)rows.size(), an.time, an.bufs.parents, an.bufs.depths, an.bufs.rest, an.bufs.inverse_bind, an.bufs.tracks,
                            an.bufs.times, an.bufs.values, c->deform.bufs.pose, c->stream));
    HIP_TRY(span.end());
    return 0;
}

// ---------------------------------------------------------------- read-backs
extern "C" int mpt_get_pose(mpt_ctx *c, int obj_id, double *pose, int cap) {
    if (use_ro(c)) return 1;
    if (check_object(c, obj_id, "mpt_get_pose")) return 1;
    const int row = c->compose.rows[obj_id].pose;
    if (row < 0) return fail("mpt_get_pose: the mesh of object %d has neither morph targets nor a skin", obj_id);
    const auto &p = c->deform.poses[row];
    if (p.copy_vert < 0 || c->deform.room.stale) return fail("mpt_get_pose: object %d has no pose on the device yet: call mpt_compose", obj_id);
    if ((size_t)std::max(cap, 0) < p.pose.size()) return fail("mpt_get_pose: room for %d doubles, the pose of object %d has %zu", cap, obj_id, p.pose.size());
    if (p.pose.empty()) return 0;
    if (!pose) return fail("mpt_get_pose: null pose");
    return read_back(c, pose, c->deform.bufs.pose + p.pose_at, p.pose.size() * sizeof(double));
}

extern "C" int mpt_anim_stats(mpt_ctx *c, mpt_anim_info *out) {
    if (!c || !out) return fail("null argument");
    *out = c->anim.stats;
    out->skeletons = c->anim.skeletons; out->clips = (int64_t)c->anim.clips.size(); out->tracks = (int64_t)c->anim.tracks_used;
    out->bound_objects = 0;
    for (const auto &p : c->deform.poses) out->bound_objects += p.clip >= 0;
    return 0;
}

extern "C" int mpt_anim_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->anim.timer, ms, nullptr, launches);
}

extern "C" int mpt_anim_trig(mpt_ctx *c, const double *x, int n, double *acos_out, double *sin_out) {
    if (use_ro(c)) return 1;
    if (n < 1 || !x || !acos_out || !sin_out) return fail("mpt_anim_trig: x, acos_out and sin_out must hold n >= 1 values");
    DevBuf<double> d;
    if (d.reserve((size_t)n * 3)) return 1;
    HIP_TRY(hipMemcpyAsync(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(mpt_launch_anim_trig(d, n, d + n, d + 2 * (size_t)n, c->stream));
    return read_back(c, acos_out, d + n, (size_t)n * sizeof(double)) || read_back(c, sin_out, d + 2 * (size_t)n, (size_t)n * sizeof(double));
}

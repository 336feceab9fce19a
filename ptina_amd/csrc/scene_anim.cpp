// scene_anim.cpp -- keyframe animation behind mpt_mesh_set_skeleton / mpt_mesh_add_clip / mpt_object_set_animation / mpt_scene_set_time
// (DESIGN.md section 3.17.1): the meshes' skeletons and clips in arenas on the device, the objects' bindings beside their poses
// (scene_deform.cpp's table), and anim_step: the part of deform_step that evaluates the bound objects' poses with anim.hip where it
// would upload them.  Behind mpt_object_set_animation_blend / mpt_scene_add_object_clip / mpt_object_set_motion (section 3.17.2): an
// object's second binding beside its first, object clips in the same arenas and list, the motion bindings, and motion_step: the part of
// mpt_compose that writes the moved objects' matrices into the object table with anim.hip's motion_kernel.  The rule itself is anim_rule.h's; the C ABI has it whole as mpt_anim_rule and a clip's validation as
// mpt_clip_check (no context, no GPU).  Behind mpt_object_set_parent (section 3.17.3): the parent bindings in the objects' rows,
// hierarchy_mark and hierarchy_step, which writes the bound children's matrices with hierarchy.hip; whole as mpt_hierarchy_rule.

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

// The whole evaluation of one pose of two blended clips (A's arrays, then B's) at scene time t.  0, or 100 + the verdict of clip A, 300 +
// that of clip B, 200 + the skeleton's, 400 + the second binding's (mpt_blend_rule), 201 for bad arrays
extern "C" int mpt_anim_blend_rule(int njoints, int ntargets, const int32_t *parents, const double *rest, const double *inverse_bind, int ntracks_a,
                                   const int32_t *tracks_a, const float *times_a, int64_t ntimes_a, const float *values_a, int64_t nvalues_a, double offset_a,
                                   double speed_a, int loop_a, int ntracks_b, const int32_t *tracks_b, const float *times_b, int64_t ntimes_b,
                                   const float *values_b, int64_t nvalues_b, double offset_b, double speed_b, int loop_b, double w0, double w1,
                                   double fade_start, double fade_duration, double t, double *pose) {
    if (njoints < 0 || ntargets < 0 || ntargets > MPT_DEFORM_MAX_TARGETS || !pose) return 201;
    if (njoints > 0) {
        const MptSkeletonVerdict v = mpt_skeleton_rule(njoints, parents, rest, inverse_bind, nullptr, 0);
        if (v != MPT_SKELETON_OK) return 200 + (int)v;
    }
    MptClipVerdict v = mpt_clip_rule(njoints, ntargets, ntracks_a, tracks_a, times_a, ntimes_a, values_a, nvalues_a, nullptr, 0);
    if (v != MPT_CLIP_OK) return 100 + (int)v;
    v = mpt_clip_rule(njoints, ntargets, ntracks_b, tracks_b, times_b, ntimes_b, values_b, nvalues_b, nullptr, 0);
    if (v != MPT_CLIP_OK) return 300 + (int)v;
    const MptBlendVerdict bv = mpt_blend_rule(offset_b, speed_b, w0, w1, fade_start, fade_duration, nullptr, 0);
    if (bv != MPT_BLEND_OK) return 400 + (int)bv;
    std::vector<MptAnimTrack> ta((size_t)ntracks_a), tb((size_t)ntracks_b);
    double a0, a1, b0, b1;
    mpt_anim_tracks(ntargets, ntracks_a, tracks_a, times_a, ta.data(), &a0, &a1);
    mpt_anim_tracks(ntargets, ntracks_b, tracks_b, times_b, tb.data(), &b0, &b1);
    mpt_anim_pose_blend(njoints, ntargets, parents, rest, inverse_bind, ntracks_a, ta.data(), times_a, values_a,
                        mpt_anim_local_time(t, offset_a, speed_a, loop_a, a0, a1), ntracks_b, tb.data(), times_b, values_b,
                        mpt_anim_local_time(t, offset_b, speed_b, loop_b, b0, b1), mpt_anim_blend_weight(t, w0, w1, fade_start, fade_duration), pose);
    return 0;
}

// ... and of one world matrix of an object moved by an object clip.  0, or 100 + the clip's verdict (as a clip of one joint and no targets),
// 500 + the binding's (mpt_motion_binding_rule), 201 for a null world
extern "C" int mpt_motion_rule(int ntracks, const int32_t *tracks, const float *times, int64_t ntimes, const float *values, int64_t nvalues, double offset,
                               double speed, int loop, const double *rest, const double *base, double t, double *world) {
    if (!world) return 201;
    const MptClipVerdict v = mpt_clip_rule(1, 0, ntracks, tracks, times, ntimes, values, nvalues, nullptr, 0);
    if (v != MPT_CLIP_OK) return 100 + (int)v;
    const MptMotionVerdict mv = mpt_motion_binding_rule(offset, speed, rest, base, nullptr, 0);
    if (mv != MPT_MOTION_OK) return 500 + (int)mv;
    mpt_ctx::MptMotion m;                                // (the defaults: rest at the origin, the identity as base)
    if (rest) memcpy(m.rest, rest, sizeof m.rest);
    if (base) memcpy(m.base, base, sizeof m.base);
    std::vector<MptAnimTrack> tr((size_t)ntracks);
    double t0, t1;
    mpt_anim_tracks(0, ntracks, tracks, times, tr.data(), &t0, &t1);
    mpt_anim_motion(ntracks, tr.data(), times, values, mpt_anim_local_time(t, offset, speed, loop, t0, t1), m.rest, m.base, world);
    return 0;
}

// ---------------------------------------------------------------- what scene_compose.cpp tells the table
void anim_scene_cleared(mpt_ctx *c, int meshes) {
    auto &an = c->anim;                                  // (the bindings of poses went with deform.poses)
    an.motions.clear(); an.moved = 0;
    an.bound_children = 0; an.order.clear(); an.depth.clear(); an.order_stale = true;   // (the parent bindings went with the objects' rows)
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

// a checked clip of mesh `mesh` (-1: an object clip) goes behind the others in the arenas and the list
static int append_clip(mpt_ctx *c, int mesh, int ntargets, int ntracks, const int32_t *tracks, const float *times, int64_t ntimes, const float *values,
                       int64_t nvalues, int *clip_id) {
    auto &an = c->anim;
    mpt_ctx::MptAnimClip clip;
    clip.mesh = mesh; clip.ntracks = ntracks; clip.track_at = an.tracks_used;
    std::vector<MptAnimTrack> tr((size_t)ntracks);
    mpt_anim_tracks(ntargets, ntracks, tracks, times, tr.data(), &clip.t0, &clip.t1);
    for (auto &r : tr) { r.time_at += (int64_t)an.times_used; r.value_at += (int64_t)an.values_used; }
    if (append(c, an.bufs.tracks, an.tracks_used, tr.data(), tr.size()) || append(c, an.bufs.times, an.times_used, times, (size_t)ntimes) ||
        append(c, an.bufs.values, an.values_used, values, (size_t)nvalues)) return 1;
    an.tracks_used += tr.size(); an.times_used += (size_t)ntimes; an.values_used += (size_t)nvalues;
    *clip_id = (int)an.clips.size();
    an.clips.push_back(clip);
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
    return append_clip(c, mesh_id, m.ntargets, ntracks, tracks, times, ntimes, values, nvalues, clip_id);
}

extern "C" int mpt_scene_add_object_clip(mpt_ctx *c, int ntracks, const int32_t *tracks, const float *times, int64_t ntimes, const float *values,
                                         int64_t nvalues, int *clip_id) {
    if (use(c)) return 1;
    if (!clip_id) return fail("mpt_scene_add_object_clip: null clip_id");
    char why[200];
    if (mpt_clip_rule(1, 0, ntracks, tracks, times, ntimes, values, nvalues, why, sizeof why) != MPT_CLIP_OK)
        return fail("mpt_scene_add_object_clip: %s (an object clip animates target 0, the object's node, on the paths T, R and S)", why);
    return append_clip(c, -1, 0, ntracks, tracks, times, ntimes, values, nvalues, clip_id);
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
        p.clip = p.clip_b = -1;                          // (both bindings)
        pose_changed(c, p);
        return 0;
    }
    const auto &clips = c->anim.clips;
    if (clip_id < 0 || (size_t)clip_id >= clips.size()) return fail("mpt_object_set_animation: unknown clip %d (%zu clips)", clip_id, clips.size());
    if (clips[clip_id].mesh < 0)
        return fail("mpt_object_set_animation: clip %d is an object clip, which moves an object (mpt_object_set_motion) and poses none", clip_id);
    if (clips[clip_id].mesh != p.mesh)
        return fail("mpt_object_set_animation: clip %d is a clip of mesh %d, object %d an object of mesh %d", clip_id, clips[clip_id].mesh, obj_id, p.mesh);
    if (!std::isfinite(offset)) return fail("mpt_object_set_animation: offset is not finite");
    if (!std::isfinite(speed)) return fail("mpt_object_set_animation: speed is not finite");
    p.clip = clip_id; p.offset = offset; p.speed = speed; p.loop = loop != 0;
    pose_changed(c, p);
    return 0;
}

extern "C" int mpt_object_set_animation_blend(mpt_ctx *c, int obj_id, int clip_b, double offset, double speed, int loop, double w0, double w1,
                                              double fade_start, double fade_duration) {
    if (use(c)) return 1;
    if (check_object(c, obj_id, "mpt_object_set_animation_blend")) return 1;
    const int row = c->compose.rows[obj_id].pose;
    if (row < 0) return fail("mpt_object_set_animation_blend: the mesh of object %d has neither morph targets nor a skin", obj_id);
    auto &p = c->deform.poses[row];
    if (clip_b == -1) {
        if (p.clip_b < 0) return 0;
        p.clip_b = -1;
        pose_changed(c, p);
        return 0;
    }
    if (p.clip < 0)
        return fail("mpt_object_set_animation_blend: object %d is not bound to a clip: mpt_object_set_animation gives the first binding", obj_id);
    const auto &clips = c->anim.clips;
    if (clip_b < 0 || (size_t)clip_b >= clips.size()) return fail("mpt_object_set_animation_blend: unknown clip %d (%zu clips)", clip_b, clips.size());
    if (clips[clip_b].mesh < 0)
        return fail("mpt_object_set_animation_blend: clip %d is an object clip, which moves an object (mpt_object_set_motion) and poses none", clip_b);
    if (clips[clip_b].mesh != p.mesh)
        return fail("mpt_object_set_animation_blend: clip %d is a clip of mesh %d, object %d an object of mesh %d", clip_b, clips[clip_b].mesh, obj_id, p.mesh);
    char why[80];
    if (mpt_blend_rule(offset, speed, w0, w1, fade_start, fade_duration, why, sizeof why) != MPT_BLEND_OK)
        return fail("mpt_object_set_animation_blend: %s", why);
    p.clip_b = clip_b; p.offset_b = offset; p.speed_b = speed; p.loop_b = loop != 0;
    p.w0 = w0; p.w1 = w1; p.fade_start = fade_start; p.fade_duration = fade_duration;
    pose_changed(c, p);
    return 0;
}

extern "C" int mpt_object_set_motion(mpt_ctx *c, int obj_id, int clip_id, double offset, double speed, int loop, const double *rest, const double *base) {
    if (use(c)) return 1;
    if (check_object(c, obj_id, "mpt_object_set_motion")) return 1;
    auto &an = c->anim;
    auto &row = c->compose.rows[obj_id];
    if (clip_id == -1) {                                 // back to the matrix mpt_object_add / mpt_object_set_world last gave: the host's row goes up
        if (row.motion < 0 || an.motions[row.motion].clip < 0) return 0;
        an.motions[row.motion].clip = -1; an.moved--;
        row.dirty |= mpt_ctx::MPT_OBJ_UPLOAD;
        return 0;
    }
    if (row.scatter >= 0)
        return fail("mpt_object_set_motion: object %d is an instance of scatter %d, which places it on its surface", obj_id, row.scatter);
    if (clip_id < 0 || (size_t)clip_id >= an.clips.size()) return fail("mpt_object_set_motion: unknown clip %d (%zu clips)", clip_id, an.clips.size());
    if (an.clips[clip_id].mesh >= 0)
        return fail("mpt_object_set_motion: clip %d is a clip of mesh %d, which poses an object (mpt_object_set_animation) and moves none: "
                    "mpt_scene_add_object_clip makes an object clip", clip_id, an.clips[clip_id].mesh);
    char why[80];
    if (mpt_motion_binding_rule(offset, speed, rest, base, why, sizeof why) != MPT_MOTION_OK) return fail("mpt_object_set_motion: %s", why);
    if (row.motion < 0) {
        row.motion = (int)an.motions.size();
        an.motions.emplace_back();
        an.motions.back().obj = obj_id;
    }
    auto &m = an.motions[row.motion];
    if (m.clip < 0) an.moved++;
    const mpt_ctx::MptMotion fresh;
    m.clip = clip_id; m.offset = offset; m.speed = speed; m.loop = loop != 0;
    memcpy(m.rest, rest ? rest : fresh.rest, sizeof m.rest);
    memcpy(m.base, base ? base : fresh.base, sizeof m.base);
    row.dirty |= mpt_ctx::MPT_OBJ_MOVED;
    return 0;
}

extern "C" int mpt_scene_set_time(mpt_ctx *c, double t) {
    if (use(c)) return 1;
    if (!std::isfinite(t)) return fail("mpt_scene_set_time: t is not finite");
    if (memcmp(&t, &c->anim.time, sizeof t) == 0) return 0;          // the same time again: nothing changed
    c->anim.time = t;
    for (auto &p : c->deform.poses)
        if (p.clip >= 0) pose_changed(c, p);
    for (const auto &m : c->anim.motions)                // (behind the poses: pose_changed sets an object's flags, this adds one)
        if (m.clip >= 0) c->compose.rows[m.obj].dirty |= mpt_ctx::MPT_OBJ_MOVED;
    return 0;
}

// ---------------------------------------------------------------- the step of deform_step
// rows: the rows of deform.poses whose object is bound and whose pose this mpt_compose writes.  One launch for all of them, queued on
// the stream behind the unbound objects' uploads and in front of the deform kernel; nothing waits for the device
int anim_step(mpt_ctx *c, const std::vector<int> &rows) {
    auto &an = c->anim;
    an.stats.evaluated_objects = (int64_t)rows.size();
    an.evaluated_blended = 0;
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
        if (p.clip_b >= 0) {
            const auto &b = an.clips[p.clip_b];
            o.blend = 1; o.ntracks_b = b.ntracks; o.loop_b = p.loop_b; o.track_b_at = (int64_t)b.track_at;
            o.offset_b = p.offset_b; o.speed_b = p.speed_b; o.t0_b = b.t0; o.t1_b = b.t1;
            o.w0 = p.w0; o.w1 = p.w1; o.fade_start = p.fade_start; o.fade_duration = p.fade_duration;
            an.evaluated_blended++;
        }
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

// The objects that object clips move: inside mpt_compose behind the upload of the object table, whose rows would overwrite what the
// kernel writes, and in front of scatter_step and the composition, which read the matrices from the table.  A bound object is evaluated
// when the table went up whole (a relayout), when its own row went up (its material changed, say) or when mpt_scene_set_time or
// mpt_object_set_motion marked it; one launch for all of them, a lane each.  Without a motion binding in the scene nothing is called.
// A moved object that has a parent binding is hierarchy_step's
int motion_step(mpt_ctx *c) {
    auto &an = c->anim;
    auto &cp = c->compose;
    an.evaluated_moved = 0;
    if (an.moved == 0) return 0;
    an.h_moved.clear();
    for (const auto &m : an.motions) {
        if (m.clip < 0) continue;
        if (cp.rows[m.obj].parent >= 0) continue;        // (a bound child: hierarchy_step evaluates its binding, and its matrix is written once)
        if (!cp.relayout && !(cp.rows[m.obj].dirty & (mpt_ctx::MPT_OBJ_MOVED | mpt_ctx::MPT_OBJ_UPLOAD))) continue;
        const auto &clip = an.clips[m.clip];
        MptMotionObj o{};
        o.obj = m.obj; o.ntracks = clip.ntracks; o.loop = m.loop; o.track_at = (int64_t)clip.track_at;
        o.offset = m.offset; o.speed = m.speed; o.t0 = clip.t0; o.t1 = clip.t1;
        memcpy(o.rest, m.rest, sizeof o.rest); memcpy(o.base, m.base, sizeof o.base);
        an.h_moved.push_back(o);
    }
    const size_t n = an.h_moved.size();
    an.evaluated_moved = (int64_t)n;
    if (n == 0) return 0;
    if (an.bufs.moved.reserve(n)) return 1;
    HIP_TRY(hipMemcpyAsync(an.bufs.moved, an.h_moved.data(), n * sizeof(MptMotionObj), hipMemcpyHostToDevice, c->stream));
    MptTimedSpan span(an.motion_timer, c->stream);
    HIP_TRY(span.begun);
    HIP_TRY(mpt_launch_motion(an.bufs.moved, (int)n, an.time, an.bufs.tracks, an.bufs.times, an.bufs.values, cp.bufs.objs, (int)cp.objs.size(), cp.epoch, c->stream));
    HIP_TRY(span.end());
    return 0;
}

// ---------------------------------------------------------------- parent bindings
extern "C" int mpt_parent_check(int nobj, const int32_t *parents, const int32_t *instance, const int32_t *njoints, int obj, int parent, int joint, char *why,
                                int why_size) {
    return (int)mpt_parent_rule(nobj, parents, instance, njoints, obj, parent, joint, why, why_size > 0 ? (size_t)why_size : 0);
}

// The whole evaluation of one object's world matrix down its chain of ancestors.  0, or 601 for bad arrays, 602 for a chain outside
// [1, 65] links, 603 / 604 for a local matrix / a named palette entry that is not finite, 100 + a link's clip's verdict, 500 + its
// motion binding's
extern "C" int mpt_hierarchy_rule(int n, const double *locals, const int32_t *ntracks, const int32_t *tracks, const float *times, const int64_t *ntimes,
                                  const float *values, const int64_t *nvalues, const double *bindings, const double *rests, const int32_t *joints,
                                  const double *palette, double t, double *world) {
    if (n < 1 || n > MPT_HIER_MAX_DEPTH + 1) return 602;
    if (!locals || !ntracks || !world) return 601;
    static const mpt_ctx::MptMotion fresh;               // (the default rest)
    std::vector<MptHierLink> links((size_t)n);
    std::vector<std::vector<MptAnimTrack>> tr((size_t)n);
    int64_t track_at = 0, time_at = 0, value_at = 0;
    for (int k = 0; k < n; k++) {
        MptHierLink &ln = links[k];
        ln = MptHierLink{};
        ln.local = locals + (size_t)k * 16; ln.ntracks = -1;
        for (int i = 0; i < 16; i++)
            if (!std::isfinite(ln.local[i])) return 603;
        if (k > 0 && joints && joints[k] >= 0) {
            if (!palette) return 601;
            ln.pal = palette + (size_t)k * 12;
            for (int i = 0; i < 12; i++)
                if (!std::isfinite(ln.pal[i])) return 604;
        }
        if (ntracks[k] < 0) continue;
        if (!ntimes || !nvalues || !bindings || ntimes[k] < 0 || nvalues[k] < 0) return 601;
        const int32_t *spec = tracks ? tracks + 4 * track_at : nullptr;
        const float *T = times ? times + time_at : nullptr, *V = values ? values + value_at : nullptr;
        const MptClipVerdict v = mpt_clip_rule(1, 0, ntracks[k], spec, T, ntimes[k], V, nvalues[k], nullptr, 0);
        if (v != MPT_CLIP_OK) return 100 + (int)v;
        const double *b = bindings + (size_t)k * 3;
        ln.rest = rests ? rests + (size_t)k * MPT_ANIM_REST : fresh.rest;
        const MptMotionVerdict mv = mpt_motion_binding_rule(b[0], b[1], ln.rest, ln.local, nullptr, 0);
        if (mv != MPT_MOTION_OK) return 500 + (int)mv;
        tr[k].resize((size_t)ntracks[k]);
        mpt_anim_tracks(0, ntracks[k], spec, T, tr[k].data(), &ln.t0, &ln.t1);
        ln.ntracks = ntracks[k]; ln.tracks = tr[k].data(); ln.times = T; ln.values = V;
        ln.offset = b[0]; ln.speed = b[1]; ln.loop = b[2] != 0.0;
        track_at += ntracks[k]; time_at += ntimes[k]; value_at += nvalues[k];
    }
    mpt_hier_chain(n, links.data(), t, world);
    return 0;
}

extern "C" int mpt_object_set_parent(mpt_ctx *c, int obj_id, int parent_id, int joint) {
    if (use(c)) return 1;
    auto &cp = c->compose;
    auto &an = c->anim;
    const int nobj = (int)cp.rows.size();
    char why[200];
    // (over the rows themselves; an object nothing is bound to -- a tree bound from its root down binds no other -- costs its parent's depth)
    const bool childless = obj_id >= 0 && obj_id < nobj && cp.rows[obj_id].children == 0;
    const MptParentVerdict v = mpt_parent_rule_of(nobj, [&](int o) { return cp.rows[o].parent; }, [&](int o) { return cp.rows[o].scatter >= 0; },
                                                  [&](int o) { return cp.meshes[cp.rows[o].mesh].deform.njoints; }, childless, obj_id, parent_id, joint, why, sizeof why);
    if (v != MPT_PARENT_OK) return fail("mpt_object_set_parent: %s (refusal %d)", why, (int)v);
    auto &row = cp.rows[obj_id];
    if (parent_id == -1) {                               // its matrix is its world again: the host's row goes up (and a motion binding is motion_kernel's again)
        if (row.parent < 0) return 0;
        cp.rows[row.parent].children--;
        row.parent = row.joint = -1;
        an.bound_children--; an.order_stale = true;
        row.dirty |= mpt_ctx::MPT_OBJ_UPLOAD;
        return 0;
    }
    if (row.parent >= 0) cp.rows[row.parent].children--;
    else an.bound_children++;
    row.parent = parent_id; row.joint = joint;
    cp.rows[parent_id].children++;
    an.order_stale = true;
    row.dirty |= mpt_ctx::MPT_OBJ_MOVED;
    return 0;
}

extern "C" int mpt_object_get_parent(mpt_ctx *c, int obj_id, int *parent_id, int *joint) {
    if (use_ro(c)) return 1;
    if (check_object(c, obj_id, "mpt_object_get_parent")) return 1;
    if (parent_id) *parent_id = c->compose.rows[obj_id].parent;
    if (joint) *joint = c->compose.rows[obj_id].joint;
    return 0;
}

// every object's depth and the bound children by depth, then id: made again behind a change of the bindings
static void hierarchy_order(mpt_ctx *c) {
    auto &an = c->anim;
    const auto &rows = c->compose.rows;
    if (!an.order_stale && an.depth.size() == rows.size()) return;   // (objects added since have no binding, and a depth all the same)
    const int nobj = (int)rows.size();
    an.depth.assign((size_t)nobj, 0);
    an.deepest = 0;
    std::vector<int> count(MPT_HIER_MAX_DEPTH + 2, 0);
    for (int o = 0; o < nobj; o++) {
        int d = 0;
        for (int a = rows[o].parent; a >= 0 && d < MPT_HIER_MAX_DEPTH; a = rows[a].parent) d++;
        an.depth[o] = d;
        if (d > 0) count[d + 1]++;
        an.deepest = std::max(an.deepest, d);
    }
    for (size_t d = 1; d < count.size(); d++) count[d] += count[d - 1];   // count[d]: the first place of depth d
    an.order.assign((size_t)an.bound_children, 0);
    for (int o = 0; o < nobj; o++)
        if (an.depth[o] > 0) an.order[(size_t)count[an.depth[o]]++] = o;
    an.order_stale = false;
}

// At the head of mpt_compose, before anything reads the dirty flags: a child is marked MPT_OBJ_MOVED when its parent's row is dirty
// for any reason -- so the marks run down a subtree, the children being walked in depth order -- or when it names a joint and the
// parent's pose is dirty.  One mpt_object_set_world, mpt_object_set_joints or mpt_scene_set_time moves a whole subtree and nothing else
void hierarchy_mark(mpt_ctx *c) {
    auto &an = c->anim;
    if (an.bound_children == 0) return;
    hierarchy_order(c);
    auto &rows = c->compose.rows;
    for (const int o : an.order) {
        const auto &parent = rows[rows[o].parent];
        if (parent.dirty || (rows[o].joint >= 0 && parent.pose >= 0 && c->deform.poses[parent.pose].dirty)) rows[o].dirty |= mpt_ctx::MPT_OBJ_MOVED;
    }
}

// The bound children: inside mpt_compose behind motion_step, so that every root's matrix is in the table, and behind deform_step, so
// that the palettes are in the pose buffer; in front of scatter_step and the composition, which read the matrices from the table.  A
// child is evaluated when hierarchy_mark or a call marked it, when its own row went up (the host's row holds its local matrix), and
// after a relayout.  The items go up ordered by depth; up to MPT_HIER_ONE_GROUP of them one launch walks the levels, above it each
// level evaluated is a launch.  Without a parent binding in the scene nothing is called
int hierarchy_step(mpt_ctx *c) {
    auto &an = c->anim;
    auto &cp = c->compose;
    an.hier_stats.evaluated = an.hier_stats.levels = an.hier_stats.launches = 0;
    if (an.bound_children == 0) return 0;
    hierarchy_order(c);
    an.h_hier.clear();
    MptHierLevels lv{};
    int nlevels = 0, depth = 0;
    for (const int obj : an.order) {
        const auto &row = cp.rows[obj];
        if (!cp.relayout && !(row.dirty & (mpt_ctx::MPT_OBJ_MOVED | mpt_ctx::MPT_OBJ_UPLOAD))) continue;
        if (an.depth[obj] != depth) { depth = an.depth[obj]; lv.at[nlevels++] = (int32_t)an.h_hier.size(); }
        MptHierObj o{};
        o.obj = obj; o.parent = row.parent; o.ntracks = -1; o.joint_at = -1;
        memcpy(o.local, cp.objs[obj].world, sizeof o.local);
        if (row.motion >= 0 && an.motions[row.motion].clip >= 0) {
            const auto &m = an.motions[row.motion];
            const auto &clip = an.clips[m.clip];
            o.ntracks = clip.ntracks; o.loop = m.loop; o.track_at = (int64_t)clip.track_at;
            o.offset = m.offset; o.speed = m.speed; o.t0 = clip.t0; o.t1 = clip.t1;
            memcpy(o.rest, m.rest, sizeof o.rest); memcpy(o.local, m.base, sizeof o.local);
        }
        if (row.joint >= 0) {
            const auto &p = c->deform.poses[cp.rows[row.parent].pose];
            o.joint_at = (int64_t)p.pose_at + cp.meshes[p.mesh].deform.ntargets + (int64_t)row.joint * 12;
        }
        an.h_hier.push_back(o);
    }
    const size_t n = an.h_hier.size();
    if (n == 0) return 0;
    lv.at[nlevels] = (int32_t)n;
    if (an.bufs.hier.reserve(n)) return 1;
    HIP_TRY(hipMemcpyAsync(an.bufs.hier, an.h_hier.data(), n * sizeof(MptHierObj), hipMemcpyHostToDevice, c->stream));
    const int64_t npose = (int64_t)c->deform.bufs.pose.cap;
    MptTimedSpan span(an.hier_timer, c->stream);
    HIP_TRY(span.begun);
    if (n <= MPT_HIER_ONE_GROUP) {
        HIP_TRY(mpt_launch_hierarchy_walk(an.bufs.hier, &lv, nlevels, an.time, an.bufs.tracks, an.bufs.times, an.bufs.values, c->deform.bufs.pose, npose,
                                          cp.bufs.objs, (int)cp.objs.size(), cp.epoch, c->stream));
        an.hier_stats.launches = 1;
    } else
        for (int l = 0; l < nlevels; l++) {
            HIP_TRY(mpt_launch_hierarchy_level(an.bufs.hier, lv.at[l], lv.at[l + 1], an.time, an.bufs.tracks, an.bufs.times, an.bufs.values,
                                               c->deform.bufs.pose, npose, cp.bufs.objs, (int)cp.objs.size(), cp.epoch, c->stream));
            an.hier_stats.launches++;
        }
    HIP_TRY(span.end());
    an.hier_stats.evaluated = (int64_t)n; an.hier_stats.levels = nlevels;
    return 0;
}

extern "C" int mpt_hierarchy_stats(mpt_ctx *c, mpt_hierarchy_info *out) {
    if (use_ro(c)) return 1;
    if (!out) return fail("null argument");
    const auto &rows = c->compose.rows;
    *out = c->anim.hier_stats;
    out->bound_children = c->anim.bound_children; out->deepest = 0;
    for (size_t o = 0; o < rows.size() && c->anim.bound_children; o++) {       // (nothing of the context changes)
        int64_t d = 0;
        for (int a = rows[o].parent; a >= 0 && d < MPT_HIER_MAX_DEPTH; a = rows[a].parent) d++;
        out->deepest = std::max(out->deepest, d);
    }
    return 0;
}

extern "C" int mpt_hierarchy_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->anim.hier_timer, ms, nullptr, launches);
}

// ---------------------------------------------------------------- read-backs
extern "C" int mpt_get_object_world(mpt_ctx *c, int obj_id, double *world) {
    if (use_ro(c)) return 1;
    if (check_object(c, obj_id, "mpt_get_object_world")) return 1;
    if (!world) return fail("mpt_get_object_world: null world");
    const auto &cp = c->compose;
    if (!cp.out_valid || cp.relayout || obj_id >= cp.out_objs)
        return fail("mpt_get_object_world: object %d has no row on the device yet: call mpt_compose", obj_id);
    return read_back(c, world, (const char *)(cp.bufs.objs + obj_id) + offsetof(MptComposeObj, world), 16 * sizeof(double));
}

extern "C" int mpt_anim_blend_stats(mpt_ctx *c, mpt_anim_blend_info *out) {
    if (!c || !out) return fail("null argument");
    const auto &an = c->anim;
    *out = mpt_anim_blend_info{};
    for (const auto &clip : an.clips) out->object_clips += clip.mesh < 0;
    for (const auto &p : c->deform.poses) out->blended_objects += p.clip >= 0 && p.clip_b >= 0;
    out->moved_objects = an.moved;
    out->evaluated_blended = an.evaluated_blended; out->evaluated_moved = an.evaluated_moved;
    return 0;
}

extern "C" int mpt_motion_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->anim.motion_timer, ms, nullptr, launches);
}

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

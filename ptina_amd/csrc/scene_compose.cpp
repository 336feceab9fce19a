// scene_compose.cpp -- scene composition behind mpt_mesh_add / mpt_object_* / mpt_compose: the mesh pool and
// the object table on the device, the layout and launch plan (mpt_compose_plan, a pure function), the launch of compose.hip into
// the buffers the tree builders read, and the lazy host copy of a composed model (model_on_host).  Objects of meshes that deform
// are composed from their deformed copies, which scene_deform.cpp's deform_step writes first, objects of
// meshes that carry a subdivision level from their subdivided copies, which scene_subdiv.cpp's subdiv_step writes behind it (3.19).

#include "miptina_ctx.h"

enum { CP_GROUP = 256 };                       // output vertices per workgroup (compose.hip CP_BLOCK)

extern "C" int mpt_compose_plan(const int32_t *faces, const int32_t *dirty, int nobj, int64_t *first, int64_t *wg_begin, int64_t *wg_count, int cap) {
    if (nobj < 0 || (nobj > 0 && !faces)) return -1;
    long long total = 0;
    for (int o = 0; o < nobj; o++) {
        if (faces[o] < 0) return -1;
        total += faces[o];
    }
    if (total * 3 > 0x7fffffffLL) return -1;
    int nr = 0;
    long long at = 0, end = -1;                // `end`: one past the last workgroup of the run being grown
    for (int o = 0; o < nobj; o++) {
        if (first) first[o] = at;
        const long long lo = at * 3, hi = (at + faces[o]) * 3;
        at += faces[o];
        if (faces[o] == 0 || (dirty && !dirty[o])) continue;
        const long long g0 = lo / CP_GROUP, g1 = (hi - 1) / CP_GROUP + 1;
        if (nr > 0 && g0 <= end) {             // touches or overlaps the run before: one run
            if (nr <= cap && wg_count) wg_count[nr - 1] += g1 - end;
        } else {
            if (nr < cap) {
                if (wg_begin) wg_begin[nr] = g0;
                if (wg_count) wg_count[nr] = g1 - g0;
            }
            nr++;
        }
        end = g1;
    }
    if (first) first[nobj] = at;
    return nr;
}

static int check_world(const double *w) {
    if (!w) return fail("null world matrix");
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(w[k])) return fail("world matrix entry %d is not finite", k);
    return 0;
}

static int check_mtlid(const mpt_ctx *c, int mtlid) {
    if (mtlid < -1 || mtlid >= c->caps.max_materials) return fail("material id %d outside [-1, %d)", mtlid, c->caps.max_materials);
    return 0;
}

// "[who: ]unknown <noun> <id> (<n> <nouns>)" unless 0 <= id < n
static int check_id(int id, size_t n, const char *who, const char *noun, const char *nouns) {
    if (id >= 0 && (size_t)id < n) return 0;
    return fail("%s%sunknown %s %d (%zu %s)", who ? who : "", who ? ": " : "", noun, id, n, nouns);
}

int check_mesh(const mpt_ctx *c, int mesh_id, const char *who) { return check_id(mesh_id, c->compose.meshes.size(), who, "mesh", "meshes"); }
int check_object(const mpt_ctx *c, int obj_id, const char *who) { return check_id(obj_id, c->compose.rows.size(), who, "object", "objects"); }

int check_fresh_mesh(const mpt_ctx *c, int mesh_id, const char *who) {
    if (check_mesh(c, mesh_id, who)) return 1;
    const auto &rows = c->compose.rows;
    for (size_t o = 0; o < rows.size(); o++)
        if (rows[o].mesh == mesh_id) return fail("%s: mesh %d already has an object (object %zu)", who, mesh_id, o);
    return 0;
}

int fetch_mesh(mpt_ctx *c, int mesh_id, std::vector<float> &rec) {
    const auto &m = c->compose.meshes[mesh_id];
    rec.resize((size_t)m.nfaces * 24);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (m.nfaces > 0) HIP_TRY(hipMemcpy(rec.data(), c->compose.bufs.pool + m.vert * 8, rec.size() * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mpt_mesh_add(mpt_ctx *c, const float *verts, int k, int *mesh_id) {
    if (use(c)) return 1;
    if (k < 0 || (k > 0 && !verts)) return fail("bad mesh arguments");
    if (k >= c->caps.max_faces) return fail("too many faces");
    auto &cp = c->compose;
    if (cp.pool_verts + (size_t)k * 3 > 0x7fffffffu) return fail("mesh pool full: %zu vertices held", cp.pool_verts);   // (MptComposeObj::mesh_vert)
    const size_t floats = (size_t)k * 24;
    if (cp.bufs.grow_pool((cp.pool_verts + (size_t)k * 3) * 8, cp.pool_verts * 8, c->stream)) return 1;
    if (k > 0) {
        HIP_TRY(hipMemcpyAsync(cp.bufs.pool + cp.pool_verts * 8, verts, floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));      // the caller's array is borrowed for the call
    }
    cp.meshes.push_back({ cp.pool_verts, k, {}, {} });       // its whole row: no targets, no skin, no level yet
    cp.pool_verts += (size_t)k * 3;
    c->deform.room.lose(c->deform.poses, cp.relayout);     // it lies where the copies behind the meshes lay
    c->subdiv.room.lose(c->subdiv.copies, cp.relayout);
    if (mesh_id) *mesh_id = (int)cp.meshes.size() - 1;
    return 0;
}

int add_object(mpt_ctx *c, int mesh_id, const double *world, int mtlid, int scatter) {
    auto &cp = c->compose;
    const int obj = (int)cp.objs.size();
    MptComposeObj o{};
    o.nfaces = subdiv_object_faces(c, mesh_id); o.mesh_vert = (int32_t)cp.meshes[mesh_id].vert; o.mtlid = mtlid;
    if (world) memcpy(o.world, world, sizeof o.world);
    else for (int d = 0; d < 4; d++) o.world[5 * d] = 1.0;
    cp.objs.push_back(o);
    cp.rows.push_back({ mesh_id, -1, -1, scatter, mpt_ctx::MPT_OBJ_UPLOAD });
    cp.relayout = true;
    deform_object_added(c, obj);
    subdiv_object_added(c, obj);
    return obj;
}

extern "C" int mpt_object_add(mpt_ctx *c, int mesh_id, const double world[16], int mtlid, int *obj_id) {
    if (use(c)) return 1;
    if (check_mesh(c, mesh_id, nullptr) || check_world(world) || check_mtlid(c, mtlid)) return 1;
    const int obj = add_object(c, mesh_id, world, mtlid, -1);
    if (obj_id) *obj_id = obj;
    return 0;
}

extern "C" int mpt_object_set_world(mpt_ctx *c, int obj_id, const double world[16]) {
    if (use(c)) return 1;
    if (check_object(c, obj_id, nullptr) || check_world(world)) return 1;
    auto &row = c->compose.rows[obj_id];
    if (row.scatter >= 0)
        return fail("mpt_object_set_world: object %d is an instance of scatter %d, which places it on its surface", obj_id, row.scatter);
    if (row.motion >= 0 && c->anim.motions[row.motion].clip >= 0)
        return fail("mpt_object_set_world: object %d is bound to object clip %d, which gives its matrix: unbind it first (mpt_object_set_motion with clip -1)",
                    obj_id, c->anim.motions[row.motion].clip);
    memcpy(c->compose.objs[obj_id].world, world, sizeof(double) * 16);
    row.dirty = mpt_ctx::MPT_OBJ_UPLOAD;
    return 0;
}

extern "C" int mpt_object_set_material(mpt_ctx *c, int obj_id, int mtlid) {
    if (use(c)) return 1;
    if (check_object(c, obj_id, nullptr) || check_mtlid(c, mtlid)) return 1;
    c->compose.objs[obj_id].mtlid = mtlid;
    c->compose.rows[obj_id].dirty = mpt_ctx::MPT_OBJ_UPLOAD;
    return 0;
}

extern "C" int mpt_scene_clear(mpt_ctx *c, int meshes) {
    if (use(c)) return 1;
    auto &cp = c->compose;
    cp.objs.clear(); cp.rows.clear();
    cp.relayout = true;
    if (meshes) { cp.meshes.clear(); cp.pool_verts = 0; }
    deform_scene_cleared(c, meshes);
    anim_scene_cleared(c, meshes);
    subdiv_scene_cleared(c, meshes);
    scatter_scene_cleared(c);
    return 0;
}

// scene_cen / scene_rad from the box of the positions: mpt_load_model's expressions on the same six numbers
static void bounding_sphere(mpt_ctx *c, int n, const double lo[3], const double hi[3]) {
    double r2 = 0;
    for (int k = 0; k < 3; k++) { c->scene_cen[k] = n ? 0.5 * (lo[k] + hi[k]) : 0.0; r2 += n ? 0.25 * (hi[k] - lo[k]) * (hi[k] - lo[k]) : 0.0; }
    c->scene_rad = std::sqrt(r2);
    if (!std::isfinite(c->scene_rad)) c->scene_rad = 1e30;
}

// The model's buffers, set aside by take() while mpt_compose grows new ones and may still refuse: they come back when the scope ends,
// unless drop() let them go first
struct KeptModel : MptNoCopy {
    MptModelBufs &model; MptModelBufs kept; bool taken = false;
    explicit KeptModel(MptModelBufs &m) : model(m) {}
    ~KeptModel() { if (taken) exchange(); }
    void exchange() { kept.d_verts.swap(model.d_verts); kept.d_mtlids.swap(model.d_mtlids); std::swap(kept.cap, model.cap); }
    void take() { exchange(); taken = true; }
    void drop() { taken = false; }
};

extern "C" int mpt_compose(mpt_ctx *c) {
    if (use(c)) return 1;
    auto &cp = c->compose;
    const int nobj = (int)cp.objs.size();
    hierarchy_mark(c);                                // a dirty parent's children are dirty (scene_anim.cpp): before anything reads the flags
    std::vector<int32_t> faces(nobj), dirty(nobj);
    long long total = 0;
    for (int o = 0; o < nobj; o++) { faces[o] = cp.objs[o].nfaces; total += faces[o]; }
    if (total >= c->caps.max_faces) return fail("too many faces");            // model.py:84
    if (subdiv_images_ready(c)) return 1;             // (a displaced copy whose image is not loaded: nothing has changed yet)
    if (scatter_ready(c)) return 1;                   // (a scatter whose surface has no faces or whose density image is not loaded: the same)
    const int n = (int)total, nverts = n * 3;
    HIP_TRY(hipStreamSynchronize(c->stream));
    bool replaced = false;
    // A compose that selects may still refuse a surface without weight once the weights are there: a model that has to grow keeps
    // its old buffers until then, and takes them back at a refusal (the composed model stays as it was)
    KeptModel kept(c->dmodel);
    if (scatter_selection_due(c) && (size_t)std::max(n, 1) > c->dmodel.cap) kept.take();
    if (c->dmodel.reserve(std::max(n, 1), &replaced)) return 1;
    const size_t groups = mpt_compose_groups((size_t)nverts);
    if (groups * 6 > cp.bufs.part.cap) { replaced = true; if (cp.bufs.part.reserve(groups * 6)) return 1; }
    if (nobj > 0 && (size_t)nobj > cp.bufs.objs.cap) { cp.relayout = true; if (cp.bufs.reserve_table((size_t)nobj)) return 1; }
    if (deform_step(c)) return 1;                     // the deformed copies first: compose_kernel reads them as meshes (scene_deform.cpp)
    if (subdiv_step(c)) return 1;                     // ... then the subdivided copies, of meshes and of deformed copies (scene_subdiv.cpp)
    scatter_mark(c);                                  // ... and the instances of the scatters that place are composed again (scene_scatter.cpp)
    const bool all = cp.relayout || replaced || !cp.out_valid;
    cp.epoch++;
    int ndirty = 0; long long recomposed = 0;
    for (int o = 0; o < nobj; o++) {
        dirty[o] = all || (cp.rows[o].dirty & mpt_ctx::MPT_OBJ_COMPOSE);
        if (!dirty[o]) continue;
        ndirty++; recomposed += faces[o];
        cp.objs[o].epoch = cp.epoch;
    }
    std::vector<int64_t> first(nobj + 1), wg_begin(std::max(nobj, 1)), wg_count(std::max(nobj, 1));
    const int nruns = mpt_compose_plan(faces.data(), all ? nullptr : dirty.data(), nobj, first.data(), wg_begin.data(), wg_count.data(), nobj);
    if (nruns < 0) return fail("too many faces");
    // the table: after a change of layout all of it and the first faces; else the changed records alone (160 bytes each)
    std::vector<int32_t> first32(nobj);
    for (int o = 0; o < nobj; o++) { cp.objs[o].first_face = (int32_t)first[o]; first32[o] = (int32_t)first[o]; }
    if (cp.relayout && nobj > 0) {
        HIP_TRY(hipMemcpyAsync(cp.bufs.objs, cp.objs.data(), (size_t)nobj * sizeof(MptComposeObj), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(cp.bufs.first, first32.data(), (size_t)nobj * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    } else {
        for (int o = 0; o < nobj; o++)
            if (cp.rows[o].dirty & mpt_ctx::MPT_OBJ_UPLOAD)   // (MPT_OBJ_PLACED or _MOVED alone: a row whose matrix the device writes)
                HIP_TRY(hipMemcpyAsync(cp.bufs.objs + o, &cp.objs[o], sizeof(MptComposeObj), hipMemcpyHostToDevice, c->stream));
    }
    std::vector<MptRun> runs((size_t)std::max(nruns, 1));
    int blocks = 0;
    for (int r = 0; r < nruns; r++) { runs[r] = { (int32_t)wg_begin[r], blocks }; blocks += (int)wg_count[r]; }
    if (!all && nruns > 0)
        HIP_TRY(hipMemcpyAsync(cp.bufs.runs, runs.data(), (size_t)nruns * sizeof(MptRun), hipMemcpyHostToDevice, c->stream));
    // the moved objects' matrices (scene_anim.cpp): behind the table's upload, which would overwrite them, and in front of the scatters,
    // whose kernels read their surfaces' matrices from the table
    if (motion_step(c)) return 1;
    // ... and the bound children's, level by level: behind their roots' matrices and the palettes, which deform_step left in the pose buffer
    if (hierarchy_step(c)) return 1;
    // the scatters' launches: behind the table's upload, which would overwrite the matrices they write, and before the composition
    if (scatter_step(c)) return 1;
    kept.drop();
    if (n > 0) {
        MptTimedSpan span(cp.timer, c->stream);
        HIP_TRY(span.begun);
        HIP_TRY(mpt_launch_compose(cp.bufs.pool, cp.bufs.objs, cp.bufs.first, nobj, nverts, cp.bufs.runs, nruns, all ? (int)groups : blocks,
                                   all ? 1 : 0, cp.epoch, c->dmodel.d_verts, c->dmodel.d_mtlids, cp.bufs.part, cp.bounds.dev, c->stream));
        HIP_TRY(span.end());
    }
    HIP_TRY(hipStreamSynchronize(c->stream));          // (also: the uploads above read host vectors that end with this call)
    cp.relayout = false; cp.out_valid = true; cp.out_objs = nobj;
    c->nfaces = n;
    c->max_mtlid = -1;
    for (int o = 0; o < nobj; o++) {
        cp.rows[o].dirty = mpt_ctx::MPT_OBJ_CLEAN;
        if (faces[o] > 0) c->max_mtlid = std::max(c->max_mtlid, (int)cp.objs[o].mtlid);
    }
    {   // mpt_load_model's box: a loop that starts from +-1e300 and never takes a NaN; the device's starts from +-infinity
        double lo[3], hi[3];
        for (int k = 0; k < 3; k++) {
            const float l = cp.bounds.host[k], h = cp.bounds.host[3 + k];
            const bool none = n == 0 || l > h;                                 // no position that is a number
            lo[k] = none ? 1e300 : (double)l; hi[k] = none ? -1e300 : (double)h;
        }
        bounding_sphere(c, n, lo, hi);
    }
    c->tree_valid = false;
    c->d_model_stale = false;
    c->h_model_stale = true;
    cp.stats.faces = n; cp.stats.recomposed = recomposed; cp.stats.dirty_objects = ndirty;
    return 0;
}

// Before anything reads c->verts / c->mtlids.  After mpt_load_model the host copy is the model and nothing happens; after
// mpt_compose the model is fetched from the device, once (modelled on download_tree, tree_build.cpp)
int model_on_host(mpt_ctx *c) {
    if (!c->h_model_stale) return 0;
    const size_t n = (size_t)c->nfaces;
    c->verts.resize(n * 24); c->mtlids.resize(n);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n > 0) {
        HIP_TRY(hipMemcpy(c->verts.data(), c->dmodel.d_verts, n * 24 * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c->mtlids.data(), c->dmodel.d_mtlids, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    c->h_model_stale = false;
    c->compose.stats.host_fetches++;
    return 0;
}

extern "C" int mpt_compose_stats(mpt_ctx *c, mpt_compose_info *out) {
    if (!c || !out) return fail("null argument");
    *out = c->compose.stats;
    out->faces = c->nfaces;
    for (int k = 0; k < 3; k++) out->scene_cen[k] = c->scene_cen[k];
    out->scene_rad = c->scene_rad;
    return 0;
}

extern "C" int mpt_get_model(mpt_ctx *c, float *verts, int32_t *mtlids, int cap_faces, int *nfaces) {
    if (use_ro(c)) return 1;
    if (nfaces) *nfaces = c->nfaces;
    if (!verts && !mtlids) return 0;
    if (cap_faces < c->nfaces) return fail("mpt_get_model: room for %d faces, the model has %d", cap_faces, c->nfaces);
    if (model_on_host(c)) return 1;
    if (verts) memcpy(verts, c->verts.data(), (size_t)c->nfaces * 24 * sizeof(float));
    if (mtlids) memcpy(mtlids, c->mtlids.data(), (size_t)c->nfaces * sizeof(int32_t));
    return 0;
}

int read_copy(mpt_ctx *c, long long copy_vert, bool stale, int k, int obj_id, float *verts, int cap_faces, const char *who, const char *noun,
              const char *mesh) {
    if (copy_vert < 0 || stale) return fail("%s: object %d has no %s copy yet: call mpt_compose", who, obj_id, noun);
    if (cap_faces < k) return fail("%s: room for %d faces, the %s of object %d has %d", who, cap_faces, mesh, obj_id, k);
    if (k > 0 && !verts) return fail("%s: null verts", who);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (k > 0) HIP_TRY(hipMemcpy(verts, c->compose.bufs.pool + (size_t)copy_vert * 8, (size_t)k * 24 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int mpt_compose_kernel_time(mpt_ctx *c, double *ms, int *launches) {
    return use_ro(c) || timer_readout(c, c->compose.timer, ms, nullptr, launches);
}

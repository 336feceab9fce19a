'''
triangle mesh model storage (reference model.py).  The mesh is kept on the host until
BVHTree().build() packs it, leaf-ordered, into the device records (csrc/mpt_types.h) -- or, through
load_meshes / add_mesh / add_object / compose, object-space meshes and an object table are kept on the device
and composed there into the model the build reads (csrc/compose.hip); a mesh may carry morph
targets and a skin, and its objects a pose each, deformed there too (csrc/deform.hip), and a Loop
subdivision level, evaluated there behind the deformation (csrc/subdiv.hip), and a subdivided mesh a
texture displacement behind that (csrc/displace.hip); and instances of a mesh may be scattered over an
object, placed there on the device and placed again when the object moves (csrc/scatter.hip).
'''

import ctypes as C

from .common import *                 # noqa: F401,F403
from .common import Singleton, register, ctx, np
from ._lib import fptr, iptr, ComposeInfo, DeformInfo, AnimInfo, SubdivInfo, DisplaceInfo, DEFORM_MAX_JOINTS, DEFORM_MAX_TARGETS, SUBDIV_MAX_LEVELS
from ._lib import SUBDIV_SCHEMES, DISPLACE_MODES, DISPLACE_CHANNELS, ScatterInfo, ScatterSpacingInfo, SCATTER_POINT_DTYPE, scatter_params, scatter_spacing


@register
class ModelPool(metaclass=Singleton):
    def __init__(self, size=2**21):
        self.size = size
        self._nfaces = 0
        self._vertices = np.zeros((0, 8), np.float32)
        self._mtlids = np.zeros(0, np.int32)
        self._composed = False           # the model is the device's composition: to_numpy fetches it
        self._mesh_faces = []            # faces of every mesh of the device's pool
        self._mesh_levels = {}           # mesh -> its subdivision level, where it has one: an object of it has faces * 4^level
        self._mesh_corners = {}          # mesh -> the corners of its polygons, where its scheme is Catmull-Clark: an object has 2 * corners * 4^(level - 1) faces
        self._mesh_displace = {}         # mesh -> [strength, midlevel] of its displacement, where it has one
        self._obj_mesh = []              # the mesh of every object of the device's table
        self._sum = (None, 0, 0)         # (that list, how many of its objects are counted, their faces): _faces_of_objects
        self._scatters = []              # per scatter: its surface, its mesh, its range of objects, its seed and parameters
        self._mesh_pose = {}             # mesh -> (morph targets, joints of its skin), where it is deformable: the shape of an object's pose

    @property
    def nfaces(self):
        return self._nfaces

    def to_numpy(self, id=None):
        if self._composed:               # (the library fetches its host copy of a composed model once, when somebody asks)
            arr, mtlids = np.empty((self._nfaces * 3, 8), np.float32), np.empty(self._nfaces, np.int32)
            ctx().call('mpt_get_model', fptr(arr), iptr(mtlids), self._nfaces, None)
            return arr, mtlids
        return self._vertices.copy(), self._mtlids.copy()

    def from_numpy(self, arr, mtlids):
        arr = np.ascontiguousarray(arr, np.float32)
        mtlids = np.ascontiguousarray(mtlids, np.int32)
        ctx().call('mpt_load_model', fptr(arr), iptr(mtlids), int(mtlids.shape[0]))
        self._vertices, self._mtlids = arr, mtlids
        self._nfaces = int(mtlids.shape[0])
        self._composed = False

    # ---- composition on the device (no reference counterpart: its add-on composes on the host at every scene change,
    #      blender.py:555-571; the arithmetic is multimesh.py:58-65)
    @staticmethod
    def _world(world):
        w = np.ascontiguousarray(world, np.float64)
        if w.shape != (4, 4):
            raise ValueError('world matrix must be 4x4, got shape %s' % (w.shape,))
        if not np.isfinite(w).all():
            raise ValueError('world matrix has an entry that is not finite')
        return w

    def _object(self, obj):
        if not 0 <= int(obj) < len(self._obj_mesh):
            raise ValueError('unknown object %r (%d objects)' % (obj, len(self._obj_mesh)))
        return int(obj)

    def add_mesh(self, p, n, t=None):
        '''a mesh for the device's pool: positions p [k,3,3], normals n [k,3,3], texcoords t [k,3,2] or None (zeros per corner, as
        multimesh.compose_multiple_meshes decides), in object space.  Stored as f32: f64 input is rounded here, at the upload,
        where compose_multiple_meshes + load round after the transform.  Returns the mesh id'''
        p, n = np.asarray(p), np.asarray(n)
        k = p.shape[0] if p.ndim else -1
        if p.shape != (k, 3, 3) or n.shape != (k, 3, 3):
            raise ValueError('positions and normals must be [k,3,3], got %s and %s' % (p.shape, n.shape))
        t = np.zeros((k, 3, 2), np.float32) if t is None else np.asarray(t)
        if t.shape != (k, 3, 2):
            raise ValueError('texcoords must be [%d,3,2], got %s' % (k, t.shape))
        if k >= self.size:
            raise ValueError('too many faces: a mesh of %d, room for fewer than %d' % (k, self.size))
        rec = np.ascontiguousarray(np.concatenate([p.reshape(k * 3, 3), n.reshape(k * 3, 3), t.reshape(k * 3, 2)], axis=1), np.float32)
        mesh = C.c_int(-1)
        ctx().call('mpt_mesh_add', fptr(rec), k, C.byref(mesh))
        self._mesh_faces.append(k)
        assert mesh.value == len(self._mesh_faces) - 1
        return mesh.value

    def add_object(self, mesh, world, mtlid=None):
        '''an object of the table: mesh `mesh` placed by the 4x4 matrix `world`, with material id mtlid (None: -1, the default
        material).  Objects are composed in the order they were added.  Returns the object id'''
        if not 0 <= int(mesh) < len(self._mesh_faces):
            raise ValueError('unknown mesh %r (%d meshes)' % (mesh, len(self._mesh_faces)))
        w = self._world(world)
        total = self._faces_of_objects() + self._object_faces(int(mesh))
        if total >= self.size:
            raise ValueError('too many faces: %d with this object, room for fewer than %d' % (total, self.size))
        obj = C.c_int(-1)
        ctx().call('mpt_object_add', int(mesh), w.ctypes.data_as(C.POINTER(C.c_double)), -1 if mtlid is None else int(mtlid), C.byref(obj))
        self._obj_mesh.append(int(mesh))
        assert obj.value == len(self._obj_mesh) - 1
        return obj.value

    def set_world(self, obj, world):
        '''move an object; the next compose() rewrites its faces only'''
        obj, w = self._object(obj), self._world(world)
        ctx().call('mpt_object_set_world', obj, w.ctypes.data_as(C.POINTER(C.c_double)))

    def set_material(self, obj, mtlid):
        obj = self._object(obj)
        ctx().call('mpt_object_set_material', obj, -1 if mtlid is None else int(mtlid))

    def clear_objects(self):
        '''drop the objects; the meshes stay in the pool'''
        ctx().call('mpt_scene_clear', 0)
        self._obj_mesh, self._scatters = [], []

    def clear_meshes(self):
        '''drop the objects and the meshes'''
        ctx().call('mpt_scene_clear', 1)
        self._obj_mesh, self._mesh_faces, self._mesh_levels, self._mesh_displace, self._scatters = [], [], {}, {}, []
        self._mesh_corners, self._mesh_pose = {}, {}

    def compose(self):
        '''write the objects, in order, as the model BVHTree().build() reads -- on the device; what load(*compose_multiple_meshes(...))
        leaves, without the arrays crossing to the host and back.  After set_world / set_material only the changed objects' faces
        are rewritten'''
        ctx().call('mpt_compose')
        self._nfaces = self._faces_of_objects()
        self._composed = True

    # ---- deformation on the device: glTF 2.0's morph targets and linear-blend skinning (csrc/deform.hip, DESIGN.md section 3.17;
    #      no reference counterpart)
    def _fresh_mesh(self, mesh):
        if not 0 <= int(mesh) < len(self._mesh_faces):
            raise ValueError('unknown mesh %r (%d meshes)' % (mesh, len(self._mesh_faces)))
        if int(mesh) in self._obj_mesh:
            raise ValueError('mesh %d already has an object: targets and skins come first' % int(mesh))
        return int(mesh)

    def add_morph_targets(self, mesh, dp, dn=None):
        '''T morph targets for a mesh that has no object yet: position deltas dp [T,k,3,3] and normal deltas dn (None: zeros), per
        face corner, stored as f32.  Objects of the mesh start with all weights 0'''
        mesh = self._fresh_mesh(mesh)
        dp = np.asarray(dp)
        k = self._mesh_faces[mesh]
        T = dp.shape[0] if dp.ndim == 4 else -1
        if dp.shape != (T, k, 3, 3):
            raise ValueError('position deltas must be [T,%d,3,3], got %s' % (k, dp.shape))
        dn = np.zeros(dp.shape, np.float32) if dn is None else np.asarray(dn)
        if dn.shape != dp.shape:
            raise ValueError('normal deltas must be %s, got %s' % (dp.shape, dn.shape))
        if not 1 <= T <= DEFORM_MAX_TARGETS:
            raise ValueError('%d morph targets: between 1 and %d' % (T, DEFORM_MAX_TARGETS))
        rec = np.ascontiguousarray(np.concatenate([dp.reshape(T, k * 3, 3), dn.reshape(T, k * 3, 3)], axis=2), np.float32)
        ctx().call('mpt_mesh_set_morph', mesh, fptr(rec), T)
        self._mesh_pose[mesh] = (T, self._mesh_pose.get(mesh, (0, 0))[1])

    def add_skin(self, mesh, joints, weights, njoints=None):
        '''a skin for a mesh that has no object yet: joint indices (any integer type) and weights [k,3,4] per face corner, over
        njoints joints (None: the largest index + 1).  Weights are stored as f32 and used as given, not renormalised.  Objects of the
        mesh start with identity joint matrices'''
        mesh = self._fresh_mesh(mesh)
        joints, weights = np.asarray(joints), np.asarray(weights)
        k = self._mesh_faces[mesh]
        if joints.shape != (k, 3, 4) or weights.shape != (k, 3, 4):
            raise ValueError('joints and weights must be [%d,3,4], got %s and %s' % (k, joints.shape, weights.shape))
        if not np.issubdtype(joints.dtype, np.integer):
            raise ValueError('joints must be integers, got %s' % joints.dtype)
        if njoints is None:
            njoints = int(joints.max()) + 1 if joints.size else 1
        njoints = int(njoints)
        if not 1 <= njoints <= DEFORM_MAX_JOINTS:
            raise ValueError('%d joints: between 1 and %d' % (njoints, DEFORM_MAX_JOINTS))
        if joints.size and (int(joints.min()) < 0 or int(joints.max()) >= njoints):      # (before the cast: it would wrap)
            raise ValueError('joint indices must lie in [0, %d), got %d .. %d' % (njoints, int(joints.min()), int(joints.max())))
        j = np.ascontiguousarray(joints.reshape(k * 3, 4), np.uint16)
        w = np.ascontiguousarray(weights.reshape(k * 3, 4), np.float32)
        ctx().call('mpt_mesh_set_skin', mesh, j.ctypes.data_as(C.POINTER(C.c_uint16)), fptr(w), njoints)
        self._mesh_pose[mesh] = (self._mesh_pose.get(mesh, (0, 0))[0], njoints)

    def set_morph_weights(self, obj, w):
        '''the morph weights [T] of an object; the next compose() deforms and rewrites this object only'''
        obj = self._object(obj)
        w = np.ascontiguousarray(w, np.float64).reshape(-1)
        ctx().call('mpt_object_set_morph_weights', obj, w.ctypes.data_as(C.POINTER(C.c_double)), int(w.size))

    def set_joints(self, obj, mats):
        '''the joint matrices [njoints,4,4] of an object (tools.skin.joint_matrices makes them: globalJoint . inverseBind, affine, in
        the object's space); the next compose() deforms and rewrites this object only'''
        obj = self._object(obj)
        m = np.ascontiguousarray(mats, np.float64)
        if m.ndim != 3 or m.shape[1:] != (4, 4):
            raise ValueError('joint matrices must be [njoints,4,4], got shape %s' % (m.shape,))
        ctx().call('mpt_object_set_joints', obj, m.ctypes.data_as(C.POINTER(C.c_double)), int(m.shape[0]))

    def _copy_to_numpy(self, symbol, obj, faces_of):
        '''the read-back of an object's derived copy in the pool: [3 faces_of(its mesh), 8] f32'''
        obj = self._object(obj)
        k = faces_of(self._obj_mesh[obj])
        arr = np.empty((k * 3, 8), np.float32)
        ctx().call(symbol, obj, fptr(arr), k)
        return arr

    def deformed_to_numpy(self, obj):
        '''the deformed copy of a deformable object as the last compose() wrote it: [3k,8] f32 records in object space'''
        return self._copy_to_numpy('mpt_get_deformed', obj, lambda mesh: self._mesh_faces[mesh])

    def deform_stats(self):
        '''_lib.DeformInfo: deformable objects, objects and corners the last compose() deformed, pool vertices the copies hold'''
        info = DeformInfo()
        ctx().call('mpt_deform_stats', C.byref(info))
        return info

    # ---- keyframe animation on the device: glTF 2.0's animations, evaluated where the poses lie (csrc/anim.hip, DESIGN.md section
    #      3.17.1; no reference counterpart).  tools/anim.py writes clips by hand; reading them from files is not part of it
    def add_skeleton(self, mesh, parents, rest_translation, rest_rotation, rest_scale, inverse_bind):
        '''the skeleton of a skinned mesh that has no object yet, behind add_skin: parents [nj] (-1: a root; parents come before their
        children), the joints' rest pose -- translations [nj,3], rotations [nj,4] as x y z w, scales [nj,3] -- and the skin's inverse
        bind matrices [nj,4,4] (affine) or [nj,3,4], all f64'''
        mesh = self._fresh_mesh(mesh)
        parents = np.asarray(parents)
        if parents.ndim != 1 or (parents.size and not np.issubdtype(parents.dtype, np.integer)):
            raise ValueError('parents must be [nj] integers, got %s of %s' % (parents.shape, parents.dtype))
        nj = int(parents.size)
        t, r, sc = (np.asarray(a, np.float64) for a in (rest_translation, rest_rotation, rest_scale))
        if t.shape != (nj, 3) or r.shape != (nj, 4) or sc.shape != (nj, 3):
            raise ValueError('the rest pose must be [%d,3], [%d,4] and [%d,3], got %s, %s and %s' % (nj, nj, nj, t.shape, r.shape, sc.shape))
        ib = np.asarray(inverse_bind, np.float64)
        if ib.shape == (nj, 4, 4):
            if not np.array_equal(ib[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (nj, 1))):
                raise ValueError('the bottom row of an inverse_bind matrix is not 0 0 0 1 (not affine)')
            ib = ib[:, :3]
        if ib.shape != (nj, 3, 4):
            raise ValueError('inverse_bind must be [%d,4,4] or [%d,3,4], got %s' % (nj, nj, ib.shape))
        rest = np.ascontiguousarray(np.concatenate([t, r, sc], axis=1))
        ib = np.ascontiguousarray(ib)
        dp = C.POINTER(C.c_double)
        ctx().call('mpt_mesh_set_skeleton', mesh, nj, iptr(np.ascontiguousarray(parents, np.int32)), rest.ctypes.data_as(dp), ib.ctypes.data_as(dp))

    def add_clip(self, mesh, tracks):
        '''a clip for a deformable mesh that has no object yet (a skinned one: behind add_skeleton): a list of tools.anim.track(...)
        -- at most one per (target, path).  Returns the clip id, which counts over all meshes'''
        from .tools.anim import pack_clip
        mesh = self._fresh_mesh(mesh)
        spec, times, values = pack_clip(tracks)
        clip = C.c_int(-1)
        ctx().call('mpt_mesh_add_clip', mesh, spec.shape[0], iptr(spec), fptr(times), times.size, fptr(values), values.size, C.byref(clip))
        return clip.value

    def set_animation(self, obj, clip, offset=0.0, speed=1.0, loop=True):
        '''bind an object to a clip of its mesh: at scene time t it is posed at the clip's time (t - offset) * speed, wrapped into the
        clip's span if loop, else clamped track by track.  clip=None unbinds: the pose is again what set_joints / set_morph_weights
        last gave (which refuse a bound object).  The next compose() poses, deforms and rewrites this object'''
        obj = self._object(obj)
        ctx().call('mpt_object_set_animation', obj, -1 if clip is None else int(clip), float(offset), float(speed), int(bool(loop)))

    def set_time(self, t):
        '''the scene's time: the next compose() poses every bound object there, in one launch on the device; the same time again
        changes nothing'''
        ctx().call('mpt_scene_set_time', float(t))

    def pose_to_numpy(self, obj):
        '''(weights [T], palette [nj,3,4]) f64: a deformable object's pose as it lies on the device after the last compose(), bound
        to a clip or not'''
        obj = self._object(obj)
        T, nj = self._mesh_pose.get(self._obj_mesh[obj], (0, 0))
        pose = np.zeros(max(T + 12 * nj, 1), np.float64)
        ctx().call('mpt_get_pose', obj, pose.ctypes.data_as(C.POINTER(C.c_double)), T + 12 * nj)
        return pose[:T].copy(), pose[T:T + 12 * nj].reshape(nj, 3, 4).copy()

    def anim_stats(self):
        '''_lib.AnimInfo: skeletons, clips and tracks of the scene, bound objects, objects the last compose() posed on the device'''
        info = AnimInfo()
        ctx().call('mpt_anim_stats', C.byref(info))
        return info

    # ---- two clips blended, and objects moved by clips
    def set_animation_blend(self, obj, clip, offset=0.0, speed=1.0, loop=True, weight=1.0, fade=None):
        '''the second binding of an object that set_animation has bound: `clip`, another clip of its mesh, is evaluated at its own
        (t - offset) * speed and mixed in by a weight in [0, 1] -- `weight` a number, or (w0, w1) with fade=(start, duration): w0 until
        scene time `start`, then linearly to w1 over `duration` (0: at once), so that a cross-fade costs nothing per frame but
        set_time.  Weight 0 is the first clip's pose, 1 this one's, bit for bit.  clip=None or -1 removes the second binding;
        set_animation(obj, None) removes both'''
        from ._lib import blend_weights
        obj = self._object(obj)
        ctx().call('mpt_object_set_animation_blend', obj, -1 if clip is None else int(clip), float(offset), float(speed), int(bool(loop)),
                   *blend_weights(weight, fade))

    def add_object_clip(self, tracks):
        '''a clip that moves objects, at any time: a list of tools.anim.track(0, 'T' | 'R' | 'S', ...), target 0 being the object's
        node -- at most one per path.  Returns the clip id, which counts on over the meshes' clips'''
        from .tools.anim import pack_clip
        spec, times, values = pack_clip(tracks)
        clip = C.c_int(-1)
        ctx().call('mpt_scene_add_object_clip', spec.shape[0], iptr(spec), fptr(times), times.size, fptr(values), values.size, C.byref(clip))
        return clip.value

    def set_motion(self, obj, clip, offset=0.0, speed=1.0, loop=True, rest=None, base=None):
        '''bind an object -- any but an instance of a scatter -- to an object clip: at scene time t its world matrix is
        base . T R S, with T, R and S the clip's tracks at (t - offset) * speed and, for a path without a track, those of `rest`
        (translation3 rotation4 xyzw scale3; None: 0 0 0, 0 0 0 1, 1 1 1); `base` [4,4] is the node's static parents (None: the
        identity).  The device writes the matrix: set_world refuses the object until clip=None or -1 unbinds it, which returns it to
        the matrix add_object / set_world last gave'''
        obj = self._object(obj)
        dp = C.POINTER(C.c_double)
        rest = None if rest is None else np.ascontiguousarray(rest, np.float64).reshape(-1)
        base = None if base is None else np.ascontiguousarray(base, np.float64).reshape(-1)
        if rest is not None and rest.size != 10:
            raise ValueError('rest must hold 10 numbers (translation3 rotation4 scale3), got %d' % rest.size)
        if base is not None and base.size != 16:
            raise ValueError('base must be [4,4], got %d numbers' % base.size)
        ctx().call('mpt_object_set_motion', obj, -1 if clip is None else int(clip), float(offset), float(speed), int(bool(loop)),
                   None if rest is None else rest.ctypes.data_as(dp), None if base is None else base.ctypes.data_as(dp))

    def world_to_numpy(self, obj):
        '''[4,4] f64: an object's world matrix as it lies on the device after the last compose(), moved by a clip or not'''
        obj = self._object(obj)
        world = np.zeros((4, 4), np.float64)
        ctx().call('mpt_get_object_world', obj, world.ctypes.data_as(C.POINTER(C.c_double)))
        return world

    def anim_blend_stats(self):
        '''_lib.AnimBlendInfo: object clips, objects with a second binding, objects with a motion binding, and how many of each the last
        compose() evaluated on the device'''
        from ._lib import AnimBlendInfo
        info = AnimBlendInfo()
        ctx().call('mpt_anim_blend_stats', C.byref(info))
        return info

    # ---- objects parented to objects and to joints (csrc/hierarchy.hip)
    def set_parent(self, obj, parent, joint=None):
        '''bind an object -- any but an instance of a scatter -- to a parent object, and with `joint` to joint `joint` of the parent's
        pose.  The object's own matrix (add_object / set_world, which stays allowed; or its motion binding's base . T R S) is from then
        on its LOCAL matrix, and compose() writes world(child) = world(parent) . local, or world(parent) . (M_joint . local) with the
        skinning matrix pose_to_numpy(parent) returns, on the device: the child moves as a vertex skinned to the joint with weight 1
        (tools.skin.attach folds the joint's bind matrix into a local given in the joint's frame).  One set_world, set_joints or
        set_time moves a whole subtree.  parent=None unparents: the object's matrix is its world again.  Refused: a cycle, an instance
        of a scatter on either side, a joint the parent's skin does not have, a chain deeper than 64'''
        obj = self._object(obj)
        parent = -1 if parent is None else self._object(parent)
        ctx().call('mpt_object_set_parent', obj, parent, -1 if joint is None else int(joint))

    def parent_of(self, obj):
        '''(parent, joint) of a bound object, joint None for the parent itself; None for an object without a parent'''
        obj = self._object(obj)
        parent, joint = C.c_int(-1), C.c_int(-1)
        ctx().call('mpt_object_get_parent', obj, C.byref(parent), C.byref(joint))
        return None if parent.value < 0 else (parent.value, None if joint.value < 0 else joint.value)

    def hierarchy_stats(self):
        '''_lib.HierarchyInfo: bound children and the deepest chain; the children the last compose() evaluated on the device, over how
        many levels, in how many launches'''
        from ._lib import HierarchyInfo
        info = HierarchyInfo()
        ctx().call('mpt_hierarchy_stats', C.byref(info))
        return info

    # ---- Loop subdivision on the device, behind the deformation (csrc/subdiv.hip; the reference's add-on
    #      is handed Blender's evaluated mesh instead)
    def _object_faces(self, mesh):
        if mesh in self._mesh_corners:
            return 2 * self._mesh_corners[mesh] << (2 * (self._mesh_levels[mesh] - 1))
        return self._mesh_faces[mesh] << (2 * self._mesh_levels.get(mesh, 0))

    def _faces_of_objects(self):
        '''the faces of all objects.  A mesh with an object keeps its face count and objects only join the list, so the sum is
        carried along: a scatter adds thousands of objects, and compose() asks every time'''
        objs, n, total = self._sum
        if objs is not self._obj_mesh or n > len(self._obj_mesh):
            n, total = 0, 0
        total += sum(self._object_faces(m) for m in self._obj_mesh[n:])
        self._sum = (self._obj_mesh, len(self._obj_mesh), total)
        return total

    def add_subdivision(self, mesh, levels, creases=None, corners=None, scheme='loop', polys=None):
        '''`levels` (1 to 5) levels of Loop subdivision for a mesh that has no object yet, before or after its targets and skin: an
        object of it then has 4^levels times the faces, smooth normals and the mesh's texcoords carried down face by face; face g of
        such an object descends from face g >> 2 * levels of the mesh.  Corners with equal positions are one control vertex; the
        mesh must be a manifold with consistent winding (open boundaries are fine), else the library says which face or vertex is
        not.

        `creases` [k,3]: a sharpness per face edge (edge j of face f runs from corner j to corner (j + 1) % 3) in subdivision levels,
        as OpenSubdiv's -- 0 smooth, inf always sharp, tools.crease.blender_crease maps Blender's 0..1; an edge takes the larger of
        what its two faces state; a negative value or a NaN is refused.  `corners` [k,3]: a flag per face corner; a control vertex
        with a flagged corner stays where it is.  An edge still sharp at the last level (and every boundary edge) splits the normals
        of the vertices on it.  Both are fixed with the level.

        scheme='catmull-clark' (Blender's Subdivision Surface modifier) subdivides a cage of polygons:
        `polys` [m] int32 holds the corner count n_j (3 to 64) of each, and polygon j is n_j - 2 consecutive triangles of the
        mesh, a fan about its first corner -- triangle i is (c_0, c_i+1, c_i+2); tools.polys.fan writes such a mesh; None makes every
        triangle a polygon.  `creases` and `corners` are then flat [sum n_j]: entry i of polygon j is the edge from its corner i to
        corner (i + 1) % n_j, respectively its corner i.  An object has 2 (sum n_j) 4^(levels - 1) faces: two per quad of the
        last level, face g descending from level-1 quad (g >> 1) >> 2 (levels - 1)'''
        if scheme not in SUBDIV_SCHEMES:
            raise ValueError('scheme %r: one of %s' % (scheme, ', '.join(SUBDIV_SCHEMES)))
        if scheme == 'loop' and polys is not None:
            raise ValueError("polys are the polygons of scheme 'catmull-clark': scheme 'loop' subdivides the triangles")
        if scheme == 'catmull-clark':
            return self._add_subdivision_cc(mesh, levels, creases, corners, polys)
        mesh, levels = self._fresh_mesh(mesh), int(levels)
        if not 1 <= levels <= SUBDIV_MAX_LEVELS:
            raise ValueError('%d levels: between 1 and %d' % (levels, SUBDIV_MAX_LEVELS))
        if mesh in self._mesh_levels:
            raise ValueError('mesh %d already has a subdivision level' % mesh)
        if self._mesh_faces[mesh] << (2 * levels) >= self.size:
            raise ValueError('too many faces: %d at level %d, room for fewer than %d' % (self._mesh_faces[mesh] << (2 * levels), levels, self.size))
        k = self._mesh_faces[mesh]
        if creases is None and corners is None:
            ctx().call('mpt_mesh_set_subdivision', mesh, levels)
        else:
            cr = None if creases is None else np.ascontiguousarray(creases, np.float32)
            co = None if corners is None else np.ascontiguousarray(np.asarray(corners) != 0, np.uint8)
            for name, a in (('creases', cr), ('corners', co)):
                if a is not None and a.shape != (k, 3):
                    raise ValueError('%s must be [%d,3], one per face %s, got %s' % (name, k, 'edge' if a is cr else 'corner', a.shape))
            ctx().call('mpt_mesh_set_subdivision_creased', mesh, levels, None if cr is None else fptr(cr),
                       None if co is None else co.ctypes.data_as(C.POINTER(C.c_uint8)))
        self._mesh_levels[mesh] = levels

    def _add_subdivision_cc(self, mesh, levels, creases, corners, polys):
        mesh, levels = self._fresh_mesh(mesh), int(levels)
        if not 1 <= levels <= SUBDIV_MAX_LEVELS:
            raise ValueError('%d levels: between 1 and %d' % (levels, SUBDIV_MAX_LEVELS))
        if mesh in self._mesh_levels:
            raise ValueError('mesh %d already has a subdivision level' % mesh)
        k = self._mesh_faces[mesh]
        po = np.full(k, 3, np.int32) if polys is None else np.ascontiguousarray(polys, np.int32)
        if po.ndim != 1:
            raise ValueError('polys must be [m], one corner count per polygon, got %s' % (po.shape,))
        ncorners = int(np.clip(po, 0, None).astype(np.int64).sum())         # (the library refuses polygons that are not the mesh's fans)
        faces = 2 * ncorners << (2 * (levels - 1))
        if faces >= self.size:
            raise ValueError('too many faces: %d at level %d, room for fewer than %d' % (faces, levels, self.size))
        cr = None if creases is None else np.ascontiguousarray(creases, np.float32)
        co = None if corners is None else np.ascontiguousarray(np.asarray(corners) != 0, np.uint8)
        for name, a in (('creases', cr), ('corners', co)):
            if a is not None and a.shape != (ncorners,):
                raise ValueError('%s must be [%d], one per polygon %s, got %s' % (name, ncorners, 'edge' if a is cr else 'corner', a.shape))
        ctx().call('mpt_mesh_set_subdivision_cc', mesh, levels, iptr(po), int(po.size), None if cr is None else fptr(cr),
                   None if co is None else co.ctypes.data_as(C.POINTER(C.c_uint8)))
        self._mesh_levels[mesh] = levels
        self._mesh_corners[mesh] = ncorners

    # ---- texture displacement of a subdivided mesh on the device (csrc/displace.hip, DESIGN.md section 3.20: Blender's Displace
    #      modifier with UV coordinates behind its subdivision surface; the reference's add-on is handed the evaluated mesh)
    def add_displacement(self, mesh, image, strength=1.0, midlevel=0.5, mode='normal', channel='mean'):
        '''a displacement for a subdivided mesh that has no object yet: the vertices of its last level move by image `image` of
        ImagePool (it need not be loaded yet; compose() needs it), sampled bilinearly at the uv of the vertex's first corner --
        mode 'normal': along the smooth normal by strength * (h - midlevel), h the channel 'r', 'g', 'b', 'a' or 'mean' (of r, g,
        b); mode 'vector': by strength * (rgb - midlevel) in object space.  The copy's normals are the displaced surface's'''
        mesh = self._fresh_mesh(mesh)
        if mesh not in self._mesh_levels:
            raise ValueError('displacement needs a subdivided mesh: mesh %d has no subdivision level' % mesh)
        if mesh in self._mesh_displace:
            raise ValueError('mesh %d already has a displacement' % mesh)
        if mode not in DISPLACE_MODES:
            raise ValueError('mode %r: one of %s' % (mode, ', '.join(DISPLACE_MODES)))
        if channel not in DISPLACE_CHANNELS:
            raise ValueError('channel %r: one of %s' % (channel, ', '.join(DISPLACE_CHANNELS)))
        image = int(getattr(image, 'id', image))                        # (an image.Image, or its id)
        if image < 0:
            raise ValueError('image id %d is negative' % image)
        strength, midlevel = self._displace_params(strength, midlevel)
        ctx().call('mpt_mesh_set_displacement', mesh, image, DISPLACE_MODES.index(mode), DISPLACE_CHANNELS.index(channel), strength, midlevel)
        self._mesh_displace[mesh] = [strength, midlevel]

    @staticmethod
    def _displace_params(strength, midlevel):
        strength, midlevel = float(strength), float(midlevel)
        if not (np.isfinite(strength) and np.isfinite(midlevel)):
            raise ValueError('strength %r and midlevel %r must be finite' % (strength, midlevel))
        return strength, midlevel

    def set_displacement(self, mesh, strength, midlevel=None):
        '''the strength (and the midlevel; None keeps it) of a displaced mesh, at any time; the next compose() displaces the copies
        of this mesh again and rewrites its objects only'''
        if int(mesh) not in self._mesh_displace:
            raise ValueError('mesh %r has no displacement' % (mesh,))
        mesh = int(mesh)
        strength, midlevel = self._displace_params(strength, self._mesh_displace[mesh][1] if midlevel is None else midlevel)
        ctx().call('mpt_mesh_set_displacement_params', mesh, strength, midlevel)
        self._mesh_displace[mesh] = [strength, midlevel]

    def displace_stats(self):
        '''_lib.DisplaceInfo: displaced meshes, their copies, copies and vertices the last compose() displaced, the image generation'''
        info = DisplaceInfo()
        ctx().call('mpt_displace_stats', C.byref(info))
        return info

    # ---- scatter: instances of a mesh placed over a surface object on the device, sticky when the surface moves
    #      (csrc/scatter.hip; Blender's "distribute points on faces" + "instance on points")
    def _scatter(self, scatter):
        if not 0 <= int(scatter) < len(self._scatters):
            raise ValueError('unknown scatter %r (%d scatters)' % (scatter, len(self._scatters)))
        return int(scatter)

    def add_scatter(self, surface, mesh, count, seed=0, mtlid=None, scale=(1, 1), align='normal', up=(0, 1, 0), random_yaw=True, density=None,
                    channel='mean', min_distance=0.0, candidates=None):
        '''`count` instances of mesh `mesh` (it may be subdivided and displaced, not deformable) scattered over the faces of object
        `surface` in proportion to their world area -- times, with density=an image of ImagePool, its `channel` at the faces' mean
        uv, clamped to [0, 1]; a face below 2^-24 of the largest weight gets none.  Each instance gets a scale drawn from
        scale=(min, max), a random yaw about its up axis (its local +Y) unless random_yaw=False, and stands along the face's
        geometric normal (align='normal') or along `up` (align='up').  The instances are objects with contiguous ids and material
        mtlid; they remember their face and their point on it, so that compose() after the surface was posed, displaced or moved
        again places them again on the device.  min_distance > 0 keeps the instances at least that far apart, through space, where
        they are born (Blender's "Poisson Disk"): `candidates` points (None: 4 * count) are drawn as above, in their order one is kept
        iff no kept one before it lies closer, and the first `count` kept are the instances; compose() refuses when fewer are kept.
        Returns (scatter id, range of object ids)'''
        surface = self._object(surface)
        if not 0 <= int(mesh) < len(self._mesh_faces):
            raise ValueError('unknown mesh %r (%d meshes)' % (mesh, len(self._mesh_faces)))
        mesh, count = int(mesh), int(count)
        if count < 1:
            raise ValueError('count %d is below 1' % count)
        if self.scatter_of(surface) is not None:
            raise ValueError('the surface, object %d, is itself an instance of scatter %d' % (surface, self.scatter_of(surface)[0]))
        total = self._faces_of_objects() + count * self._object_faces(mesh)
        if total >= self.size:
            raise ValueError('too many faces: %d with %d instances, room for fewer than %d' % (total, count, self.size))
        p = scatter_params(scale, align, up, random_yaw, density, channel)
        r, m = scatter_spacing(count, min_distance, candidates)
        sid, first = C.c_int(-1), C.c_int(-1)
        ctx().call('mpt_scatter_add', surface, mesh, count, int(seed) & (2 ** 64 - 1), -1 if mtlid is None else int(mtlid), C.byref(p), C.byref(sid),
                   C.byref(first))
        assert first.value == len(self._obj_mesh) and sid.value == len(self._scatters)
        if r > 0:
            ctx().call('mpt_scatter_set_spacing', sid.value, r, m)
        self._obj_mesh.extend([mesh] * count)
        self._scatters.append(dict(surface=surface, mesh=mesh, objects=range(first.value, first.value + count), seed=int(seed),
                                   params=dict(scale=scale, align=align, up=up, random_yaw=random_yaw, density=density, channel=channel),
                                   spacing=dict(min_distance=min_distance, candidates=candidates)))
        return sid.value, self._scatters[-1]['objects']

    def set_scatter(self, scatter, **params):
        '''new parameters (add_scatter's keywords scale ... channel, min_distance and candidates; the others keep their values) for a
        scatter; the next compose() selects and places its instances again'''
        s = self._scatters[self._scatter(scatter)]
        unknown = set(params) - set(s['params']) - set(s['spacing'])
        if unknown:
            raise ValueError('unknown scatter parameters: %s' % ', '.join(sorted(unknown)))
        merged = dict(s['params'], **{k: v for k, v in params.items() if k in s['params']})
        spacing = dict(s['spacing'], **{k: v for k, v in params.items() if k in s['spacing']})
        p = scatter_params(**merged)
        r, m = scatter_spacing(len(s['objects']), **spacing)
        if not all(k in s['spacing'] for k in params) or not params:
            ctx().call('mpt_scatter_set_params', int(scatter), C.byref(p))
        if any(k in s['spacing'] for k in params):
            ctx().call('mpt_scatter_set_spacing', int(scatter), r, m)
        s['params'], s['spacing'] = merged, spacing

    def rescatter(self, scatter, seed=None):
        '''scatter again with a new seed (None: the old seed + 1); the next compose() selects and places the instances again.  The
        old seed on the same surface gives the old instances back bit for bit'''
        s = self._scatters[self._scatter(scatter)]
        seed = s['seed'] + 1 if seed is None else int(seed)
        ctx().call('mpt_scatter_rescatter', int(scatter), seed & (2 ** 64 - 1))
        s['seed'] = seed

    def scatter_of(self, obj):
        '''(scatter id, instance index) of an object id -- as BVHTree().pick() and intersect() report it -- or None for an object
        that is no instance'''
        for sid, s in enumerate(self._scatters):
            if int(obj) in s['objects']:
                return sid, int(obj) - s['objects'].start
        return None

    def scatter_to_numpy(self, scatter):
        '''(records [count] of _lib.SCATTER_POINT_DTYPE, world matrices [count,4,4] f64, shares q [F] uint32) of a scatter as the last
        compose() left them on the device'''
        s = self._scatters[self._scatter(scatter)]
        n, F = len(s['objects']), self._object_faces(self._obj_mesh[s['surface']])
        points, worlds, q = np.zeros(n, SCATTER_POINT_DTYPE), np.zeros((n, 4, 4), np.float64), np.zeros(F, np.uint32)
        ctx().call('mpt_scatter_get', int(scatter), points.ctypes.data_as(C.c_void_p), worlds.ctypes.data_as(C.POINTER(C.c_double)),
                   q.ctypes.data_as(C.POINTER(C.c_uint32)))
        return points, worlds, q

    def scatter_stats(self):
        '''_lib.ScatterInfo: scatters and instances; scatters that selected, scatters and instances placed, the weight / scan /
        selection / placement launches and the host's reads of the last compose()'''
        info = ScatterInfo()
        ctx().call('mpt_scatter_stats', C.byref(info))
        return info

    def scatter_spacing(self, scatter):
        '''(candidates, kept, rounds, kept_flags [candidates] bool, index [count] int64) of a spaced scatter's last elimination:
        the candidates drawn, how many of them were kept, the rounds the device took, which were kept, and the candidate that became
        each instance'''
        s = self._scatters[self._scatter(scatter)]
        m, kept, rounds = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        ctx().call('mpt_scatter_get_spacing', int(scatter), C.byref(m), C.byref(kept), C.byref(rounds), None, None)
        flags, index = np.zeros(m.value, np.uint8), np.zeros(len(s['objects']), np.int64)
        ctx().call('mpt_scatter_get_spacing', int(scatter), None, None, None, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                   index.ctypes.data_as(C.POINTER(C.c_int64)))
        return m.value, kept.value, rounds.value, flags.astype(bool), index

    def scatter_spacing_stats(self):
        '''_lib.ScatterSpacingInfo of the last compose(): the spaced scatters that selected, their candidates and kept candidates,
        the most rounds one took, the grid / round / compaction kernels launched and the host's waits; all zero without one'''
        info = ScatterSpacingInfo()
        ctx().call('mpt_scatter_spacing_stats', C.byref(info))
        return info

    def subdivided_to_numpy(self, obj):
        '''the subdivided copy of an object of a subdivided mesh as the last compose() wrote it -- displaced, if the mesh carries a
        displacement: [3 k 4^levels, 8] f32 records in object space (a Catmull-Clark copy: [3 * 2 (sum n_j) 4^(levels - 1), 8])'''
        return self._copy_to_numpy('mpt_get_subdivided', obj, self._object_faces)

    def subdiv_stats(self):
        '''_lib.SubdivInfo: objects of subdivided meshes, copies, copies and faces the last compose() refined, pool vertices the
        copies hold'''
        info = SubdivInfo()
        ctx().call('mpt_subdiv_stats', C.byref(info))
        return info

    def compose_stats(self):
        '''_lib.ComposeInfo: faces, faces the last compose() wrote, objects it found changed, fetches of the host copy, bounding sphere'''
        info = ComposeInfo()
        ctx().call('mpt_compose_stats', C.byref(info))
        return info

    def load_meshes(self, primitives):
        '''the reference's list of (p, n, t, w, m) tuples (multimesh.compose_multiple_meshes's argument) composed on the device:
        drops what the pool and the table held, adds a mesh per distinct (p, n, t) -- tuples that share the same array objects
        share one mesh -- and an object per tuple, and composes.  Returns the object ids, in order'''
        primitives = list(primitives)
        if not primitives:
            raise ValueError('no primitives')
        self.clear_meshes()
        meshes, objs = {}, []
        for p, n, t, w, m in primitives:
            key = (id(p), id(n), id(t))
            if key not in meshes:
                meshes[key] = self.add_mesh(p, n, t)
            objs.append(self.add_object(meshes[key], w, m))
        self.compose()
        return objs

    def load(self, arr, mtlids=None):
        '''reference model.py:62-86: [3n,8] array (pos3 nrm3 uv2), or an OBJ-style dict, or a path'''
        if isinstance(arr, str):
            from .tools.readobj import readobj
            arr = readobj(arr)

        if isinstance(arr, dict):
            f = arr['f']
            verts = arr['v'][f[:, :, 0]].reshape(f.shape[0] * 3, 3)
            norms = arr['vn'][f[:, :, 2]].reshape(f.shape[0] * 3, 3)
            coors = arr['vt'][f[:, :, 1]].reshape(f.shape[0] * 3, 2)
            arr = np.concatenate([verts, norms, coors], axis=1)

        arr = np.asarray(arr)
        if arr.dtype == np.float64:
            arr = arr.astype(np.float32)

        assert arr.shape[0] % 3 == 0
        if mtlids is None:
            mtlids = -np.ones(arr.shape[0] // 3, dtype=np.int32)
        else:
            mtlids = np.asarray(mtlids)
            assert mtlids.shape[0] == arr.shape[0] // 3
        assert mtlids.shape[0] < self.size, 'too many faces'

        self.from_numpy(arr, mtlids)

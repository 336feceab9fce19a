'''
linear BVH (reference tree/lbvh.py).  build() = Morton codes -> keyed sort -> Karras
hierarchy -> boxes, packed into the traversal records (csrc/miptina.cpp mpt_build_tree);
intersect() (lbvh.py:314-347) is csrc/pt_device.h bvh_closest / bvh_occluded inside the engines' kernels, and -- asked from
Python for a batch of rays -- intersect() / occluded() / pick() below (csrc/query_kernel.hip).
'''

from ..common import *                # noqa: F401,F403
from ..common import Singleton, register, ctx, np
from .._lib import fptr, iptr, RefitInfo
import ctypes as C


# update()'s default: a refitted tree is built again once its cost has grown by more than this factor.  Measured on the turntable
# of tools/refit_bench.py (99 382 triangles in 64 objects, one of them turned through a full turn in 36 steps and refitted at every
# step, 512 x 512 x 8 spp): refit + render first costs more than build + render at a growth of 1.47, rounded down to one decimal
# (profiles/r23_refit_bench.json).
DEFAULT_MAX_GROWTH = 1.4

# the walk types of the production PathEngine kernels, by their MPT_WALK_* numbers (include/miptina.h; walk_trace())
WALKS = ('gather', 'lds', 'wide_exact', 'wide_quant', 'lds4')


class LinearBVH:
    def __init__(self, n=2**22):
        self.capacity = n

    def build(self):
        ctx().call('mpt_build_tree')

    def refit(self):
        '''keep the built trees and fit their boxes, and the triangle records, to the model as it is now -- after
        ModelPool().set_world + compose(), or load() of as many faces -- on the device (csrc/refit.hip; no
        reference counterpart: its add-on builds again, blender.py:555-571).  Returns the growth: the binary tree's cost now over
        its cost as built (refit_stats()), 1.0 for a tree without nodes.  Raises where a refit is not allowed; the message names
        build_tree()'''
        ctx().call('mpt_refit_tree')
        return float(self.refit_stats().growth)

    def refit_stats(self):
        '''_lib.RefitInfo: faces the trees were built for (-1: none), wide nodes, refits since the build, fetches of the model's host
        copy the refits caused (0), cost_built, cost_now and growth'''
        info = RefitInfo()
        ctx().call('mpt_refit_stats', C.byref(info))
        return info

    def can_refit(self):
        '''would refit() be allowed for the model as it stands? (the rule refit() itself applies, csrc/refit_rule.h)'''
        return bool(self.refit_stats().allowed)

    def update(self, max_growth=DEFAULT_MAX_GROWTH):
        '''refit() where a refit is allowed, build() otherwise -- and build() after a refit that left the tree's cost more than
        max_growth times what it was when built (inf: never).  Returns 'refit' or 'build', whichever ran last'''
        if self.can_refit():
            if self.refit() <= max_growth:
                return 'refit'
        self.build()
        return 'build'

    def to_numpy(self):
        '''the reference-layout arrays (lbvh.py:48-56) of the built tree'''
        from ..model import ModelPool
        n = ModelPool().nfaces
        ni = max(n - 1, 1)
        child = np.zeros((ni, 2), np.int32)
        leaf = np.zeros(max(n, 1), np.int32)
        bmin = np.zeros((ni, 3), np.float32)
        bmax = np.zeros((ni, 3), np.float32)
        mc = np.zeros(max(n, 1), np.int32)
        depth = C.c_int32(0)
        ctx().call('mpt_get_tree', iptr(child), iptr(leaf), fptr(bmin), fptr(bmax), iptr(mc),
                   C.byref(depth))
        k = max(n - 1, 0)
        return dict(child=child[:k], leaf=leaf[:n], bmin=bmin[:k], bmax=bmax[:k], mc=mc[:n],
                    depth=depth.value)

    def records(self):
        '''the node and triangle records the kernels fetch, as they lie on the device (mpt_get_records): a dict of uint32 arrays
        snode [n-1][2][4], fnode [n-1][4][4], tgeo [n][4][4], tshade [n][4][4] and tfast [n+1][3][4]'''
        n = C.c_int(0)
        ctx().call('mpt_get_records', None, None, None, None, None, 0, C.byref(n))
        n = n.value
        k = max(n - 1, 0)
        out = dict(snode=np.zeros((k, 2, 4), np.float32), fnode=np.zeros((k, 4, 4), np.float32), tgeo=np.zeros((n, 4, 4), np.float32),
                   tshade=np.zeros((n, 4, 4), np.float32), tfast=np.zeros((n + 1, 3, 4), np.float32))
        ctx().call('mpt_get_records', *(fptr(out[key]) for key in ('snode', 'fnode', 'tgeo', 'tshade', 'tfast')), n, C.byref(C.c_int(0)))
        return {key: a.view(np.uint32) for key, a in out.items()}

    # ------------------------------------------------------------ batch ray queries (reference lbvh.py:314-347, one ray per call there)
    def intersect(self, o, d, avoid=None, chunk=0):
        '''the closest hit of each of n rays against the built tree, by the context's build.  o and d broadcast to [n][3] (one
        origin with many directions works); d may have any length -- it is normalised for the caller, so depth is a world
        distance; avoid is a face (scalar or [n]; -1 or None: none) the ray ignores.  A ray with a non-finite component or a zero
        direction is a miss.  Returns a dict of numpy arrays [n]: hit (bool), depth (f32; 1e6, the reference's inf, on a miss),
        index (the face, -1 on a miss), u, v (the hit's barycentrics along v1 - v0 and v2 - v0) and object (the object of
        ModelPool().load_meshes whose faces hold index; -1 on a miss or for a model that came from load()).  Raises where the
        tree is not built for the model as it stands.  chunk: rays per launch (0: the library's default)'''
        o, d, n = _rays(o, d)
        av = _per_ray(avoid, n, np.int32, 'avoid')
        out = {k: np.zeros(n, t) for k, t in (('hit', np.int32), ('depth', np.float32), ('index', np.int32), ('u', np.float32),
                                              ('v', np.float32), ('object', np.int32))}
        ctx().call('mpt_query_closest', n, fptr(o), fptr(d), None if av is None else iptr(av), iptr(out['hit']), fptr(out['depth']),
                   iptr(out['index']), fptr(out['u']), fptr(out['v']), iptr(out['object']), int(chunk))
        out['hit'] = out['hit'] != 0
        return out

    def occluded(self, o, d, dis=np.inf, avoid=None, chunk=0):
        '''the reference's shadow test for each of n rays (path.py:50-51): is there a hit no farther than dis?  o, d and avoid as
        intersect takes them; dis a scalar or [n] (inf: any hit counts).  Returns bool [n]'''
        o, d, n = _rays(o, d)
        av = _per_ray(avoid, n, np.int32, 'avoid')
        di = None if np.ndim(dis) == 0 and dis == np.inf else _per_ray(dis, n, np.float32, 'dis')
        occ = np.zeros(n, np.int32)
        ctx().call('mpt_query_occluded', n, fptr(o), fptr(d), None if di is None else fptr(di), None if av is None else iptr(av),
                   iptr(occ), int(chunk))
        return occ != 0

    def walk_trace(self, walk, o, d, avoid=None, dis=None, chunk=0):
        '''test door (mpt_walk_trace, csrc/walk_eval.hip): n rays through the traversal of the production
        PathEngine kernels -- walk names one of WALKS ('gather', 'lds', 'wide_exact', 'wide_quant', 'lds4') or its number.  o, d
        and avoid as intersect takes them.  dis None: the closest hit as the shading stage would be handed it -> the dict of
        intersect() without object, depth / u / v the walk's own f32 values.  dis (a scalar or [n]): the rays are shadow rays ->
        bool [n], occluded.  Raises -- there is no fall-back -- in strict mode, for a stale tree and for a walk that cannot serve
        the scene'''
        o, d, n = _rays(o, d)
        av = _per_ray(avoid, n, np.int32, 'avoid')
        di = _per_ray(dis, n, np.float32, 'dis')
        kind = WALKS.index(walk) if isinstance(walk, str) else int(walk)
        out = {k: np.zeros(n, t) for k, t in (('hit', np.int32), ('depth', np.float32), ('index', np.int32), ('u', np.float32), ('v', np.float32))}
        ctx().call('mpt_walk_trace', kind, n, fptr(o), fptr(d), None if av is None else iptr(av), None if di is None else fptr(di),
                   iptr(out['hit']), fptr(out['depth']), iptr(out['index']), fptr(out['u']), fptr(out['v']), int(chunk))
        out['hit'] = out['hit'] != 0
        return out['hit'] if di is not None else out

    def pick(self, x, y):
        '''what the camera sees at clip point (x, y), each in [-1, 1]: (object, face, depth) of the closest hit of the camera ray
        through it, or None.  The ray is generated on the host from the f32 matrix Camera() uploaded, as the kernels'
        camera_generate does (reference camera.py:34-39); a convenience over intersect()'''
        from ..camera import Camera
        M = Camera().V2W
        one = np.float32(1)
        a = M @ np.array([x, y, -one, one], np.float32)
        b = M @ np.array([x, y, one, one], np.float32)
        o = (a[:3] / a[3]).astype(np.float32)
        r = self.intersect(o, (b[:3] / b[3]).astype(np.float32) - o)
        if not r['hit'][0]:
            return None
        return int(r['object'][0]), int(r['index'][0]), float(r['depth'][0])


def _rays(o, d):
    '''origins and directions broadcast against each other to contiguous f32 [n][3] -> (o, d, n)'''
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    if o.ndim == 0 or d.ndim == 0 or o.shape[-1] != 3 or d.shape[-1] != 3:
        raise ValueError('origins %s and directions %s: the last axis must hold 3 numbers' % (o.shape, d.shape))
    o, d = np.broadcast_arrays(o.reshape(-1, 3), d.reshape(-1, 3))
    return np.ascontiguousarray(o), np.ascontiguousarray(d), int(o.shape[0])


def _per_ray(value, n, dtype, what):
    '''None, a scalar or [n] -> None or a contiguous [n] array'''
    if value is None:
        return None
    a = np.asarray(value, dtype)
    if a.ndim == 0:
        return np.full(n, a, dtype)
    if a.shape != (n,):
        raise ValueError('%s has shape %s for %d rays' % (what, a.shape, n))
    return np.ascontiguousarray(a)


@register
class BVHTree(LinearBVH, metaclass=Singleton):
    pass

'''
linear BVH (reference tree/lbvh.py).  build() = Morton codes -> keyed sort -> Karras
hierarchy -> boxes, packed into the traversal records (csrc/miptina.cpp mpt_build_tree);
intersect() (lbvh.py:314-347) is csrc/pt_device.h bvh_closest / bvh_occluded.
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


@register
class BVHTree(LinearBVH, metaclass=Singleton):
    pass

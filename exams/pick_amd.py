#!/usr/bin/env python3
'''
Pick and move: the scene of exams/animate_amd.py (the Cornell walls and two boxes as meshes and objects on the device), the object
under a pixel found by BVHTree().pick, moved with ModelPool().set_world -> compose() -> BVHTree().update(), and picked again.
pick() is the closest hit of the camera ray through a clip point, asked of the built tree by a batch ray query
(BVHTree().intersect, csrc/query_kernel.hip); the reference can ask its tree only from inside a kernel (lbvh.py:314-347).

    python exams/pick_amd.py [--size 256] [--pixel 102 115] [--shift 0.5 0.0 0.3]
'''
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptina_amd.things import *              # noqa: E402,F401,F403
from ptina_amd.engine.path import *         # noqa: E402,F401,F403
from ptina_amd import scenes                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--pixel', type=int, nargs=2, default=[102, 115], help='film pixel (i, j), i to the right and j up')
ap.add_argument('--shift', type=float, nargs=3, default=[0.5, 0.0, 0.3], help='how far the picked object is moved')
args = ap.parse_args()

ti.init(ti.cuda)
init_things()
PathEngine()
FilmTable().set_size(args.size, args.size)
_, _, materials, images = scenes.scene_s34()
MaterialPool().load(materials)
ImagePool().load(images)
Camera().set_perspective(scenes.BENCH_CAMERA)


def placed(center, yaw_deg):
    th = np.radians(yaw_deg)
    return np.array([[np.cos(th), 0, np.sin(th), center[0]], [0, 1, 0, center[1]], [-np.sin(th), 0, np.cos(th), center[2]], [0, 0, 0, 1.0]])


# the reference's list of (p, n, t, world, material) tuples: the walls by material where they are, the boxes placed by their matrices
wp, wn, wt, wm = scenes.cornell_walls()
names = ['walls of material 0', 'walls of material 1', 'walls of material 2']
worlds = [np.eye(4) for _ in names]
primitives = [(wp[wm == mtl], wn[wm == mtl], wt[wm == mtl], worlds[mtl], mtl) for mtl in (0, 1, 2)]
for name, half, center, yaw, mtl in (('tall box', (0.6, 1.2, 0.6), (-0.7, 1.2, -0.6), 18.0, 3), ('short box', (0.6, 0.6, 0.6), (0.75, 0.6, 0.55), -17.0, 4)):
    p, n, t = scenes.box((0, 0, 0), half, 0.0, mtl)[:3]
    names.append(name)
    worlds.append(placed(center, yaw))
    primitives.append((p, n, t, worlds[-1], mtl))
objs = ModelPool().load_meshes(primitives)
BVHTree().build()

x, y = (args.pixel[0] + 0.5) / args.size * 2 - 1, (args.pixel[1] + 0.5) / args.size * 2 - 1
first = BVHTree().pick(x, y)
if first is None:
    print('pixel (%d, %d): nothing there' % tuple(args.pixel))
    sys.exit(0)
obj, face, depth = first
print('pixel (%d, %d): object %d (%s), face %d, %.4f away' % (*args.pixel, obj, names[obj], face, depth))

moved = worlds[obj].copy()
moved[:3, 3] += args.shift
ModelPool().set_world(objs[obj], moved)
ModelPool().compose()
how = BVHTree().update()
again = BVHTree().pick(x, y)
print('moved by %s (%s): the pixel now shows %s' % (args.shift, how, 'nothing' if again is None else
                                                    'object %d (%s), face %d, %.4f away' % (again[0], names[again[0]], again[1], again[2])))

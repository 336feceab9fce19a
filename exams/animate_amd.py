#!/usr/bin/env python3
'''
A turntable: the Cornell scene's tall box turned about its own axis over N frames, the scene kept on the device.  The walls and
the two boxes are meshes of ModelPool's pool and objects of its table; each frame is
    ModelPool().set_world(box, matrix) -> compose() -> BVHTree().build() -> PathEngine().render() x spp -> FilmTable().get_display()
so nothing but the matrix crosses to the device and nothing but the 8-bit picture comes back.  With --refit a frame is
    set_world -> compose() -> BVHTree().update() -> render ...
and update() keeps the built tree and fits its boxes to the turned box (csrc/refit.hip), building again only when the tree's
cost has grown past --max-growth.  The reference's add-on runs
compose_multiple_meshes + load_model + build_tree over the whole scene at every change (blender.py:555-571).

    python exams/animate_amd.py [--frames 12] [--size 256] [--spp 8] [--out DIR] [--refit [--max-growth G]]
'''
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptina_amd.things import *              # noqa: E402,F401,F403
from ptina_amd.engine.path import *         # noqa: E402,F401,F403
from ptina_amd.image import write_png       # noqa: E402
from ptina_amd import scenes                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=12)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--spp', type=int, default=8)
ap.add_argument('--out', default='.')
ap.add_argument('--refit', action='store_true', help='BVHTree().update() instead of build() at every frame')
ap.add_argument('--max-growth', type=float, default=None, help="update()'s bound (default: the library's)")
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


# the s34 scene as objects: the walls where they are, the boxes as axis-aligned meshes about the origin placed by their matrices
wp, wn, wt, wm = scenes.cornell_walls()
pool = ModelPool()
for mtl in (0, 1, 2):
    pick = wm == mtl
    pool.add_object(pool.add_mesh(wp[pick], wn[pick], wt[pick]), np.eye(4), mtl)
tall = pool.add_object(pool.add_mesh(*scenes.box((0, 0, 0), (0.6, 1.2, 0.6), 0.0, 3)[:3]), placed((-0.7, 1.2, -0.6), 18.0), 3)
pool.add_object(pool.add_mesh(*scenes.box((0, 0, 0), (0.6, 0.6, 0.6), 0.0, 4)[:3]), placed((0.75, 0.6, 0.55), -17.0), 4)
pool.compose()

os.makedirs(args.out, exist_ok=True)
t0 = time.perf_counter()
refitted, largest = 0, 1.0
for f in range(args.frames):
    pool.set_world(tall, placed((-0.7, 1.2, -0.6), 18.0 + 360.0 * f / args.frames))
    pool.compose()
    if args.refit:
        how = BVHTree().update() if args.max_growth is None else BVHTree().update(args.max_growth)
        refitted += how == 'refit'
        largest = max(largest, BVHTree().refit_stats().growth if how == 'refit' else 1.0)
    else:
        BVHTree().build()
    FilmTable().clear()
    PathEngine().render(args.spp)
    img = FilmTable().get_display(layout='display')
    write_png(os.path.join(args.out, 'turntable_%03d.png' % f), img)
    info = pool.compose_stats()
    print('frame %d: %d of %d faces recomposed, mean byte %.2f' % (f, info.recomposed, info.faces, float(img[..., :3].mean())))
dt = time.perf_counter() - t0
print('%d frames of %dx%d at %d spp in %.2f s (PNG writing included), host copy of the model fetched %d times: written to %s'
      % (args.frames, args.size, args.size, args.spp, dt, pool.compose_stats().host_fetches, args.out))
if args.refit:
    print('%d of %d frames refitted, the others built; largest growth of a refitted tree %.3f' % (refitted, args.frames, largest))

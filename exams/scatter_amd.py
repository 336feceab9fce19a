#!/usr/bin/env python3
'''
Tufts on the rippling pond of exams/displace_amd.py: the flat cage of 8 x 8 quads with a Loop subdivision level and a displacement
by a procedural ripple image lies on the floor of the Cornell room, and --count tufts (three crossed blades, 6 triangles) are
scattered over it on the device, more of them where the ripple image is bright.  Each frame is
    ModelPool().set_displacement(pond, strength) -> compose() -> BVHTree().update() -> PathEngine().render() x spp
so nothing but two numbers crosses to the device: the pond is displaced again there (csrc/displace.hip), every tuft is placed again
on the face and at the barycentric point it was born on, along the face's normal as it is now (csrc/scatter.hip: the placement
kernel alone; weights, scan and selection ran once, in the first compose), the pond's and the tufts' faces are composed again and
the built tree is fitted to them (csrc/refit.hip) -- instance count, topology and face count never change.
--min-distance R keeps the tufts at least R apart where they are born (csrc/scatter_space.hip: four times --count candidates, the
greedy elimination in the first compose; 0.02 suits the default count): no two of them stand in each other.

    python exams/scatter_amd.py [--frames 12] [--levels 4] [--count 2000] [--min-distance 0] [--size 256] [--spp 8] [--image 256] [--out DIR]
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
ap.add_argument('--levels', type=int, default=4)
ap.add_argument('--count', type=int, default=2000)
ap.add_argument('--min-distance', type=float, default=0.0)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--spp', type=int, default=8)
ap.add_argument('--image', type=int, default=256)
ap.add_argument('--out', default='.')
args = ap.parse_args()

QUADS, SIDE = 8, 1.6


def cage():
    '''(p, n [k,3,3], t [k,3,2]): a flat grid of quads in the plane y = 0, each split in two, texcoords over the unit square'''
    x = np.linspace(-SIDE / 2, SIDE / 2, QUADS + 1)
    p, t = [], []
    for j in range(QUADS):
        for i in range(QUADS):
            quad = [(i, j), (i, j + 1), (i + 1, j + 1), (i + 1, j)]           # (wound so that the normal is +y)
            for tri in ((quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])):
                p.append([(x[a], 0.0, x[b]) for a, b in tri])
                t.append([(a / QUADS, b / QUADS) for a, b in tri])
    p = np.array(p, np.float32)
    n = np.tile(np.float32([0, 1, 0]), (p.shape[0], 3, 1))
    return p, n, np.array(t, np.float32)


def tuft():
    '''(p, n [6,3,3], None): three blades through the local +Y axis, one unit high, each a quad narrowing to the top'''
    p, n = [], []
    for k in range(3):
        a = np.pi * k / 3
        d, side = np.array([np.cos(a), 0.0, np.sin(a)]), np.array([-np.sin(a), 0.0, np.cos(a)])
        lo0, lo1, hi0, hi1 = -0.3 * d, 0.3 * d, -0.08 * d + [0, 1, 0], 0.08 * d + [0, 1, 0]
        p += [[lo0, lo1, hi1], [lo0, hi1, hi0]]
        n += [[side] * 3, [side] * 3]
    return np.array(p, np.float32), np.array(n, np.float32), None


def ripples(size):
    '''[size,size,4] f32: the height of two ring waves in every channel, in [0, 1]'''
    u = (np.arange(size) + 0.5) / size
    x, y = np.meshgrid(u, u, indexing='ij')
    h = 0.5 + 0.25 * np.cos(40 * np.hypot(x - 0.35, y - 0.4)) + 0.25 * np.cos(55 * np.hypot(x - 0.7, y - 0.65))
    return np.float32(np.repeat(h[:, :, None], 4, axis=2))


def shift(x, y, z):
    m = np.eye(4)
    m[:3, 3] = [x, y, z]
    return m


ti.init(ti.cuda)
init_things()
PathEngine()
FilmTable().set_size(args.size, args.size)
_, _, materials, images = scenes.scene_s34()
MaterialPool().load(materials)
ImagePool().load(images)
ripple = ImagePool().load_one(ripples(args.image))
Camera().set_perspective(scenes.BENCH_CAMERA)

wp, wn, wt_, wm = scenes.cornell_walls()
pool = ModelPool()
for mtl in (0, 1, 2):
    pick = wm == mtl
    pool.add_object(pool.add_mesh(wp[pick], wn[pick], wt_[pick]), np.eye(4), mtl)
mesh = pool.add_mesh(*cage())
pool.add_subdivision(mesh, args.levels)
pool.add_displacement(mesh, ripple, strength=0.0, midlevel=0.5, mode='normal', channel='r')
pond = pool.add_object(mesh, shift(0.0, 0.25, -0.2), 3)
scatter, tufts = pool.add_scatter(pond, pool.add_mesh(*tuft()), args.count, seed=1, mtlid=1, scale=(0.03, 0.07), density=ripple, channel='r',
                                   min_distance=args.min_distance)
pool.compose()
if args.min_distance > 0:
    m, kept, rounds, _, _ = pool.scatter_spacing(scatter)
    print('%d of %d candidates stand at least %g apart (%d rounds on the device): the first %d are the tufts' % (kept, m, args.min_distance, rounds, args.count))
s = pool.scatter_stats()
print('%d tufts (objects %d .. %d) scattered over %d faces: %d weight, %d scan, %d selection and %d placement launches'
      % (s.instances, tufts.start, tufts.stop - 1, pool._object_faces(mesh), s.weight_launches, s.scan_launches, s.select_launches, s.place_launches))
BVHTree().build()

os.makedirs(args.out, exist_ok=True)
t0 = time.perf_counter()
refitted = 0
for f in range(args.frames):
    phase = 2 * np.pi * f / args.frames
    pool.set_displacement(mesh, 0.12 * np.sin(phase))
    pool.compose()
    refitted += BVHTree().update() == 'refit'
    FilmTable().clear()
    PathEngine().render(args.spp)
    img = FilmTable().get_display(layout='display')
    write_png(os.path.join(args.out, 'scatter_%03d.png' % f), img)
    s, c = pool.scatter_stats(), pool.compose_stats()
    print('frame %d: strength %+.3f, %d tufts placed again in %d launch (selection launches: %d), %d of %d faces recomposed, mean byte %.2f'
          % (f, 0.12 * np.sin(phase), s.placed_instances, s.place_launches, s.select_launches, c.recomposed, c.faces, float(img[..., :3].mean())))
dt = time.perf_counter() - t0
print('%d frames of %dx%d at %d spp in %.2f s (PNG writing included), %d refitted: written to %s'
      % (args.frames, args.size, args.size, args.spp, dt, refitted, args.out))

#!/usr/bin/env python3
'''
A coarse tube that bends and comes out smooth: a skinned control cage of 8 sides x 8 rings (128 triangles, 8 joints) with a Loop
subdivision level standing in the Cornell room, the scene kept on the device.  Each frame is
    ModelPool().set_joints(tube, palette) -> compose() -> BVHTree().update() -> PathEngine().render() x spp
so nothing but the pose (8 matrices) crosses to the device: the cage's corners are skinned there (csrc/deform.hip), the posed cage
is subdivided there (csrc/subdiv.hip: 128 x 4^levels faces with smooth normals), the tube's faces are composed again and the built
tree is fitted to them (csrc/refit.hip) -- topology and face count never change.  With --levels 0 the cage itself is rendered.
With --creases two cubes of 12 triangles stand beside the tube: one with Blender's edge crease 1 on its 12 edges
(tools.crease.blender_crease: sharpness inf), which stays a cube with a flat normal per face, and one without, which comes out a
blob.
With --scheme catmull-clark the tube's 64 quads and the cubes' six are the cages (each quad is stored as the fan of two triangles it
already is), subdivided as Blender's Subdivision Surface modifier does: no diagonal shows.

    python exams/subdivide_amd.py [--frames 12] [--levels 3] [--size 256] [--spp 8] [--out DIR] [--creases] [--scheme catmull-clark]
'''
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptina_amd.things import *              # noqa: E402,F401,F403
from ptina_amd.engine.path import *         # noqa: E402,F401,F403
from ptina_amd.image import write_png       # noqa: E402
from ptina_amd.tools.skin import joint_matrices   # noqa: E402
from ptina_amd.tools.crease import blender_crease   # noqa: E402
from ptina_amd import scenes                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=12)
ap.add_argument('--levels', type=int, default=3)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--spp', type=int, default=8)
ap.add_argument('--out', default='.')
ap.add_argument('--creases', action='store_true', help='a creased cube beside a smooth one')
ap.add_argument('--scheme', default='loop', choices=('loop', 'catmull-clark'))
args = ap.parse_args()
CC = args.scheme == 'catmull-clark'

JOINTS, HEIGHT, RADIUS, RINGS, SIDES = 8, 2.4, 0.25, 8, 8


def cage():
    '''(p, n [k,3,3], joints, weights [k,3,4]): rings of quads round the y axis, the last side joined to the first by index (so the
    corners weld: the tube is closed round and open at its ends), each vertex bound to the two joints its height lies between'''
    ang = 2 * np.pi * np.arange(SIDES) / SIDES
    y = np.linspace(0.0, HEIGHT, RINGS + 1)
    nrm = np.stack([np.cos(ang), np.zeros(SIDES), np.sin(ang)], axis=-1)
    pos = np.float32(RADIUS * nrm[None] + np.stack([np.zeros(RINGS + 1), y, np.zeros(RINGS + 1)], axis=-1)[:, None])   # [ring, side, 3]
    at = np.clip(y / HEIGHT * JOINTS - 0.5, 0.0, JOINTS - 1.0)
    j0 = np.floor(at).astype(np.int64)
    j1 = np.minimum(j0 + 1, JOINTS - 1)
    f = at - j0
    p, n, jt, wt = [], [], [], []
    for r in range(RINGS):
        for s in range(SIDES):
            quad = [(r, s), (r + 1, s), (r + 1, (s + 1) % SIDES), (r, (s + 1) % SIDES)]
            for tri in ((quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])):
                p.append([pos[a, b] for a, b in tri])
                n.append([nrm[b] for a, b in tri])
                jt.append([[j0[a], j1[a], 0, 0] for a, b in tri])
                wt.append([[1.0 - f[a], f[a], 0, 0] for a, b in tri])
    return np.array(p, np.float32), np.array(n, np.float32), np.array(jt), np.array(wt, np.float32)


def cube(half):
    '''(p, n [12,3,3], crease [12,3]): a cube of 12 triangles and Blender's crease 1 on its 12 edges -- a face edge whose ends
    differ in one coordinate; the diagonals of its faces stay smooth'''
    v = np.float32([(x, y, z) for z in (-half, half) for y in (-half, half) for x in (-half, half)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    faces = np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))])
    p = v[faces]
    along = (p != np.roll(p, -1, axis=1)).sum(axis=2) == 1
    n = np.repeat(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, None], 3, axis=1)
    return p, np.float32(n / np.linalg.norm(n, axis=2, keepdims=True)), np.where(along, blender_crease(1.0), np.float32(0))


def shift(x, y, z):
    m = np.eye(4)
    m[:3, 3] = [x, y, z]
    return m


def palette(bend):
    '''the 8 joints as a chain up the tube, each turned by bend / 8 radians about z against its parent'''
    seg = HEIGHT / JOINTS
    c, s = np.cos(bend / JOINTS), np.sin(bend / JOINTS)
    turn = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    local = np.stack([shift(0, 0 if j == 0 else seg, 0) @ turn for j in range(JOINTS)])
    inverse_bind = np.stack([shift(0, -j * seg, 0) for j in range(JOINTS)])
    return joint_matrices(np.arange(JOINTS) - 1, local, inverse_bind)


ti.init(ti.cuda)
init_things()
PathEngine()
FilmTable().set_size(args.size, args.size)
_, _, materials, images = scenes.scene_s34()
MaterialPool().load(materials)
ImagePool().load(images)
Camera().set_perspective(scenes.BENCH_CAMERA)

wp, wn, wt_, wm = scenes.cornell_walls()
pool = ModelPool()
for mtl in (0, 1, 2):
    pick = wm == mtl
    pool.add_object(pool.add_mesh(wp[pick], wn[pick], wt_[pick]), np.eye(4), mtl)
p, n, joints, weights = cage()
mesh = pool.add_mesh(p, n)
pool.add_skin(mesh, joints, weights, JOINTS)
if args.levels:
    pool.add_subdivision(mesh, args.levels, scheme=args.scheme, polys=np.full(RINGS * SIDES, 4, np.int32) if CC else None)
obj = pool.add_object(mesh, shift(0.0, 0.0, -0.3), 3)
if args.creases and args.levels:
    cp, cn, crease = cube(0.3)
    for x, creases in ((-0.8, crease), (0.8, None)):
        m = pool.add_mesh(cp, cn)
        if CC:                                # the six quads: their four edges each, all of Blender's crease 1
            pool.add_subdivision(m, args.levels, creases=None if creases is None else np.full(24, blender_crease(1.0)), scheme=args.scheme,
                                 polys=np.full(6, 4, np.int32))
        else:
            pool.add_subdivision(m, args.levels, creases=creases)
        pool.add_object(m, shift(x, 0.3, 0.2), 3)
pool.compose()
BVHTree().build()

os.makedirs(args.out, exist_ok=True)
t0 = time.perf_counter()
refitted = 0
for f in range(args.frames):
    phase = 2 * np.pi * f / args.frames
    pool.set_joints(obj, palette(1.2 * np.sin(phase)))
    pool.compose()
    refitted += BVHTree().update() == 'refit'
    FilmTable().clear()
    PathEngine().render(args.spp)
    img = FilmTable().get_display(layout='display')
    write_png(os.path.join(args.out, 'subdivide_%03d.png' % f), img)
    s, c = pool.subdiv_stats(), pool.compose_stats()
    print('frame %d: %d cage faces -> %d faces refined, %d of %d faces recomposed, mean byte %.2f'
          % (f, p.shape[0], s.refined_faces, c.recomposed, c.faces, float(img[..., :3].mean())))
dt = time.perf_counter() - t0
print('%d frames of %dx%d at %d spp in %.2f s (PNG writing included), %d refitted: written to %s'
      % (args.frames, args.size, args.size, args.spp, dt, refitted, args.out))

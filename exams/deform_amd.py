#!/usr/bin/env python3
'''
A tube that bends: a skinned cylinder with 8 joints and one morph target (a bulge round its middle) standing in the Cornell room,
the scene kept on the device.  The tube is a mesh of ModelPool's pool with a skin and a target, and an object of its table; each
frame is
    ModelPool().set_joints(tube, palette) + set_morph_weights -> compose() -> BVHTree().update() -> PathEngine().render() x spp
so nothing but the pose (8 matrices and a weight) crosses to the device: the corners are skinned there (csrc/deform.hip), the
tube's faces are composed again and the built tree is fitted to them (csrc/refit.hip).  With --rebuild a frame builds the tree
instead, for comparison.

    python exams/deform_amd.py [--frames 12] [--size 256] [--spp 8] [--out DIR] [--rebuild]
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
from ptina_amd import scenes                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=12)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--spp', type=int, default=8)
ap.add_argument('--out', default='.')
ap.add_argument('--rebuild', action='store_true', help='BVHTree().build() instead of update() at every frame')
args = ap.parse_args()

JOINTS, HEIGHT, RADIUS, RINGS, SIDES = 8, 2.4, 0.22, 64, 32


def tube():
    '''(p, n [k,3,3], joints, weights [k,3,4], bulge dp, dn [1,k,3,3]): rings of quads round the y axis, each corner bound to the
    two joints its height lies between'''
    y = np.linspace(0.0, HEIGHT, RINGS + 1)
    a = np.linspace(0.0, 2 * np.pi, SIDES + 1)
    yy, aa = np.meshgrid(y, a, indexing='ij')
    nrm = np.stack([np.cos(aa), np.zeros_like(aa), np.sin(aa)], axis=-1)
    pos = RADIUS * nrm + np.stack([np.zeros_like(yy), yy, np.zeros_like(yy)], axis=-1)
    at = np.clip(yy / HEIGHT * JOINTS - 0.5, 0.0, JOINTS - 1.0)              # joint j sits in the middle of its eighth
    j0 = np.floor(at).astype(np.int64)
    j1 = np.minimum(j0 + 1, JOINTS - 1)
    f = at - j0
    jt = np.stack([j0, j1, np.zeros_like(j0), np.zeros_like(j0)], axis=-1)
    wt = np.stack([1.0 - f, f, np.zeros_like(f), np.zeros_like(f)], axis=-1)
    bulge = np.exp(-((yy - 0.5 * HEIGHT) / (0.12 * HEIGHT)) ** 2)[..., None]
    dp = 0.8 * RADIUS * bulge * nrm

    def tris(x):
        c = x[:-1, :-1], x[1:, :-1], x[1:, 1:], x[:-1, 1:]
        return np.concatenate([np.stack([c[0], c[1], c[2]], axis=-2).reshape(-1, 3, x.shape[-1]),
                               np.stack([c[0], c[2], c[3]], axis=-2).reshape(-1, 3, x.shape[-1])])
    return tris(pos), tris(nrm), tris(jt), tris(wt), tris(dp)[None], np.zeros_like(tris(dp))[None]


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

wp, wn, wt, wm = scenes.cornell_walls()
pool = ModelPool()
for mtl in (0, 1, 2):
    pick = wm == mtl
    pool.add_object(pool.add_mesh(wp[pick], wn[pick], wt[pick]), np.eye(4), mtl)
p, n, joints, weights, dp, dn = tube()
mesh = pool.add_mesh(p, n)
pool.add_morph_targets(mesh, dp, dn)
pool.add_skin(mesh, joints, weights, JOINTS)
obj = pool.add_object(mesh, shift(0.0, 0.0, -0.3), 3)
pool.compose()
BVHTree().build()

os.makedirs(args.out, exist_ok=True)
t0 = time.perf_counter()
refitted = 0
for f in range(args.frames):
    phase = 2 * np.pi * f / args.frames
    pool.set_joints(obj, palette(1.2 * np.sin(phase)))
    pool.set_morph_weights(obj, [0.5 - 0.5 * np.cos(phase)])
    pool.compose()
    if args.rebuild:
        BVHTree().build()
    else:
        refitted += BVHTree().update() == 'refit'
    FilmTable().clear()
    PathEngine().render(args.spp)
    img = FilmTable().get_display(layout='display')
    write_png(os.path.join(args.out, 'deform_%03d.png' % f), img)
    d, c = pool.deform_stats(), pool.compose_stats()
    print('frame %d: %d corners deformed, %d of %d faces recomposed, mean byte %.2f'
          % (f, d.deformed_corners, c.recomposed, c.faces, float(img[..., :3].mean())))
dt = time.perf_counter() - t0
print('%d frames of %dx%d at %d spp in %.2f s (PNG writing included), %d refitted: written to %s'
      % (args.frames, args.size, args.size, args.spp, dt, refitted, args.out))

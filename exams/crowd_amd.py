#!/usr/bin/env python3
'''
A crowd that sways: many objects of ONE skinned tube (8 joints, a morph target that bulges its middle) standing in the Cornell room,
all bound to one clip at different offsets, the scene kept on the device.  Skeleton and clip are given once; each frame is
    ModelPool().set_time(t) -> compose() -> BVHTree().update() -> PathEngine().render() x spp
so nothing but the time crosses to the device: every object's pose is evaluated there (csrc/anim.hip), in one launch, the corners
are skinned there (csrc/deform.hip), the faces composed again and the built tree fitted to them (csrc/refit.hip).

    python exams/crowd_amd.py [--objects 24] [--frames 12] [--size 256] [--spp 8] [--out DIR] [--blend] [--props]

--blend: every object gets a second clip -- a faster, wider sway: the walk turns into a run -- blended in by
a cross-fade whose start is staggered over the crowd, and a few rigid props circle above it on object clips (set_motion).  Still
nothing but the time crosses to the device.

--props (section 3.17.3): every character carries a rigid prop, a small drum, on its top joint (set_parent with a joint, the joint's
bind matrix folded in with tools.skin.attach): the prop's matrix is world(character) . palette[top] . local, written on the device by
csrc/hierarchy.hip behind the poses.
'''
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptina_amd.things import *              # noqa: E402,F401,F403
from ptina_amd.engine.path import *         # noqa: E402,F401,F403
from ptina_amd.image import write_png       # noqa: E402
from ptina_amd.tools.anim import quaternion, rest_pose, track   # noqa: E402
from ptina_amd.tools.skin import attach     # noqa: E402
from ptina_amd import scenes                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--objects', type=int, default=24)
ap.add_argument('--frames', type=int, default=12)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--spp', type=int, default=8)
ap.add_argument('--out', default='.')
ap.add_argument('--blend', action='store_true', help='cross-fade every object from the walk to a run, staggered; rigid props on object clips')
ap.add_argument('--props', action='store_true', help='a rigid prop on the top joint of every character (set_parent)')
args = ap.parse_args()

JOINTS, HEIGHT, RADIUS, RINGS, SIDES, PERIOD = 8, 0.9, 0.05, 24, 12, 2.0


def tube():
    '''(p, n [k,3,3], joints, weights [k,3,4], bulge dp [1,k,3,3]): rings of quads round the y axis, each corner bound to the two
    joints its height lies between'''
    y = np.linspace(0.0, HEIGHT, RINGS + 1)
    a = np.linspace(0.0, 2 * np.pi, SIDES + 1)
    yy, aa = np.meshgrid(y, a, indexing='ij')
    nrm = np.stack([np.cos(aa), np.zeros_like(aa), np.sin(aa)], axis=-1)
    pos = RADIUS * nrm + np.stack([np.zeros_like(yy), yy, np.zeros_like(yy)], axis=-1)
    at = np.clip(yy / HEIGHT * JOINTS - 0.5, 0.0, JOINTS - 1.0)
    j0 = np.floor(at).astype(np.int64)
    f = at - j0
    jt = np.stack([j0, np.minimum(j0 + 1, JOINTS - 1), np.zeros_like(j0), np.zeros_like(j0)], axis=-1)
    wt = np.stack([1.0 - f, f, np.zeros_like(f), np.zeros_like(f)], axis=-1)
    dp = 0.8 * RADIUS * np.exp(-((yy - 0.5 * HEIGHT) / (0.12 * HEIGHT)) ** 2)[..., None] * nrm

    def tris(x):
        c = x[:-1, :-1], x[1:, :-1], x[1:, 1:], x[:-1, 1:]
        return np.concatenate([np.stack([c[0], c[1], c[2]], axis=-2).reshape(-1, 3, x.shape[-1]),
                               np.stack([c[0], c[2], c[3]], axis=-2).reshape(-1, 3, x.shape[-1])])
    return tris(pos), tris(nrm), tris(jt), tris(wt), tris(dp)[None]


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
Camera().set_perspective(scenes.BENCH_CAMERA)

wp, wn, wt, wm = scenes.cornell_walls()
pool = ModelPool()
for mtl in (0, 1, 2):
    pick = wm == mtl
    pool.add_object(pool.add_mesh(wp[pick], wn[pick], wt[pick]), np.eye(4), mtl)
p, n, joints, weights, dp = tube()
mesh = pool.add_mesh(p, n)
pool.add_morph_targets(mesh, dp)
pool.add_skin(mesh, joints, weights, JOINTS)
# the skeleton: a chain up the tube, at rest straight; the clip: every joint sways about z, the root hops, the bulge breathes
seg = HEIGHT / JOINTS
t, r, s = rest_pose(JOINTS)
t[1:, 1] = seg
inverse_bind = np.stack([shift(0, -j * seg, 0) for j in range(JOINTS)])
pool.add_skeleton(mesh, np.arange(JOINTS) - 1, t, r, s, inverse_bind)
times = np.linspace(0.0, PERIOD, 17)
phase = 2 * np.pi * times / PERIOD
tracks = [track(j, 'R', times, [quaternion([0, 0, 1], 1.2 * np.sin(a) / JOINTS) for a in phase]) for j in range(JOINTS)]
tracks.append(track(0, 'T', times, np.stack([0 * times, 0.08 * np.abs(np.sin(phase)), 0 * times], axis=1)))
tracks.append(track(None, 'W', times, (0.5 - 0.5 * np.cos(phase))[:, None]))
clip = pool.add_clip(mesh, tracks)
if args.blend:                                     # the run: half the period, twice the sway, a higher hop
    fast = np.linspace(0.0, 0.5 * PERIOD, 17)
    run = [track(j, 'R', fast, [quaternion([0, 0, 1], 2.4 * np.sin(a) / JOINTS) for a in phase]) for j in range(JOINTS)]
    run.append(track(0, 'T', fast, np.stack([0 * fast, 0.16 * np.abs(np.sin(phase)), 0 * fast], axis=1)))
    run_clip = pool.add_clip(mesh, run)
g = np.random.default_rng(1)
side = int(np.ceil(np.sqrt(args.objects)))
if args.props or args.blend:
    prop = pool.add_mesh(0.06 * (p - [0, 0.5 * HEIGHT, 0]) / RADIUS * [1, RADIUS / HEIGHT, 1], n)      # the tube squashed to a drum
characters = []
for o in range(args.objects):
    x, z = (o % side + 0.5) / side, (o // side + 0.5) / side
    obj = pool.add_object(mesh, shift(-0.8 + 1.6 * x, 0.0, -0.9 + 1.4 * z), 3)
    pool.set_animation(obj, clip, offset=g.uniform(0.0, PERIOD), speed=g.uniform(0.8, 1.25))
    characters.append(obj)
    if args.blend:                                 # the fade runs across the crowd: the first object starts at once, the last at half the period
        pool.set_animation_blend(obj, run_clip, offset=g.uniform(0.0, PERIOD), weight=(0.0, 1.0), fade=(0.5 * PERIOD * o / args.objects, 0.4 * PERIOD))
if args.props:                                     # a drum a little above the top joint's origin, in that joint's frame
    for o, obj in enumerate(characters):
        pool.set_parent(pool.add_object(prop, attach(inverse_bind[JOINTS - 1], shift(0, seg + 0.04, 0)), 1 + o % 2), obj, JOINTS - 1)
if args.blend:
    turn = [quaternion([0, 1, 0], a) for a in phase]
    for k in range(4):
        orbit = pool.add_object_clip([track(0, 'R', times, turn), track(0, 'T', times, np.stack([0 * times, 0.05 * np.sin(phase + k), 0 * times], axis=1))])
        pool.set_motion(pool.add_object(prop, np.eye(4), 1 + k % 2), orbit, offset=0.25 * k * PERIOD,
                        base=shift(0, 1.2, -0.2) @ shift(*(0.45 * np.array([np.cos(1.57 * k), 0, np.sin(1.57 * k)]))))
pool.compose()
BVHTree().build()

os.makedirs(args.out, exist_ok=True)
t0 = time.perf_counter()
refitted = 0
for f in range(args.frames):
    pool.set_time(PERIOD * f / args.frames)
    pool.compose()
    refitted += BVHTree().update() == 'refit'
    FilmTable().clear()
    PathEngine().render(args.spp)
    img = FilmTable().get_display(layout='display')
    write_png(os.path.join(args.out, 'crowd_%03d.png' % f), img)
    a, d, c, b, h = pool.anim_stats(), pool.deform_stats(), pool.compose_stats(), pool.anim_blend_stats(), pool.hierarchy_stats()
    print('frame %d: %d objects posed on the device (%d blended), %d moved there, %d carried by a parent, %d corners deformed, %d of %d faces recomposed, mean byte %.2f'
          % (f, a.evaluated_objects, b.evaluated_blended, b.evaluated_moved, h.evaluated, d.deformed_corners, c.recomposed, c.faces, float(img[..., :3].mean())))
dt = time.perf_counter() - t0
print('%d frames of %dx%d at %d spp in %.2f s (PNG writing included), %d refitted: written to %s'
      % (args.frames, args.size, args.size, args.spp, dt, refitted, args.out))

#!/usr/bin/env python3
'''
PTina's material-ball demo (reference exams/matball.py) driven through the `ptina.*` names, without the GUI: the
same objects and call order -- init_things, BruteEngine, FilmTable.set_size, ModelPool.load of a UV sphere,
BVHTree.build, then frames of Camera.set_perspective + BruteEngine.render + FilmTable.get_image.  The sphere asset
of the original is not distributed: the sphere is generated (ptina_amd.scenes.bumpy_sphere without the bumps).
The demo's `metallic` and `roughness` sliders are command-line arguments and set the sphere's material; the light
is the pool's default point light plus a grey world light, found by the brute-force engine only when a bounce ray
hits them.  The last image is written to a .npy.

    python exams/matball_amd.py [--size 256] [--frames 16] [--metallic 1] [--roughness 0] [--out matball.npy]
'''
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ptina                                 # noqa: E402,F401  (ptina.* -> ptina_amd.*)
from ptina.things import *                   # noqa: E402,F401,F403
from ptina.engine.brute import *             # noqa: E402,F401,F403
from ptina_amd import scenes                 # noqa: E402
import numpy as np                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--frames', type=int, default=16)
ap.add_argument('--metallic', type=float, default=1.0)
ap.add_argument('--roughness', type=float, default=0.0)
ap.add_argument('--out', default='matball.npy')
args = ap.parse_args()

ti.init(ti.gpu)
init_things()

BruteEngine()
FilmTable().set_size(args.size, args.size)

P, N, T, M = scenes.bumpy_sphere(segments=32, rings=16, bump=0.0, mtl=0)
vertices = np.concatenate([P, N, T], axis=2).reshape(-1, 8)
ModelPool().load(vertices, M)
MaterialPool().load([scenes.material(basecolor=(0.8, 0.8, 0.8), metallic=args.metallic, roughness=args.roughness)])
WorldLight().set([0.5, 0.5, 0.5, 1.0], -1)

BVHTree().build()

img = None
for frame in range(args.frames):
    if frame == 0:                           # gui.control.process_events(): the view was (re)set
        FilmTable().clear()
    Camera().set_perspective(scenes.BENCH_CAMERA)
    BruteEngine().render()
    img = FilmTable().get_image()

np.save(args.out, img)
print(f'{args.frames} brute-force frames at {args.size}x{args.size}, metallic {args.metallic}, roughness {args.roughness}: '
      f'mean {float(img[..., :3].mean()):.6f}, finite {bool(np.isfinite(img).all())} -> {args.out}')

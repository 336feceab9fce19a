#!/usr/bin/env python3
'''
PTina's Metropolis demo (reference exams/metropolis.py) driven through the `ptina.*` names, without
the GUI: the same objects and call order -- init_things, MLTPathEngine, FilmTable.set_size, pools,
BVHTree.build, Camera.set_perspective, LSP / Sigma written as 0-d fields, then frames of
FilmTable.clear + MLTPathEngine.reset (the demo's "camera moved" branch, once) and
MLTPathEngine.render + FilmTable.get_image.  The glTF asset of the original is not distributed, so
the scene comes from ptina_amd.scenes.  The last image is written to a .npy.

    python exams/metropolis_amd.py [--scene s978|s34] [--size 512] [--frames 16] [--lsp 0.25] [--sigma 0.01] [--out img.npy]
'''
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ptina                                 # noqa: E402,F401  (ptina.* -> ptina_amd.*)
from ptina.things import *                   # noqa: E402,F401,F403
from ptina.engine.mltpath import *           # noqa: E402,F401,F403
from ptina_amd import scenes                 # noqa: E402
import numpy as np                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--scene', default='s978')
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--frames', type=int, default=16)
ap.add_argument('--lsp', type=float, default=None)
ap.add_argument('--sigma', type=float, default=None)
ap.add_argument('--out', default='metropolis.npy')
args = ap.parse_args()

ti.init(ti.gpu)
init_things()
MLTPathEngine()
FilmTable().set_size(args.size, args.size)

vertices, mtlids, materials, images = scenes.get_scene(args.scene)
ModelPool().load(vertices, mtlids)
MaterialPool().load(materials)
ImagePool().load(images)
BVHTree().build()
Camera().set_perspective(scenes.BENCH_CAMERA)

if args.lsp is not None:
    MLTPathEngine().LSP[None] = args.lsp
if args.sigma is not None:
    MLTPathEngine().Sigma[None] = args.sigma

img = None
for frame in range(args.frames):
    if frame == 0:                           # gui.control.process_events(): the view was (re)set
        FilmTable().clear()
        MLTPathEngine().reset()
    MLTPathEngine().render()
    img = FilmTable().get_image()

np.save(args.out, img)
print(f'{args.frames} Metropolis frames of {MLTPathEngine().nchains} chains at {args.size}x{args.size}: '
      f'mean {float(img[..., :3].mean()):.6f}, finite {bool(np.isfinite(img).all())} -> {args.out}')

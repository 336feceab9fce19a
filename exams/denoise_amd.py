#!/usr/bin/env python3
'''
A low-sample render and its denoised image: the benchmark scene (exams/benchmark_amd.py) at 4 samples per pixel plus 2 frames
of the PreviewEngine (albedo into film pass 1, shading normal into pass 2: the reference's denoiser AOVs, engine/preview.py),
then FilmTable.get_image() and FilmTable.get_denoised() -- the edge-avoiding A-Trous filter run on the device, guided by those two
passes.  The reference leaves this step to Blender's compositor; here it is one call.  Writes noisy.npy and denoised.npy
([size][size][4] f32).  --variance SIGMA (try 4) also guides the filter by every pixel's own noise: the film is marked after half of
the samples, and get_denoised(variance=SIGMA) takes its colour tolerance from the two halves' difference.

    python exams/denoise_amd.py [--scene s978|s34] [--size 512] [--spp 4] [--preview 2] [--iterations 5] [--variance SIGMA] [--out DIR]
'''
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptina_amd.things import *              # noqa: E402,F401,F403
from ptina_amd.engine.path import *         # noqa: E402,F401,F403
from ptina_amd.engine.preview import PreviewEngine   # noqa: E402
from ptina_amd import scenes                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--scene', default='s978')
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--spp', type=int, default=4)
ap.add_argument('--preview', type=int, default=2)
ap.add_argument('--iterations', type=int, default=5)
ap.add_argument('--variance', type=float, default=None)
ap.add_argument('--out', default='.')
args = ap.parse_args()

ti.init(ti.cuda)
init_things()
PathEngine()
PreviewEngine()
FilmTable().set_size(args.size, args.size)

vertices, mtlids, materials, images = scenes.get_scene(args.scene)
ModelPool().load(vertices, mtlids)
MaterialPool().load(materials)
ImagePool().load(images)
BVHTree().build()
Camera().set_perspective(scenes.BENCH_CAMERA)

for i in range(args.spp):
    PathEngine().render()
    if args.variance and i + 1 == max(args.spp // 2, 1):
        FilmTable().mark()
for i in range(args.preview):
    PreviewEngine().render()
noisy = FilmTable().get_image()
denoised = FilmTable().get_denoised(iterations=args.iterations, variance=args.variance)

os.makedirs(args.out, exist_ok=True)
np.save(os.path.join(args.out, 'noisy.npy'), noisy)
np.save(os.path.join(args.out, 'denoised.npy'), denoised)
print(f'{args.scene} {args.size}x{args.size}, {args.spp} spp + {args.preview} preview frames: noisy.npy, denoised.npy in {args.out}; '
      f'mean |denoised - noisy| = {float(abs(denoised[..., :3] - noisy[..., :3]).mean()):.4f}')

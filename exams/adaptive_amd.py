#!/usr/bin/env python3
'''
Adaptive sampling: the Cornell benchmark scene rendered to the same noise threshold twice -- by PathEngine.render_until(), which
samples every pixel of every frame until the whole film has passed, and by PathEngine.render_adaptive(), which after each check
samples only the pixels whose own estimate has not passed yet (FilmTable.select: Cycles' criterion, so --noise is Blender's noise
threshold, and with dilate their neighbours) -- and the samples both took.  Written as PNGs with ptina_amd.image.write_png: the
adaptive image (FilmTable.get_display) and the per-pixel sample-count map (FilmTable.get_samples: black = the fewest samples a
pixel took, white = the most).  The reference's scripts count samples (exams/benchmark.py renders a fixed number of frames).

    python exams/adaptive_amd.py [--scene s978|s34] [--size 512] [--noise 0.05] [--min-spp 16] [--max-spp 4096] [--dilate 1]
                                 [--switch S] [--out DIR]
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
ap.add_argument('--scene', default='s978')
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--noise', type=float, default=0.05)
ap.add_argument('--min-spp', type=int, default=16)
ap.add_argument('--max-spp', type=int, default=4096)
ap.add_argument('--dilate', type=int, default=1)
ap.add_argument('--switch', type=float, default=None)
ap.add_argument('--out', default='.')
args = ap.parse_args()

ti.init(ti.cuda)
init_things()
PathEngine()
FilmTable().set_size(args.size, args.size)

vertices, mtlids, materials, images = scenes.get_scene(args.scene)
ModelPool().load(vertices, mtlids)
MaterialPool().load(materials)
ImagePool().load(images)
BVHTree().build()
Camera().set_perspective(scenes.BENCH_CAMERA)

FilmTable().clear()
t0 = time.perf_counter()
until = PathEngine().render_until(args.noise, args.max_spp, min_spp=args.min_spp)
FilmTable().get_raw()
t_until = time.perf_counter() - t0
valid = until.history[-1][1].valid
print(f'render_until:    {"converged" if until.converged else "NOT converged"} at {until.spp} spp, {until.spp * valid} samples, {t_until:.3f} s')

FilmTable().clear()
t0 = time.perf_counter()
adaptive = PathEngine().render_adaptive(args.noise, args.max_spp, min_spp=args.min_spp, dilate=args.dilate, switch=args.switch)
count = FilmTable().get_samples()
t_adaptive = time.perf_counter() - t0
for level, st, active, kind in adaptive.history:
    print(f'{level:6d} spp after a {kind} pass: {st.above} of {st.valid} pixels above {args.noise:g}, {active} listed')
print(f'render_adaptive: {"converged" if adaptive.converged else "NOT converged"} at level {adaptive.spp}, {adaptive.samples} samples, '
      f'{t_adaptive:.3f} s: {adaptive.samples / max(until.spp * valid, 1):.3f} of render_until\'s samples')
assert adaptive.samples == int(count.astype(np.int64).sum())

os.makedirs(args.out, exist_ok=True)
write_png(os.path.join(args.out, 'adaptive.png'), FilmTable().get_display(layout='display'))
lo, hi = float(count.min()), float(count.max())
grey = ((np.swapaxes(count, 0, 1)[::-1] - lo) / max(hi - lo, 1.0) * 255).astype(np.uint8)
rgba = np.ascontiguousarray(np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=-1))
write_png(os.path.join(args.out, 'sample_count.png'), rgba)
print(f'{args.scene} {args.size}x{args.size}: adaptive.png and sample_count.png (black {lo:g}, white {hi:g} samples) written to {args.out}')

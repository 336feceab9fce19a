#!/usr/bin/env python3
'''
Render until the picture is converged instead of to a hand-picked sample count: the benchmark scene through
PathEngine.render_until() -- a doubling schedule that asks the device after each doubling how noisy the film still is
(FilmTable.get_noise: Cycles' adaptive-sampling criterion, so --noise is Blender's noise threshold) and stops when at most
--fraction of the pixels are above it -- then the final image (FilmTable.get_display) and the error map of the last check, both
written as PNGs with ptina_amd.image.write_png, after one more doubling that asks for the map.  In the map black is converged and white is --noise x 4 or worse.  The reference's
scripts count samples (exams/benchmark.py renders a fixed number of frames).

    python exams/converge_amd.py [--scene s978|s34] [--size 512] [--noise 0.05] [--fraction 0.05] [--min-spp 16] [--max-spp 4096]
                                 [--out DIR]
'''
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptina_amd.things import *              # noqa: E402,F401,F403
from ptina_amd.engine.path import *         # noqa: E402,F401,F403
from ptina_amd.image import write_png       # noqa: E402
from ptina_amd import scenes                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--scene', default='s978')
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--noise', type=float, default=0.05)
ap.add_argument('--fraction', type=float, default=0.05)
ap.add_argument('--min-spp', type=int, default=16)
ap.add_argument('--max-spp', type=int, default=4096)
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
result = PathEngine().render_until(args.noise, args.max_spp, min_spp=args.min_spp, fraction=args.fraction)
for spp, st in result.history:
    print(f'{spp:6d} spp: mean e {st.mean:.5f}, max {st.max:.4f}, {100 * st.fraction:.2f} % of {st.valid} pixels above {args.noise:g}')
print(f'{"converged" if result.converged else "NOT converged"} at {result.spp} spp')

# the loop asks for the statistics only (32 bytes per check); for the picture of WHERE the noise is, one more doubling, with the map
PathEngine().render(result.spp)
last = FilmTable().get_noise(args.noise, map=True)
print(f'{2 * result.spp:6d} spp: mean e {last.mean:.5f}, max {last.max:.4f}, {100 * last.fraction:.2f} % above (the film and the map written)')

os.makedirs(args.out, exist_ok=True)
write_png(os.path.join(args.out, 'converged.png'), FilmTable().get_display(layout='display'))
grey = (np.clip(np.swapaxes(last.map, 0, 1)[::-1] / (4 * args.noise), 0, 1) * 255).astype(np.uint8)
rgba = np.ascontiguousarray(np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=-1))
write_png(os.path.join(args.out, 'noise_map.png'), rgba)
print(f'{args.scene} {args.size}x{args.size}: converged.png and noise_map.png written to {args.out}')

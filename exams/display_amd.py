#!/usr/bin/env python3
'''
The benchmark scene as a picture: a few samples per pixel plus two frames of the PreviewEngine, then FilmTable.get_display() --
the film metered, tone-mapped (ACES), sRGB-encoded, dithered and quantised to 8 bits on the device -- once from film pass 0 and
once behind the denoiser (denoised=True), each written as a PNG with ptina_amd.image.write_png (zlib and struct only).  The
reference's scripts end in ti.imshow of linear radiance; its tone mapping (ptina/wip/tonemapping.py) was never wired in -- that
functor is --op ptina --exposure 0.3 --transfer gamma here.

    python exams/display_amd.py [--scene s978|s34] [--size 512] [--spp 4] [--preview 2] [--op aces] [--transfer srgb]
                                [--exposure AUTO] [--out DIR]
'''
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptina_amd.things import *              # noqa: E402,F401,F403
from ptina_amd.engine.path import *         # noqa: E402,F401,F403
from ptina_amd.engine.preview import PreviewEngine   # noqa: E402
from ptina_amd.image import write_png       # noqa: E402
from ptina_amd import scenes                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--scene', default='s978')
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--spp', type=int, default=4)
ap.add_argument('--preview', type=int, default=2)
ap.add_argument('--op', default='aces', choices=['linear', 'ptina', 'reinhard', 'aces'])
ap.add_argument('--transfer', default='srgb', choices=['srgb', 'gamma'])
ap.add_argument('--exposure', type=float, default=None, help='manual exposure (default: metered)')
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
for i in range(args.preview):
    PreviewEngine().render()

os.makedirs(args.out, exist_ok=True)
kw = dict(op=args.op, transfer=args.transfer, exposure=args.exposure, layout='display')
for name, denoised in (('display.png', False), ('display_denoised.png', True)):
    img = FilmTable().get_display(denoised=denoised, **kw)
    write_png(os.path.join(args.out, name), img)
    print(f'{name}: {img.shape[1]}x{img.shape[0]} RGBA8, exposure {FilmTable().last_exposure:.6g}'
          f' ({"metered" if args.exposure is None else "given"}), mean byte {float(img[..., :3].mean()):.2f}')
print(f'{args.scene} {args.size}x{args.size}, {args.spp} spp + {args.preview} preview frames, {args.op} / {args.transfer}: written to {args.out}')

#!/usr/bin/env python3
'''
An orbit: the camera circles the 978-triangle scene at a few samples a frame, once starting every frame from an empty film
(FilmTable().clear(), what the other exams do) and once carrying the accumulated film over to the new view:
    render x spp -> get_display() -> FilmTable().keep_history() -> Camera().set_perspective(next) -> FilmTable().reproject() -> render ...
reproject() resamples the film on the device (csrc/history_kernel.hip, history.hip): every pixel takes the sums of the place where
the surface point it sees now lay in the view before; what was hidden, off-screen or another object starts from zero, and a pixel's
history counts for at most --max-history samples, so the new samples keep up with the moving view.  Both runs write their PNGs;
the second prints how much of each frame kept its history.  The reference's add-on clears at every change of the view.

    python exams/temporal_amd.py [--frames 24] [--size 256] [--spp 4] [--degrees 60] [--max-history 32] [--out DIR]
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
ap.add_argument('--frames', type=int, default=24)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--spp', type=int, default=4)
ap.add_argument('--degrees', type=float, default=60.0, help='the arc of the orbit, centred on the benchmark view')
ap.add_argument('--max-history', type=float, default=32.0)
ap.add_argument('--out', default='.')
args = ap.parse_args()

ti.init(ti.cuda)
init_things()
PathEngine()
FilmTable().set_size(args.size, args.size)
vertices, mtlids, materials, images = scenes.scene_s978()
ModelPool().load(vertices, mtlids)
MaterialPool().load(materials)
ImagePool().load(images)
BVHTree().build()


def orbit(degrees):
    '''the benchmark camera carried about the vertical axis through the room's centre'''
    th = np.radians(degrees)
    turn = np.array([[np.cos(th), 0, np.sin(th), 0], [0, 1, 0, 0], [-np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1.0]])
    return np.asarray(scenes.BENCH_CAMERA, np.float64) @ turn


os.makedirs(args.out, exist_ok=True)
film = FilmTable()
for label, carry in (('clear', False), ('reproject', True)):
    film.clear()
    film.drop_history()
    t0 = time.perf_counter()
    kept = []
    for f in range(args.frames):
        Camera().set_perspective(orbit(args.degrees * (f / max(args.frames - 1, 1) - 0.5)))
        if carry and f:
            kept.append(film.reproject(max_history=args.max_history).kept_fraction)
        else:
            film.clear()
        PathEngine().render(args.spp)
        img = film.get_display(layout='display')
        write_png(os.path.join(args.out, 'orbit_%s_%03d.png' % (label, f)), img)
        if carry:
            film.keep_history()
    dt = time.perf_counter() - t0
    print('%s: %d frames of %dx%d at %d spp in %.2f s (PNG writing included)' % (label, args.frames, args.size, args.size, args.spp, dt))
    if kept:
        keep_ms, reproject_ms, _ = film.history_kernel_time()
        print('   history kept in %.1f %% of the pixels on average (least %.1f %%); keep_history %.3f ms and reproject %.3f ms a frame on the device'
              % (100 * sum(kept) / len(kept), 100 * min(kept), keep_ms / args.frames, reproject_ms / len(kept)))

#!/usr/bin/env python3
'''
What FilmTable.get_display costs (csrc/display.hip) on the s978 scene at 4 frames + 2 preview frames,
512x512 and 2048x2048, against the read-back the parent already has: the same run's get_image(0) (16 bytes per pixel over PCIe,
linear f32), and get_image(0) followed by the numpy conversion a user writes today (clip, gamma, scale, cast, transpose, flip --
what ti.imwrite does plus a transfer curve).  Per film size one JSON line with, for each variant, the median wall time of --repeat
calls after two warm-up calls and, for get_display, the HIP-event time of its kernels (mpt_display_kernel_time):

  get_display: FILM and DISPLAY layout x metered and manual exposure, from pass 0; DISPLAY layout behind the denoiser.

    python tools/display_bench.py [--repeat 20] [--sizes 512 2048]
'''
import argparse
import json

import numpy as np

from benchlib import setup, median, wall_ms


def numpy_display(img):
    '''what a user writes today behind get_image: ti.imwrite's clip, transpose and flip, with a gamma curve in front of the cast'''
    a = np.clip(img[..., :3], 0, 1) ** np.float32(1 / 2.2)
    return (np.swapaxes(a, 0, 1)[::-1] * 255).astype(np.uint8)


def bench(size, repeat):
    path, preview, film = setup(size, preview=True)
    path.render(4)
    preview.render(2)
    film.get_image()
    out = {'metric': 'display_ms', 'scene': 's978', 'size': size, 'frames': 4, 'preview_frames': 2, 'repeat': repeat,
           'columns': ['wall median', 'wall min', 'kernel median']}
    out['get_image'] = list(wall_ms(lambda: film.get_image(0), repeat))
    out['get_image+numpy'] = list(wall_ms(lambda: numpy_display(film.get_image(0)), repeat))
    variants = {
        'film auto': dict(layout='film'), 'film manual': dict(layout='film', exposure=0.3),
        'display auto': dict(layout='display'), 'display manual': dict(layout='display', exposure=0.3),
        'display auto denoised': dict(layout='display', denoised=True),
    }
    for name, kw in variants.items():
        kern = []
        film.display_kernel_time()
        w = wall_ms(lambda: film.get_display(**kw), repeat, after=lambda: kern.append(film.display_kernel_time()[0]))
        out['get_display ' + name] = list(w) + [round(median(kern[2:]), 4)]
    # the same run's get_image once more, behind everything: drift of the yardstick itself
    out['get_image_again'] = list(wall_ms(lambda: film.get_image(0), repeat))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--sizes', type=int, nargs='*', default=[512, 2048])
    args = ap.parse_args()
    for size in args.sizes:
        bench(size, args.repeat)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
'''
What one convergence check costs (csrc/noise.hip) on the s978 scene at 4 + 4 frames, 512x512 and 2048x2048:
FilmTable.get_noise() -- statistics only, with the map, and re-marking -- against the only route to the same estimate without it:
two get_raw() read-backs (the film now, and the film at the mark, which a caller without a device mark has to read back when it
takes it) and the numpy restatement tests/noise_ref.py.  Per film size one JSON line with, for each variant, the median and the
least wall time of --repeat calls after two warm-up calls and, for get_noise, the median HIP-event time of its kernels
(mpt_noise_kernel_time) with what that is in bytes per second: 32 bytes read per pixel, 4 more written with the map, 16 more when
re-marking.  A re-marking check leaves no sample behind the mark, so a frame is rendered (and waited for) before each, outside the
timed call.

    python tools/noise_bench.py [--repeat 20] [--sizes 512 2048]
'''
import argparse
import json
import os
import sys

from benchlib import ROOT, setup, median, wall_ms

sys.path.insert(0, os.path.join(ROOT, 'tests'))


def bench(size, repeat):
    from noise_ref import noise_ref
    from ptina_amd.common import ctx
    path, film = setup(size)
    npix = size * size
    path.render(4)
    film.mark()
    mark = film.get_raw(0)
    path.render(4)
    film.get_image()
    out = {'metric': 'noise_check_ms', 'scene': 's978', 'size': size, 'frames': '4+4', 'repeat': repeat,
           'columns': ['wall median', 'wall min', 'kernel median', 'kernel GB/s']}
    r = film.get_noise(0.05)
    _, _, st = noise_ref(film.get_raw(0), mark, 0.05)
    out['agree'] = bool((r.valid, r.above) == (st.valid, st.above) and r.max == float(st.max))
    out['mean_e'] = round(r.mean, 5)

    # the route without the feature, first (the mark is still the one read back above)
    out['get_raw'] = list(wall_ms(lambda: film.get_raw(0), repeat))

    def by_hand():
        new_mark = film.get_raw(0)              # (stands for the read-back that took the mark)
        noise_ref(film.get_raw(0), mark, 0.05)
        return new_mark
    out['2 x get_raw + numpy'] = list(wall_ms(by_hand, max(3, repeat // 4)))

    def one_more_frame():
        path.render(1)
        ctx().call('mpt_synchronize')
    variants = {'stats': (dict(), 32), 'stats+map': (dict(map=True), 36), 'stats remark': (dict(remark=True), 48),
                'stats+map remark': (dict(map=True, remark=True), 52)}
    for name, (kw, bytes_per_pixel) in variants.items():
        kern = []

        film.noise_kernel_time()
        w = wall_ms(lambda: film.get_noise(0.05, **kw), repeat, one_more_frame if kw.get('remark') else None,
                    lambda: kern.append(film.noise_kernel_time()[0]))
        k = median(kern[2:])
        out['get_noise ' + name] = list(w) + [round(k, 4), round(npix * bytes_per_pixel / (k * 1e-3) / 1e9, 1) if k > 0 else None]
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

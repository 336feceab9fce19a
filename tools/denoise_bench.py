#!/usr/bin/env python3
'''
What FilmTable.get_denoised costs (csrc/denoise.hip) on the s978 scene at 4 frames + 2 preview frames,
512x512 and 2048x2048, timed by the HIP events around the filter's kernels (mpt_denoise_kernel_time), median of --repeat calls
after two warm-up calls.  Per film size, one JSON line with

  - ms per call at iterations 0 .. 5: iterations = 0 is the resolve pass alone on the same film (the streaming pass over the
    same pixels the parent already has: the yardstick), and the step from k to k + 1 iterations is the iteration of stride 2^k;
  - the same with every stride as gathers (option "denoise_lds" = 0) beside the default (strides 1 and 2 from a tile in LDS);
  - denoise ms / resolve ms at the defaults;
  - the bytes an iteration must move (read e, a, n once, write e once: 64 bytes per pixel) over its time, as a fraction of the
    HBM peak (8.0 TB/s by the data sheet; 6.29 TB/s is what a float4 copy reaches).

and then the headline step -- render(32) + read-back at 512x512 -- as wall time per step with get_image and with get_denoised
in its place.  --variance SIGMA times the variance-guided mode instead (get_denoised(variance=SIGMA)): the
same film -- the mark is taken after 2 of the 4 frames either way -- and 72 bytes per pixel and iteration (v read and written too).

    python tools/denoise_bench.py [--repeat 20] [--sizes 512 2048] [--steps 50] [--variance 4]
'''
import argparse
import json
import time

from benchlib import setup, median

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def call_ms(film, repeat, **kw):
    for _ in range(2):
        film.get_denoised(**kw)
    film.denoise_kernel_time()
    ms = []
    for _ in range(repeat):
        film.get_denoised(**kw)
        t, n = film.denoise_kernel_time()
        assert n == 1
        ms.append(t)
    return median(ms)


def kernels(size, repeat, variance=None):
    from ptina_amd.common import ctx
    path, preview, film = setup(size, preview=True)
    path.render(2)
    film.mark()
    path.render(2)
    preview.render(2)
    film.get_image()
    out = {'metric': 'denoise_kernel_ms', 'scene': 's978', 'size': size, 'frames': 4, 'preview_frames': 2, 'repeat': repeat,
           'variance': variance}
    for lds in (1, 0):
        ctx().set_option('denoise_lds', lds)
        out['ms_per_call_lds%d' % lds] = [round(call_ms(film, repeat, iterations=k, variance=variance), 4) for k in range(6)]
    ctx().set_option('denoise_lds', 1)
    for key in ('ms_per_call_lds1', 'ms_per_call_lds0'):
        t = out[key]
        out[key.replace('ms_per_call', 'ms_per_iteration')] = [round(t[k + 1] - t[k], 4) for k in range(1, 5)]
    t = out['ms_per_call_lds1']
    out['resolve_ms'] = t[0]
    out['denoise_ms'] = t[5]
    out['denoise_over_resolve'] = round(t[5] / t[0], 2)
    # (prologue + first iteration + epilogue) = t[1]; an iteration of stride 2^k = t[k + 1] - t[k] for k >= 1
    out['ms_first_iteration_with_prologue_and_epilogue'] = t[1]
    it = (t[5] - t[1]) / 4
    nbytes = (72.0 if variance else 64.0) * size * size
    out['mean_ms_per_iteration'] = round(it, 4)
    out['iteration_bytes'] = int(nbytes)
    out['iteration_bytes_per_s_over_hbm_spec'] = round(nbytes / (it * 1e-3) / HBM_SPEC, 3)
    out['iteration_bytes_per_s_over_hbm_copy'] = round(nbytes / (it * 1e-3) / HBM_COPY, 3)
    print(json.dumps(out), flush=True)


def headline(steps, variance=None):
    path, preview, film = setup(512, preview=True)
    preview.render(2)
    path.render(32)
    film.mark()
    out = {'metric': 'headline_step_ms', 'scene': 's978', 'size': 512, 'spp': 32, 'steps': steps, 'variance': variance}
    for name, read in (('get_image', film.get_image), ('get_denoised', lambda: film.get_denoised(variance=variance)), ('get_image_again', film.get_image)):
        for _ in range(3):
            path.render(32)
            read()
        t0 = time.perf_counter()
        for _ in range(steps):
            path.render(32)
            read()
        out['ms_per_step_' + name] = round((time.perf_counter() - t0) / steps * 1e3, 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--sizes', type=int, nargs='*', default=[512, 2048])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--variance', type=float, default=None, help='time the variance-guided mode at this sigma_variance')
    args = ap.parse_args()
    for size in args.sizes:
        kernels(size, args.repeat, args.variance)
    if args.steps > 0:
        headline(args.steps, args.variance)


if __name__ == '__main__':
    main()

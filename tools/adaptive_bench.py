#!/usr/bin/env python3
'''
What adaptive sampling costs and saves (csrc/adapt_select.hip, csrc/adapt_kernel.hip) on the s978 scene at
512x512, production build.  Medians of --repeat calls after three warm-up calls, from HIP-event times (mpt_adapt_kernel_time,
mpt_kernel_time, mpt_noise_kernel_time).  Three JSON lines:

  (a) samples/s of PathEngine.render_selected(--frames) with every pixel listed, with the noisiest 10 % and the noisiest 1 % listed
      (by FilmTable.get_noise's map at 16 + 16 frames: what a selection lists), beside PathEngine.render(--frames) on the same
      context.  The ratio at "every pixel listed" is the break-even share of active pixels: engine.DEFAULT_SWITCH is that ratio
      rounded down to a multiple of 0.05 (and 0.05 if it comes out lower).
  (b) the selection's time with and without dilate, beside get_noise's statistics.
  (c) end to end: wall time and samples of render_until(--noise, --max-spp) and of render_adaptive(--noise, --max-spp), each on a
      cleared film (--e2e-repeat times; the Sobol sampler is reset before each, so every run renders the same frames).

    python tools/adaptive_bench.py [--size 512] [--frames 32] [--repeat 20] [--noise 0.05] [--max-spp 4096] [--e2e-repeat 3]
'''
import argparse
import json
import math
import time

from benchlib import setup, median, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--noise', type=float, default=0.05)
    ap.add_argument('--max-spp', type=int, default=4096)
    ap.add_argument('--e2e-repeat', type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    from ptina_amd.common import ctx
    from ptina_amd.sampling.sobol import SobolSampler
    import ptina_amd.engine as engine
    path, film = setup(args.size)
    npix, warm = args.size * args.size, 3

    # ---- (a) the list kernel's rate against the production kernels'
    path.render(16)
    film.mark()
    path.render(16)
    e = film.get_noise(args.noise, map=True).map.reshape(-1)
    order = np.argsort(-e, kind='stable')
    out = {'metric': 'adaptive_list_pass', 'scene': 's978', 'size': args.size, 'frames': args.frames, 'repeat': args.repeat}
    film.get_image()
    ctx().kernel_time()
    ms = []
    for _ in range(args.repeat + warm):
        path.render(args.frames)
        film.get_image()
        ms.append(ctx().kernel_time()[0])
    pms = median(ms[warm:])
    out['path_kernel_ms'] = round(pms, 4)
    out['path_Msamples_per_s'] = round(npix * args.frames / (pms * 1e-3) / 1e6, 1)
    for label, share in (('every pixel', 1.0), ('noisiest 10 %', 0.1), ('noisiest 1 %', 0.01)):
        n = max(1, int(round(share * npix)))
        film.set_selection(np.sort(order[:n]))
        film.adapt_kernel_time()
        ms = []
        for _ in range(args.repeat + warm):
            path.render_selected(args.frames)
            ms.append(film.adapt_kernel_time()[1])
        k = median(ms[warm:])
        rate = n * args.frames / (k * 1e-3) / 1e6
        out[label] = {'listed': n, 'kernel_ms': round(k, 4), 'Msamples_per_s': round(rate, 1), 'of_path_engine': round(rate / out['path_Msamples_per_s'], 4)}
    r = out['every pixel']['of_path_engine']
    out['break_even_share'] = r
    out['switch_default'] = max(0.05, math.floor(r / 0.05 + 1e-9) * 0.05)
    out['switch_in_code'] = engine.DEFAULT_SWITCH
    print(json.dumps(out), flush=True)

    # ---- (b) the selection beside the noise check
    film.clear()
    path.render(16)
    film.mark()
    path.render(16)
    film.get_image()
    out = {'metric': 'adaptive_select_ms', 'scene': 's978', 'size': args.size, 'frames': '16+16', 'repeat': args.repeat,
           'columns': ['wall median', 'wall min', 'kernel median']}
    kern = []
    film.noise_kernel_time()
    w = wall_ms(lambda: film.get_noise(args.noise), args.repeat, None, lambda: kern.append(film.noise_kernel_time()[0]))
    out['get_noise stats'] = list(w) + [round(median(kern[2:]), 4)]
    for dilate in (0, 1):
        kern = []
        film.adapt_kernel_time()
        w = wall_ms(lambda: film.select(args.noise, dilate), args.repeat, None, lambda: kern.append(film.adapt_kernel_time()[0]))
        st, count = film.select(args.noise, dilate)
        out['select dilate=%d' % dilate] = list(w) + [round(median(kern[2:]), 4)]
        out['listed dilate=%d' % dilate] = [count, st.above, st.valid]
    print(json.dumps(out), flush=True)

    # ---- (c) end to end
    out = {'metric': 'adaptive_end_to_end', 'scene': 's978', 'size': args.size, 'noise': args.noise, 'max_spp': args.max_spp,
           'switch': engine.DEFAULT_SWITCH, 'runs': args.e2e_repeat}
    for name in ('render_until', 'render_adaptive'):
        walls = []
        for _ in range(args.e2e_repeat):
            SobolSampler().reset()
            film.clear()
            ctx().call('mpt_synchronize')
            t0 = time.perf_counter()
            res = getattr(path, name)(args.noise, args.max_spp)
            ctx().call('mpt_synchronize')
            walls.append((time.perf_counter() - t0) * 1e3)
        valid = res.history[-1][1].valid
        samples = res.samples if name == 'render_adaptive' else res.spp * valid
        out[name] = {'wall_ms': [round(x, 2) for x in walls], 'spp': res.spp, 'converged': res.converged, 'samples': samples,
                     'checks': len(res.history)}
        if name == 'render_adaptive':
            out[name]['passes'] = [(h[0], h[1].above, h[2], h[3]) for h in res.history]
    out['samples_ratio'] = round(out['render_adaptive']['samples'] / out['render_until']['samples'], 4)
    out['wall_ratio'] = round(min(out['render_adaptive']['wall_ms']) / min(out['render_until']['wall_ms']), 4)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()

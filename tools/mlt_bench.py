#!/usr/bin/env python3
'''
Metropolis engine throughput (MLTPathEngine, csrc/mlt_kernel.hip) on the s978 scene at 512x512, production build:
K iterations of 2^18 chains after W warm-up iterations, timed by the HIP events around the chain kernels and the
splat passes, and the PathEngine's samples/s on the same scene in the same process for scale.  Prints one JSON line.

    python tools/mlt_bench.py [--iters 64] [--warmup 8] [--nchains 262144] [--size 512] [--frames 32]
'''
import argparse
import json
import time

from benchlib import setup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=64)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--nchains', type=int, default=2**18)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--scene', default='s978')
    args = ap.parse_args()

    eng, _ = setup(args.size, args.scene)
    from ptina_amd.common import ctx
    from ptina_amd.things import FilmTable
    from ptina_amd.engine.mltpath import MLTPathEngine
    mlt = MLTPathEngine(nchains=args.nchains)

    def mlt_times():
        return ctx().timer('mpt_mlt_kernel_time', segments=2)

    mlt.render(args.warmup)
    FilmTable().get_raw()
    mlt_times()
    t0 = time.perf_counter()
    mlt.render(args.iters)
    FilmTable().get_raw()
    wall = time.perf_counter() - t0
    chain_ms, splat_ms, launches = mlt_times()
    paths = args.nchains * args.iters

    FilmTable().clear()
    eng.render(args.frames)
    FilmTable().get_image()
    ctx().kernel_time()
    t0 = time.perf_counter()
    eng.render(args.frames)
    FilmTable().get_image()
    pwall = time.perf_counter() - t0
    pms, _ = ctx().kernel_time()
    samples = args.size * args.size * args.frames

    print(json.dumps({
        'metric': 'mlt_paths_per_s', 'scene': args.scene, 'size': args.size, 'nchains': args.nchains, 'iters': args.iters,
        'launches': launches, 'chain_ms': round(chain_ms, 3), 'splat_ms': round(splat_ms, 3),
        'chain_us_per_iter': round(1e3 * chain_ms / args.iters, 2), 'splat_us_per_iter': round(1e3 * splat_ms / args.iters, 2),
        'mlt_Mpaths_per_s': round(paths / ((chain_ms + splat_ms) / 1e3) / 1e6, 1),
        'mlt_Mpaths_per_s_wall': round(paths / wall / 1e6, 1),
        'path_Msamples_per_s': round(samples / (pms / 1e3) / 1e6, 1) if pms > 0 else None,
        'path_Msamples_per_s_wall': round(samples / pwall / 1e6, 1),
    }))


if __name__ == '__main__':
    main()

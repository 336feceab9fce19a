#!/usr/bin/env python3
'''
Brute-force engine throughput (BruteEngine, csrc/brute_kernel.hip) on the s978 scene at 512x512, production build:
`--frames` frames in one batch after one warm-up batch, timed by the HIP events around the kernel (mpt_brute_kernel_time),
beside the PathEngine's samples/s on the same scene in the same process.  Prints one JSON line.

With --bias: how far the PathEngine's expectation lies from the brute-force one in scenes WITH pool lights (the reference's
MIS weights and light pdfs are not those of an unbiased estimator: DESIGN.md section 3.8), measured on the 34-triangle
scene with its default point light and with the area + point light pair of the reference fixtures: mean radiance of both
engines over --blocks blocks of --spp samples at 64x64, and the standard error of each.  A second JSON line.

    python tools/brute_bench.py [--frames 32] [--size 512] [--scene s978] [--bias] [--blocks 16] [--spp 256]
'''
import argparse
import json
import os
import sys
import time

import benchlib
from benchlib import ROOT, median


def setup(scene, size, lights=None, world=None):
    from ptina_amd.things import LightPool, WorldLight
    from ptina_amd.engine.brute import BruteEngine
    path, _ = benchlib.setup(size, scene)
    if lights is not None:
        LightPool().clear()
        for l in lights:
            LightPool().add(*l)
    if world is not None:
        WorldLight().set(*world)
    return path, BruteEngine()


def rate(args):
    from ptina_amd.common import ctx
    from ptina_amd.things import FilmTable
    path, brute = setup(args.scene, args.size)
    samples = args.size * args.size * args.frames
    brute.render(args.frames)
    FilmTable().get_raw()
    brute.kernel_time()
    runs = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        brute.render(args.frames)
        FilmTable().get_raw()
        wall = time.perf_counter() - t0
        ms, launches = brute.kernel_time()
        runs.append((ms, wall, launches))
    FilmTable().clear()
    path.render(args.frames)
    FilmTable().get_image()
    ctx().kernel_time()
    pruns = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        path.render(args.frames)
        FilmTable().get_image()
        pwall = time.perf_counter() - t0
        pms, _ = ctx().kernel_time()
        pruns.append((pms, pwall))
    ms = median([r[0] for r in runs])
    pms = median([r[0] for r in pruns])
    print(json.dumps({
        'metric': 'brute_samples_per_s', 'scene': args.scene, 'size': args.size, 'frames': args.frames, 'launches': runs[0][2],
        'brute_kernel_ms': [round(r[0], 3) for r in runs], 'brute_Msamples_per_s': round(samples / (ms / 1e3) / 1e6, 1),
        'brute_Msamples_per_s_wall': round(samples / min(r[1] for r in runs) / 1e6, 1),
        'path_kernel_ms': [round(r[0], 3) for r in pruns], 'path_Msamples_per_s': round(samples / (pms / 1e3) / 1e6, 1) if pms > 0 else None,
        'path_Msamples_per_s_wall': round(samples / min(r[1] for r in pruns) / 1e6, 1),
    }), flush=True)


def bias(args):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import make_reference_path_golden as G
    from ptina_amd.things import FilmTable
    out = {'metric': 'path_minus_brute_mean_radiance', 'size': 64, 'blocks': args.blocks, 'spp': args.spp}
    for key in ('s34', 'lobes'):
        scene, lights, world = G.scene_of(key)
        path, brute = setup(scene, 64, lights, world)
        res = {}
        for label, eng in (('path', path), ('brute', brute)):
            m = []
            for _ in range(args.blocks):
                FilmTable().clear()
                eng.render(args.spp)
                raw = FilmTable().get_raw().astype(np.float64)
                m.append(float((raw[:, :3] / raw[:, 3:4]).mean()))
            res[label] = (float(np.mean(m)), float(np.std(m, ddof=1) / np.sqrt(len(m))))
        d = res['path'][0] - res['brute'][0]
        se = float(np.hypot(res['path'][1], res['brute'][1]))
        out[key] = {'path_mean': round(res['path'][0], 5), 'path_se': round(res['path'][1], 5), 'brute_mean': round(res['brute'][0], 5),
                    'brute_se': round(res['brute'][1], 5), 'path_minus_brute': round(d, 5), 'relative': round(d / res['brute'][0], 4),
                    'standard_errors': round(abs(d) / se, 1) if se > 0 else None}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=32)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--scene', default='s978')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--bias', action='store_true')
    ap.add_argument('--blocks', type=int, default=16)
    ap.add_argument('--spp', type=int, default=256)
    args = ap.parse_args()
    rate(args)
    if args.bias:
        bias(args)


if __name__ == '__main__':
    main()

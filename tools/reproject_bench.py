#!/usr/bin/env python3
'''
What carrying the film over to a new view costs (FilmTable.keep_history / reproject, csrc/history_kernel.hip, history.hip; DESIGN.md
section 3.18), production build, on the 978-triangle headline scene and on a million random triangles (c5), at a --size x --size
film.  Per scene, by the library's HIP-event timers: keep_history() (the copy of the positions and the G-buffer kernel) and
reproject() (the motion kernel, the resample launch with its fold, the two cleared passes) after a camera yaw of +-2 degrees, and
for an unchanged view (every pixel static); one warm-up pair, then --repeat pairs: the median and the spread (least, largest).
Beside them the yardstick: the kernel time of a 1-spp PathEngine step on the same scene and film (mpt_kernel_time).

    python tools/reproject_bench.py [--scenes s978 c5] [--size 512] [--repeat 9] [--out FILE]
'''
import argparse
import json

import numpy as np

import benchlib
from benchlib import median


def spread(v):
    return {'median': round(median(v), 4), 'least': round(min(v), 4), 'largest': round(max(v), 4)}


def yawed(pers, degrees):
    '''the camera of `pers` turned about the world's y axis through its own centre of projection'''
    pers = np.asarray(pers, np.float64)
    rows = pers[[0, 1, 3]]
    eye = np.linalg.solve(rows[:, :3], -rows[:, 3])
    th = np.radians(degrees)
    R, T, Tinv = np.eye(4), np.eye(4), np.eye(4)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = np.cos(th), np.sin(th), -np.sin(th), np.cos(th)
    T[:3, 3], Tinv[:3, 3] = eye, -eye
    return pers @ T @ R @ Tinv


def bench(scene, args):
    from ptina_amd import scenes
    from ptina_amd.common import ctx
    from ptina_amd.things import Camera, ModelPool
    eng, film = benchlib.setup(args.size, scene)
    out = {'metric': 'reproject_ms', 'scene': scene, 'faces': ModelPool().nfaces, 'size': args.size, 'repeat': args.repeat,
           'fast_depth': ctx().get_option('fast_depth')}
    eng.render(8)
    ctx().call('mpt_synchronize')
    cams = [np.asarray(scenes.BENCH_CAMERA, np.float64), yawed(scenes.BENCH_CAMERA, 2.0)]
    for label, turn in (('yaw_2_degrees', True), ('unchanged_view', False)):
        keep, reproject, share = [], [], []
        film.history_kernel_time()
        for k in range(args.repeat + 1):
            film.keep_history()
            if turn:
                Camera().set_perspective(cams[(k + 1) % 2])
            res = film.reproject()
            keep_ms, reproject_ms, calls = film.history_kernel_time()
            assert calls == 2
            if k:                                            # (the first pair warms up: its buffers are made there)
                keep.append(keep_ms)
                reproject.append(reproject_ms)
                share.append(res.kept_fraction)
            eng.render(1)                                    # (new samples on top, as a viewport would add them)
        Camera().set_perspective(cams[0])
        out[label] = {'keep_ms': spread(keep), 'reproject_ms': spread(reproject), 'kept_fraction': round(median(share), 4)}
    film.clear()
    eng.render(1)
    ctx().call('mpt_synchronize')
    ctx().kernel_time()
    step = []
    for _ in range(args.repeat):
        eng.render(1)
        ctx().call('mpt_synchronize')
        step.append(ctx().kernel_time()[0])
    out['path_1spp_kernel_ms'] = spread(step)
    out['pair_over_1spp'] = round((out['yaw_2_degrees']['keep_ms']['median'] + out['yaw_2_degrees']['reproject_ms']['median']) / median(step), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', nargs='*', default=['s978', 'c5'])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--repeat', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    results = []
    for scene in args.scenes:
        results.append(bench(scene, args))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

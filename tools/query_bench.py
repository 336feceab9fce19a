#!/usr/bin/env python3
'''
Batch ray query throughput (BVHTree.intersect / occluded, csrc/query_kernel.hip), production build, on the
978-triangle headline scene, the 99 382-triangle c4 scene and a million random triangles (c5).  Two ray sets per scene: the primary
camera rays through the pixel centres of a --size x --size film in the order the one-lane-per-pixel kernels walk it (16x16 tiles,
an 8x8 sub-tile per wave: coherent), and the same rays shuffled (incoherent).  Per set: rays/s of mpt_query_closest and
mpt_query_occluded by the kernel timer (mpt_query_kernel_time) and by wall time, which includes the copies of 24 bytes of rays
in and up to 24 of answers out per ray; one warm-up call, then --repeat calls: the median and the spread (least, largest).

The yardstick of the coherent set is the preview kernel on the same scene and film: one camera ray per pixel through the same
tracer (plus its shading of the hit and three film elements per pixel).  Its launch has no event timer, so a frame's cost is
taken from wall time: (a call of 1 + K frames, one launch, waited for) - (a call of 1 frame), over K.

    python tools/query_bench.py [--scenes s978 c4 c5] [--size 512] [--repeat 7] [--preview-frames 16] [--out FILE]
'''
import argparse
import json
import time

import numpy as np

import benchlib
from benchlib import median


def camera_rays(size):
    '''the rays through the pixel centres, generated as BVHTree.pick does, in tile order -> (o [n][3], d [n][3])'''
    from ptina_amd.camera import Camera
    M = Camera().V2W
    t = np.arange(size // 16)
    tx, ty, wave, lane = np.meshgrid(t, t, np.arange(4), np.arange(64), indexing='ij')
    i = (tx * 16 + (wave >> 1) * 8 + (lane >> 3)).reshape(-1)
    j = (ty * 16 + (wave & 1) * 8 + (lane & 7)).reshape(-1)
    x = ((i + 0.5) / size * 2 - 1).astype(np.float32)
    y = ((j + 0.5) / size * 2 - 1).astype(np.float32)
    one = np.ones_like(x)
    a = np.stack([x, y, -one, one], axis=1) @ M.T
    b = np.stack([x, y, one, one], axis=1) @ M.T
    o = (a[:, :3] / a[:, 3:]).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray((b[:, :3] / b[:, 3:]).astype(np.float32) - o)


def spread(v):
    return {'median': round(median(v), 4), 'least': round(min(v), 4), 'largest': round(max(v), 4)}


def time_query(call, n, repeat):
    from ptina_amd.common import ctx
    call()
    ctx().timer('mpt_query_kernel_time')
    kernel, wall = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(ctx().timer('mpt_query_kernel_time')[0])
    return {'kernel_ms': spread(kernel), 'wall_ms': spread(wall), 'Mrays_per_s_kernel': round(n / median(kernel) / 1e3, 1),
            'Mrays_per_s_wall': round(n / median(wall) / 1e3, 1)}


def preview_frame_ms(preview, film, frames, repeat):
    from ptina_amd.common import ctx

    def call(k):
        t0 = time.perf_counter()
        preview.render(k)
        ctx().call('mpt_synchronize')
        return (time.perf_counter() - t0) * 1e3
    call(1 + frames)
    per = []
    for _ in range(repeat):
        short = call(1)
        per.append((call(1 + frames) - short) / frames)
    film.clear()
    return per


def bench(scene, args):
    from ptina_amd.common import ctx
    from ptina_amd.things import BVHTree, ModelPool
    _, preview, film = benchlib.setup(args.size, scene, preview=True)
    o, d = camera_rays(args.size)
    n = o.shape[0]
    tree = BVHTree()
    out = {'metric': 'query_rays_per_s', 'scene': scene, 'faces': ModelPool().nfaces, 'size': args.size, 'rays': n, 'repeat': args.repeat,
           'fast_depth': ctx().get_option('fast_depth')}
    hit = tree.intersect(o, d)['hit']
    out['hit_share'] = round(float(hit.mean()), 4)
    order = np.random.default_rng(1).permutation(n)
    for label, (ro, rd) in (('coherent', (o, d)), ('shuffled', (np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])))):
        out[label] = {'closest': time_query(lambda: tree.intersect(ro, rd), n, args.repeat),
                      'occluded': time_query(lambda: tree.occluded(ro, rd), n, args.repeat)}
    per = preview_frame_ms(preview, film, args.preview_frames, args.repeat)
    out['preview_frame_ms_wall'] = spread(per)
    out['preview_Mrays_per_s'] = round(n / median(per) / 1e3, 1)
    out['closest_over_preview'] = round(out['coherent']['closest']['kernel_ms']['median'] / median(per), 3)
    out['shuffled_over_coherent'] = {k: round(out['shuffled'][k]['kernel_ms']['median'] / out['coherent'][k]['kernel_ms']['median'], 3)
                                     for k in ('closest', 'occluded')}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', nargs='*', default=['s978', 'c4', 'c5'])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--preview-frames', type=int, default=16)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.size % 16 == 0
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

#!/usr/bin/env python3
'''
What a pose change costs (csrc/deform.hip) on compose_bench's two scenes -- 99 382 triangles (c4) and
1 000 000, each cut into 64 objects -- with every object's mesh carrying 16 morph targets, 4 of them with non-zero weights, and a
64-joint skin.  Per size one JSON line with
  the HIP-event time of the deform kernel alone, every object posed and one object of 64 posed, with the bytes it touches once per
  second (per corner: 32 read and 32 written of the record, 24 per target with a non-zero weight, 24 of the skin; the palette
  apart), and the rate of a device-to-device copy of as many bytes (mpt_stress_copies, wall time of --copies copies) as the yardstick;
  the median and the least wall time (ms, through to a device synchronise) of
  a  set_joints of one object + compose() + BVHTree().refit()
  b  the road without this feature: numpy skinning of that object on the host (tests/deform_ref.py), numpy composition of it,
     ModelPool().load of the whole model + refit()         (numpy on THIS host's CPU)
  c  the same + BVHTree().build() in place of the refit

    python tools/deform_bench.py [--sizes 99382 1000000] [--repeat 10] [--repeat-host 3] [--copies 50]
'''
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

from benchlib import median, wall_ms
from compose_bench import primitives

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import deform_ref                                                             # noqa: E402

TARGETS, NONZERO, JOINTS = 16, 4, 64


def bench(size, repeat, repeat_host, copies):
    from ptina_amd import _lib
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.multimesh import compose_multiple_meshes
    from ptina_amd.things import init_things, ModelPool, MaterialPool, BVHTree
    prims, mats = primitives(size)
    nobj = len(prims)
    reset_all()
    init_things()
    MaterialPool().load(mats)
    pool, tree, c = ModelPool(), BVHTree(), ctx()
    g = np.random.default_rng(2)
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731
    rigs = []
    for p, n, t, w, m in prims:
        k = p.shape[0]
        mesh = pool.add_mesh(p, n, t)
        dp = (0.01 * g.standard_normal((TARGETS, k, 3, 3), dtype=np.float32))
        jt = g.integers(0, JOINTS, size=(k, 3, 4))
        wt = g.uniform(0.05, 1.0, size=(k, 3, 4))
        wt = (wt / wt.sum(axis=2, keepdims=True)).astype(np.float32)
        pool.add_morph_targets(mesh, dp)
        pool.add_skin(mesh, jt, wt, JOINTS)
        pool.add_object(mesh, w, m)
        rigs.append((dp, jt, wt))

    def pose():
        w = np.zeros(TARGETS)
        w[g.choice(TARGETS, NONZERO, replace=False)] = g.uniform(0.2, 1.0, NONZERO)
        return w, deform_ref.random_joints(g, JOINTS, amount=0.05)
    palettes = [pose()[1] for _ in range(32)]                                  # (made outside the timed parts)
    turn = [0]

    def palette():
        turn[0] += 1
        return palettes[turn[0] % len(palettes)]
    for o in range(nobj):
        w, mats_ = pose()
        pool.set_morph_weights(o, w)
        pool.set_joints(o, mats_)
    pool.compose()
    tree.build()
    sync()
    out = {'metric': 'pose_change_ms', 'faces': size, 'objects': nobj, 'targets': TARGETS, 'nonzero_weights': NONZERO, 'joints': JOINTS,
           'chunk_corners': _lib.DEFORM_CHUNK, 'repeat': repeat, 'host': platform.processor() or platform.machine(), 'columns': ['wall median', 'wall min']}
    per_corner = 64 + 24 * NONZERO + 24
    kern = {}
    for name, objs in (('every object', range(nobj)), ('one object', [nobj // 2])):
        ms = []
        c.timer('mpt_deform_kernel_time')
        for _ in range(repeat + 2):
            for o in objs:
                pool.set_joints(o, palette())
            pool.compose()
            ms.append(c.timer('mpt_deform_kernel_time')[0])
        kern[name] = median(ms[2:])
        corners = pool.deform_stats().deformed_corners
        out['deform kernel, %s (ms, corners, GB/s)' % name] = [round(kern[name], 4), int(corners),
                                                                        round(corners * per_corner / (kern[name] * 1e-3) / 1e9, 1)]
    moved = 3 * size * per_corner
    mb = max(1, round(moved / 2 / 2 ** 20))
    rates = []
    for _ in range(5):
        c.call('mpt_stress_copies', mb, 2)
        c.call('mpt_stress_copies', mb, 0)
        t0 = time.perf_counter()
        c.call('mpt_stress_copies', mb, copies)
        c.call('mpt_stress_copies', mb, 0)
        rates.append(copies * 2 * (mb << 20) / (time.perf_counter() - t0) / 1e9)
    out['device-to-device copy of %d MiB (GB/s read + written, wall of %d copies)' % (mb, copies)] = round(median(rates), 1)
    out['deform / copy rate'] = round((moved / (kern['every object'] * 1e-3) / 1e9) / median(rates), 3)

    one = nobj // 2

    def device_road():
        pool.set_joints(one, palette())
        pool.compose()
        tree.refit()
        sync()
    tree.build()
    out['a set_joints + compose + refit'] = list(wall_ms(device_road, repeat))
    out['deformed objects, corners of a'] = [int(pool.deform_stats().deformed_objects), int(pool.deform_stats().deformed_corners)]

    # the road open without the feature: the host keeps the composed model, skins the one object in numpy and loads everything
    model_v, model_m = pool.to_numpy()
    first = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in prims])])
    p, n, t, world, mtl = prims[one]
    rec = deform_ref.records(p, n, t)
    dp, jt, wt = rigs[one]
    k3 = rec.shape[0]
    deltas = np.concatenate([dp.reshape(TARGETS, k3, 3), np.zeros((TARGETS, k3, 3), np.float32)], axis=2)
    w_one = pose()[0]

    def host_road(rebuild):
        def run():
            copy = deform_ref.deform(rec, deltas, w_one, jt.reshape(k3, 4), wt.reshape(k3, 4), palette())
            v, _ = compose_multiple_meshes([(*deform_ref.split(copy), world, mtl)])
            model_v[3 * first[one]:3 * first[one + 1]] = v
            pool.load(model_v, model_m)
            tree.build() if rebuild else tree.refit()
            sync()
        return run
    pool.load(model_v, model_m)
    tree.build()
    out['b numpy skinning + load + refit (host CPU: %s)' % out['host']] = list(wall_ms(host_road(False), repeat_host))
    out['c numpy skinning + load + build'] = list(wall_ms(host_road(True), repeat_host))
    print(json.dumps(out), flush=True)
    reset_all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[99382, 1000000])
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--repeat-host', type=int, default=3)
    ap.add_argument('--copies', type=int, default=50)
    args = ap.parse_args()
    for size in args.sizes:
        bench(size, args.repeat, args.repeat_host, args.copies)


if __name__ == '__main__':
    main()

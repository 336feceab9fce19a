#!/usr/bin/env python3
'''
What a scene edit costs (csrc/compose.hip) at 99 382 triangles (the c4 scene) and 1 000 000 (c5), each cut
into 64 objects of consecutive faces with a world matrix of their own.  Per size one JSON line with the median and the least wall
time (ms, the call through to a device synchronise) of
  a  the host path: ptina_amd.multimesh.compose_multiple_meshes + ModelPool().load + BVHTree().build()   (numpy on THIS host's CPU)
  b  ModelPool().load_meshes + BVHTree().build()
  c  ModelPool().set_world of one object + compose() + build()
the HIP-event time of the compose kernels alone -- everything written (after set_world of every object) and one object of 64 -- with
the bytes they move per second (32 read and 32 written per vertex, 4 written per face), and the rate of a device-to-device copy of
as many bytes (mpt_stress_copies, wall time of --copies copies) as the yardstick.

    python tools/compose_bench.py [--sizes 99382 1000000] [--repeat 10] [--repeat-host 3] [--copies 50]
'''
import argparse
import json
import platform
import time

import numpy as np

from benchlib import median, wall_ms


def primitives(size, nobj=64):
    from ptina_amd import scenes
    v, m, mats, _ = scenes.scene_c4() if size == 99382 else scenes.scene_random_tris(size)
    n = m.shape[0]
    assert n == size, (n, size)
    g = np.random.default_rng(size)
    cut = [n * o // nobj for o in range(nobj + 1)]
    prims = []
    for o in range(nobj):
        r = v[3 * cut[o]:3 * cut[o + 1]].reshape(-1, 3, 8)
        prims.append((r[..., 0:3].copy(), r[..., 3:6].copy(), r[..., 6:8].copy(), world(g), int(m[cut[o]])))
    return prims, mats


def world(g):
    th = g.uniform(-0.2, 0.2)
    w = np.array([[np.cos(th), 0, np.sin(th), 0], [0, 1, 0, 0], [-np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1.0]])
    w[:3, 3] = g.uniform(-0.05, 0.05, 3)
    return w


def bench(size, repeat, repeat_host, copies):
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.multimesh import compose_multiple_meshes
    from ptina_amd.things import init_things, ModelPool, MaterialPool, BVHTree
    prims, mats = primitives(size)
    reset_all()
    init_things()
    MaterialPool().load(mats)
    pool, tree, c = ModelPool(), BVHTree(), ctx()
    g = np.random.default_rng(1)
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731
    out = {'metric': 'scene_edit_ms', 'faces': size, 'objects': len(prims), 'repeat': repeat, 'host': platform.processor() or platform.machine(),
           'columns': ['wall median', 'wall min']}

    def host_path():
        v, m = compose_multiple_meshes(prims)
        pool.load(v, m)
        tree.build()
        sync()
    out['a compose_multiple_meshes + load + build (host CPU: %s)' % out['host']] = list(wall_ms(host_path, repeat_host))

    def device_path():
        pool.load_meshes(prims)
        tree.build()
        sync()
    out['b load_meshes + build'] = list(wall_ms(device_path, repeat))

    def edit():
        pool.set_world(int(g.integers(len(prims))), world(g))
        pool.compose()
        tree.build()
        sync()
    out['c set_world + compose + build'] = list(wall_ms(edit, repeat))
    assert pool.compose_stats().host_fetches == 0 or size <= 8192
    out['build alone'] = list(wall_ms(lambda: (tree.build(), sync()), repeat))
    out['sah_fallback'] = c.get_option('sah_fallback')

    moved = 3 * size * 64 + 4 * size                                           # bytes a composition of everything reads and writes
    kern = {}
    for name, objs in (('all', range(len(prims))), ('one', [len(prims) // 2])):
        ms = []
        c.timer('mpt_compose_kernel_time')
        for _ in range(repeat + 2):
            for o in objs:
                pool.set_world(o, world(g))
            pool.compose()
            ms.append(c.timer('mpt_compose_kernel_time')[0])
        kern[name] = median(ms[2:])
        faces = pool.compose_stats().recomposed
        out['compose kernels, %s objects (ms, faces, GB/s)' % name] = [round(kern[name], 4), int(faces),
                                                                         round((3 * faces * 64 + 4 * faces) / (kern[name] * 1e-3) / 1e9, 1)]
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
    out['compose / copy rate'] = round((moved / (kern['all'] * 1e-3) / 1e9) / median(rates), 3)
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

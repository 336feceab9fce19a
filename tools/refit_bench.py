#!/usr/bin/env python3
'''
What a refit costs against the build it replaces (csrc/refit.hip, csrc/tree_refit.cpp), on s34, s978, the
99 382 triangles of c4 and 1 000 000 random ones, each cut into objects of consecutive faces (8 for the two small scenes, 64
above: tools/compose_bench.py's scene).  Per size one JSON line with the median and the least wall time (ms, the call through
to a device synchronise; --repeat calls after two warm-ups) of
  a  ModelPool().set_world of one object + compose() + BVHTree().build()
  b  the same with BVHTree().refit()
  build alone and refit alone (the refit of an unchanged model: the same kernels over the same bytes)
the HIP-event time of the refit's kernels, the bytes of the records a refit rewrites and reads (per face: 96 of vertices, 128
of tgeo / tshade, 48 of tfast, 32 of snode, 64 of fnode, 24 of bmin / bmax; per wide node 128 + 64) per second of that kernel
time, and the rate of a device-to-device copy of as many bytes (mpt_stress_copies) as the yardstick.

--turntable STEPS (at --turntable-size faces, default 99 382): one object of 64 is turned about the y axis through a full turn
in STEPS steps and refitted at every step with no build in between; per step the growth, refit + render and -- the same frame
on a freshly built tree -- build + render, at 512 x 512 x 8 spp (wall ms).  The last line names the growth at which
refit + render first costs more than build + render: BVHTree().update()'s default max_growth is that, rounded down to one
decimal (inf if the two never cross).

    python tools/refit_bench.py [--sizes 34 978 99382 1000000] [--repeat 10] [--copies 50] [--turntable 36]
'''
import argparse
import json
import time

import numpy as np

from benchlib import median, wall_ms
from compose_bench import world


def primitives(size):
    from ptina_amd import scenes
    small = {34: scenes.scene_s34, 978: scenes.scene_s978}
    v, m, mats, imgs = small[size]() if size in small else scenes.scene_c4() if size == 99382 else scenes.scene_random_tris(size)
    n = m.shape[0]
    assert n == size, (n, size)
    nobj = 8 if size in small else 64
    g = np.random.default_rng(size)
    cut = [n * o // nobj for o in range(nobj + 1)]
    prims = []
    for o in range(nobj):
        r = np.asarray(v, np.float32)[3 * cut[o]:3 * cut[o + 1]].reshape(-1, 3, 8)
        prims.append((r[..., 0:3].copy(), r[..., 3:6].copy(), r[..., 6:8].copy(), world(g), int(m[cut[o]])))
    return prims, mats, imgs


def start(size, film=None):
    from ptina_amd import scenes
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import init_things, ModelPool, MaterialPool, ImagePool, BVHTree, FilmTable, Camera
    from ptina_amd.engine.path import PathEngine
    prims, mats, imgs = primitives(size)
    reset_all()
    init_things()
    eng = PathEngine()
    MaterialPool().load(mats)
    ImagePool().load(imgs)
    if film:
        FilmTable().set_size(film, film)
        Camera().set_perspective(scenes.BENCH_CAMERA)
    ModelPool().load_meshes(prims)
    BVHTree().build()
    return prims, eng, ModelPool(), BVHTree(), ctx()


def bench(size, repeat, copies):
    from ptina_amd.common import reset_all
    prims, _, pool, tree, c = start(size)
    g = np.random.default_rng(1)
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731
    out = {'metric': 'refit_ms', 'faces': size, 'objects': len(prims), 'repeat': repeat, 'columns': ['wall median', 'wall min']}

    def edit(then):
        pool.set_world(int(g.integers(len(prims))), world(g))
        pool.compose()
        then()
        sync()
    out['a set_world + compose + build'] = list(wall_ms(lambda: edit(tree.build), repeat))
    growth = []
    out['b set_world + compose + refit'] = list(wall_ms(lambda: edit(lambda: growth.append(tree.refit())), repeat))
    out['growth after %d refits' % len(growth)] = round(growth[-1], 4)
    out['build alone'] = list(wall_ms(lambda: (tree.build(), sync()), repeat))
    tree.refit()
    c.timer('mpt_refit_kernel_time')
    out['refit alone'] = list(wall_ms(lambda: (tree.refit(), sync()), repeat))
    ms, calls = c.timer('mpt_refit_kernel_time')
    kern = ms / max(calls, 1)
    info = tree.refit_stats()
    moved = size * (96 + 128 + 48 + 32 + 64 + 24) + int(info.wide_nodes) * (128 + 64)
    out['refit kernels (ms per call, bytes, GB/s)'] = [round(kern, 4), moved, round(moved / (kern * 1e-3) / 1e9, 1)]
    out['build / refit, edit sequence'] = round(out['a set_world + compose + build'][0] / out['b set_world + compose + refit'][0], 2)
    out['build / refit, alone'] = round(out['build alone'][0] / out['refit alone'][0], 2)
    out['host_fetches by refits'] = int(info.host_fetches)
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
    print(json.dumps(out), flush=True)
    reset_all()


def turntable(size, steps, film=512, spp=8):
    from ptina_amd.common import reset_all
    from ptina_amd.things import FilmTable
    prims, eng, pool, tree, c = start(size, film)
    obj = len(prims) // 2
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731

    def timed(call):
        sync()
        t0 = time.perf_counter()
        call()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def render():
        FilmTable().clear()
        eng.render(spp)
        c.call('mpt_flush')

    def placed(k):
        th = 2 * np.pi * k / steps
        return np.array([[np.cos(th), 0, np.sin(th), 0], [0, 1, 0, 0], [-np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1.0]]) @ prims[obj][3]
    render()
    sync()
    rows = []
    # pass 1: refits only, no build in between; pass 2: the same frames on freshly built trees
    pool.set_world(obj, placed(0)), pool.compose(), tree.build()
    for k in range(1, steps + 1):
        pool.set_world(obj, placed(k))
        pool.compose()
        growth = []
        t_refit = timed(lambda: growth.append(tree.refit()))
        t_render = median([timed(render) for _ in range(3)])
        rows.append({'step': k, 'growth': round(growth[0], 4), 'refit_ms': round(t_refit, 4), 'render_refitted_ms': round(t_render, 4)})
    for k in range(1, steps + 1):
        pool.set_world(obj, placed(k))
        pool.compose()
        rows[k - 1]['build_ms'] = round(timed(tree.build), 4)
        rows[k - 1]['render_built_ms'] = round(median([timed(render) for _ in range(3)]), 4)
    cross = None
    for r in rows:
        print(json.dumps(dict(r, metric='refit_turntable', faces=size, film=film, spp=spp)), flush=True)
        if cross is None and r['refit_ms'] + r['render_refitted_ms'] > r['build_ms'] + r['render_built_ms']:
            cross = r
    default = 'inf' if cross is None else np.floor(cross['growth'] * 10) / 10
    print(json.dumps({'metric': 'refit_default_max_growth', 'faces': size, 'steps': steps, 'first step where refit + render > build + render': cross,
                      'largest growth of the turn': max(r['growth'] for r in rows), 'default max_growth': default}), flush=True)
    reset_all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[34, 978, 99382, 1000000])
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--copies', type=int, default=50)
    ap.add_argument('--turntable', type=int, default=0)
    ap.add_argument('--turntable-size', type=int, default=99382)
    args = ap.parse_args()
    for size in args.sizes:
        bench(size, args.repeat, args.copies)
    if args.turntable:
        turntable(args.turntable_size, args.turntable)


if __name__ == '__main__':
    main()

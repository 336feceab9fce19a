#!/usr/bin/env python3
'''
What a strength change of a displaced subdivided mesh costs (csrc/displace.hip).  subdiv_bench's two scenes:
64 objects, each a bumpy open grid of quads split in two -- 7 x 7 quads (98 faces) and 22 x 22 (968 faces) -- at level 2, 100 352 and
991 232 triangles, every mesh (rigid here: one copy each) displaced along its normals by one 256 x 256 image.  Per size one JSON line
with
  the HIP-event times of the displacement launch beside the normal kernel's (which does the same ring walk) and the records', every
  mesh's strength changed and one mesh's of 64 (median of --repeat composes);
  the median and the least wall time (ms, through to a device synchronise) of
  a  set_displacement of one mesh + compose() + BVHTree().update()
  b  the road without this feature: the numpy restatement (tests/displace_ref.py, with the topology made beforehand) of that mesh on
     the host, numpy composition of it, ModelPool().load of the whole model + build()            (numpy on THIS host's CPU)
  the host time of mpt_mesh_set_displacement (the first-corner table and the uv check of one mesh) per mesh.
The lines are also written to --out as a JSON list.

    python tools/displace_bench.py [--quads 7 22] [--levels 2] [--image 256] [--repeat 10] [--repeat-host 2] [--out FILE]
'''
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

from benchlib import median, wall_ms
from compose_bench import world

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import deform_ref                                                             # noqa: E402
import displace_ref                                                           # noqa: E402
import subdiv_ref                                                             # noqa: E402

NOBJ = 64


def bench(quads, levels, image_size, repeat, repeat_host):
    from ptina_amd import _lib
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.multimesh import compose_multiple_meshes
    from ptina_amd.things import init_things, ModelPool, BVHTree, ImagePool
    reset_all()
    init_things()
    pool, tree, c = ModelPool(), BVHTree(), ctx()
    g = np.random.default_rng(quads)
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731
    image = displace_ref.random_image(quads, image_size, image_size)
    ImagePool().load([image])
    rec = subdiv_ref.mesh_records(*subdiv_ref.grid(quads, quads))
    k = rec.shape[0] // 3
    worlds, set_ms = [], []
    for o in range(NOBJ):
        mesh = pool.add_mesh(*deform_ref.split(rec))
        pool.add_subdivision(mesh, levels)
        t0 = time.perf_counter()
        pool.add_displacement(mesh, 0, strength=0.05, midlevel=0.5, mode='normal', channel='mean')
        set_ms.append((time.perf_counter() - t0) * 1e3)
        worlds.append(world(g))
        pool.add_object(mesh, worlds[-1], -1)
    strengths = [0.02 + 0.002 * i for i in range(32)]
    turn = [0]

    def strength():
        turn[0] += 1
        return strengths[turn[0] % len(strengths)]
    pool.compose()
    tree.build()
    sync()
    size = pool.nfaces
    out = {'metric': 'displaced_strength_change_ms', 'cage_faces': k * NOBJ, 'faces': size, 'objects': NOBJ, 'levels': levels,
           'image': [image_size, image_size], 'chunk_items': _lib.SUBDIV_CHUNK, 'repeat': repeat, 'host': platform.processor() or platform.machine(),
           'columns': ['wall median', 'wall min']}
    out['mpt_mesh_set_displacement of one mesh of %d faces (host ms: median, least)' % k] = [round(median(set_ms), 3), round(min(set_ms), 3)]
    for name, meshes in (('every mesh', range(NOBJ)), ('one mesh', [NOBJ // 2])):
        ms = []
        c.timer('mpt_subdiv_kernel_time', 3)
        c.timer('mpt_displace_kernel_time')
        for _ in range(repeat + 2):
            for m in meshes:
                pool.set_displacement(m, strength())
            pool.compose()
            ms.append(c.timer('mpt_subdiv_kernel_time', 3) + c.timer('mpt_displace_kernel_time'))
        ms = ms[2:]
        seg = [median([m[s] for m in ms]) for s in (4, 1, 2, 0)]
        d = pool.displace_stats()
        out['kernels, %s (ms: displacement, normals, records, refine levels; vertices displaced; launches per compose: subdivision, displacement)' % name] = [
            round(seg[0], 4), round(seg[1], 4), round(seg[2], 4), round(seg[3], 4), int(d.displaced_verts), int(ms[0][3]), int(ms[0][5])]

    one = NOBJ // 2

    def device_road():
        pool.set_displacement(one, strength())
        pool.compose()
        kind = tree.update(max_growth=float('inf'))
        sync()
        return kind
    tree.build()
    assert device_road() == 'refit'
    out['a set_displacement + compose + update'] = list(wall_ms(device_road, repeat))
    out['displaced copies, vertices of a'] = [int(pool.displace_stats().displaced_copies), int(pool.displace_stats().displaced_verts)]

    # the road open without the feature: subdivide and displace the one mesh in numpy, compose it, load everything, build
    model_v, model_m = pool.to_numpy()
    per = size // NOBJ
    topo = subdiv_ref.topology(rec, levels)

    def host_road():
        fine = displace_ref.displace(rec, levels, image, displace_ref.NORMAL, displace_ref.MEAN, strength(), 0.5, topo=topo)
        v, _ = compose_multiple_meshes([(*deform_ref.split(fine), worlds[one], -1)])
        model_v[3 * per * one:3 * per * (one + 1)] = v
        pool.load(model_v, model_m)
        tree.build()
        sync()
    out['b numpy subdivision + displacement + load + build (host CPU: %s)' % out['host']] = list(wall_ms(host_road, repeat_host))
    print(json.dumps(out), flush=True)
    reset_all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quads', type=int, nargs='*', default=[7, 22])
    ap.add_argument('--levels', type=int, default=2)
    ap.add_argument('--image', type=int, default=256)
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--repeat-host', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = [bench(quads, args.levels, args.image, args.repeat, args.repeat_host) for quads in args.quads]
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(lines, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

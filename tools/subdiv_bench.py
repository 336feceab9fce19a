#!/usr/bin/env python3
'''
What a pose change of a subdivided character costs (csrc/subdiv.hip).  The cages are 64 skinned objects, each
a bumpy open grid of quads split in two -- 7 x 7 quads (98 faces) and 22 x 22 (968 faces) -- so that at level 2 the model has
100 352 and 991 232 triangles, the sizes of compose_bench's two scenes (99 382 and 1 000 000; those scenes themselves cannot be
cages: cut into 64 runs of faces they are not manifold).  Every mesh carries a 64-joint skin.  Per size one JSON line with
  the HIP-event times of the refine launches, the normals and the records, every object posed and one object of 64 posed;
  the rate of the record kernel (96 bytes written per refined face) against a device-to-device copy that writes as many bytes
  (mpt_stress_copies, wall time of --copies copies): the figure of merit;
  the median and the least wall time (ms, through to a device synchronise) of
  a  set_joints of one object + compose() + BVHTree().update()
  b  the road without this feature: numpy skinning (tests/deform_ref.py) and numpy subdivision (tests/subdiv_ref.py, with the
     topology made beforehand) of that object on the host, numpy composition of it, ModelPool().load of the whole model +
     build()                                                (numpy on THIS host's CPU)
  the host time of mpt_mesh_set_subdivision (the topology of one cage, on the host) per mesh.
With --creases every size is measured twice, a JSON line each: with every grid line (the quads' edges, not
their diagonals) at sharpness inf, and with none (the uncreased call); the lines also name the records of the last level against
its vertices, and road b subdivides by tests/subdiv_crease_ref.py.
With --scheme catmull-clark the same grids are cages of quads -- each quad the fan of two triangles it
already is -- so that the face counts are those of above; road b subdivides by tests/subdiv_cc_ref.py.

    python tools/subdiv_bench.py [--quads 7 22] [--levels 2] [--repeat 10] [--repeat-host 2] [--copies 50] [--creases] [--scheme catmull-clark]
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
import subdiv_ref                                                             # noqa: E402
import subdiv_crease_ref                                                      # noqa: E402
import subdiv_cc_ref                                                          # noqa: E402

JOINTS, NOBJ = 64, 64


def grid_lines(quads):
    '''[k,3] f32: inf on every edge of subdiv_ref.grid(quads, quads) that is a grid line -- its ends differ by 1 or by quads + 1'''
    faces = np.array(subdiv_ref.grid(quads, quads)[1])
    step = np.abs(faces - np.roll(faces, -1, axis=1))
    return np.where((step == 1) | (step == quads + 1), np.float32(np.inf), np.float32(0)).astype(np.float32)


def bench(quads, levels, repeat, repeat_host, copies, creases=None, scheme='loop'):
    from ptina_amd import _lib
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.multimesh import compose_multiple_meshes
    from ptina_amd.things import init_things, ModelPool, BVHTree
    reset_all()
    init_things()
    pool, tree, c = ModelPool(), BVHTree(), ctx()
    g = np.random.default_rng(quads)
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731
    rec = subdiv_ref.mesh_records(*subdiv_ref.grid(quads, quads))
    k = rec.shape[0] // 3
    lines = grid_lines(quads) if creases == 'lines' else None
    cc = scheme == 'catmull-clark'
    polys = np.full(quads * quads, 4, np.int32) if cc else None
    if cc and lines is not None:                                               # per quad (a, b, c, d): all four edges are grid lines
        lines = np.full(4 * quads * quads, np.inf, np.float32)
    rigs, worlds, set_ms = [], [], []
    for o in range(NOBJ):
        mesh = pool.add_mesh(*deform_ref.split(rec))
        jt = g.integers(0, JOINTS, size=(k, 3, 4))
        wt = g.uniform(0.05, 1.0, size=(k, 3, 4))
        wt = (wt / wt.sum(axis=2, keepdims=True)).astype(np.float32)
        pool.add_skin(mesh, jt, wt, JOINTS)
        t0 = time.perf_counter()
        if cc:
            pool.add_subdivision(mesh, levels, creases=lines, scheme=scheme, polys=polys)
        elif lines is None:
            pool.add_subdivision(mesh, levels)
        else:
            pool.add_subdivision(mesh, levels, creases=lines)
        set_ms.append((time.perf_counter() - t0) * 1e3)
        worlds.append(world(g))
        pool.add_object(mesh, worlds[-1], -1)
        rigs.append((jt, wt))
    palettes = [deform_ref.random_joints(g, JOINTS, amount=0.05) for _ in range(32)]   # (made outside the timed parts)
    turn = [0]

    def palette():
        turn[0] += 1
        return palettes[turn[0] % len(palettes)]
    for o in range(NOBJ):
        pool.set_joints(o, palette())
    pool.compose()
    tree.build()
    sync()
    size = pool.nfaces
    out = {'metric': 'subdivided_pose_change_ms', 'cage_faces': k * NOBJ, 'faces': size, 'objects': NOBJ, 'levels': levels, 'joints': JOINTS,
           'scheme': scheme, 'chunk_items': _lib.SUBDIV_CHUNK, 'repeat': repeat, 'host': platform.processor() or platform.machine(), 'columns': ['wall median', 'wall min']}
    if creases is not None:
        _, _, tables = _lib.subdiv_topology_cc(rec, levels, polys, lines) if cc else _lib.subdiv_topology_creased(rec, levels, lines)
        out['creases'] = 'every grid line inf' if creases == 'lines' else 'none'
        out['records, vertices of the last level (one cage)'] = [len(tables['records']), int(tables['counts'][levels, 0])]
    out['mpt_mesh_set_subdivision of one cage of %d faces (host ms: median, least)' % k] = [round(median(set_ms), 3), round(min(set_ms), 3)]
    emit = {}
    for name, objs in (('every object', range(NOBJ)), ('one object', [NOBJ // 2])):
        ms = []
        c.timer('mpt_subdiv_kernel_time', 3)
        for _ in range(repeat + 2):
            for o in objs:
                pool.set_joints(o, palette())
            pool.compose()
            ms.append(c.timer('mpt_subdiv_kernel_time', 3))
        ms = ms[2:]
        seg = [median([m[s] for m in ms]) for s in range(3)]
        emit[name] = seg[2]
        faces = pool.subdiv_stats().refined_faces
        out['subdivision kernels, %s (ms: refine levels, normals, records; faces; launches per compose)' % name] = [
            round(seg[0], 4), round(seg[1], 4), round(seg[2], 4), int(faces), int(ms[0][3])]
    written = 96 * size
    mb = max(1, round(written / 2 ** 20))
    rates = []
    for _ in range(5):
        c.call('mpt_stress_copies', mb, 2)
        c.call('mpt_stress_copies', mb, 0)
        t0 = time.perf_counter()
        c.call('mpt_stress_copies', mb, copies)
        c.call('mpt_stress_copies', mb, 0)
        rates.append(copies * (mb << 20) / (time.perf_counter() - t0) / 1e9)
    out['device-to-device copy of %d MiB (GB/s written, wall of %d copies)' % (mb, copies)] = round(median(rates), 1)
    out['record kernel (GB/s written)'] = round(written / (emit['every object'] * 1e-3) / 1e9, 1)
    out['record kernel / copy rate'] = round((written / (emit['every object'] * 1e-3) / 1e9) / median(rates), 3)

    one = NOBJ // 2

    def device_road():
        pool.set_joints(one, palette())
        pool.compose()
        kind = tree.update(max_growth=float('inf'))
        sync()
        return kind
    tree.build()
    assert device_road() == 'refit'
    out['a set_joints + compose + update'] = list(wall_ms(device_road, repeat))
    out['refined copies, faces of a'] = [int(pool.subdiv_stats().refined_copies), int(pool.subdiv_stats().refined_faces)]

    # the road open without the feature: skin, subdivide and compose the one object in numpy, load everything, build
    model_v, model_m = pool.to_numpy()
    per = size // NOBJ
    jt, wt = rigs[one]
    if cc:
        topo = subdiv_cc_ref.topology(rec, levels, polys, lines)
    else:
        topo = subdiv_ref.topology(rec, levels) if creases is None else subdiv_crease_ref.topology(rec, levels, lines)

    def host_road():
        copy = deform_ref.deform(rec, None, None, jt.reshape(k * 3, 4), wt.reshape(k * 3, 4), palette())
        if cc:
            fine = subdiv_cc_ref.subdivide(rec, levels, topo=topo, control=copy)
        elif creases is None:
            fine = subdiv_ref.subdivide(rec, levels, topo, control=copy)
        else:
            fine = subdiv_crease_ref.subdivide(rec, levels, topo=topo, control=copy)
        v, _ = compose_multiple_meshes([(*deform_ref.split(fine), worlds[one], -1)])
        model_v[3 * per * one:3 * per * (one + 1)] = v
        pool.load(model_v, model_m)
        tree.build()
        sync()
    if repeat_host > 0:
        out['b numpy skinning + numpy subdivision + load + build (host CPU: %s)' % out['host']] = list(wall_ms(host_road, repeat_host))
    print(json.dumps(out), flush=True)
    reset_all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quads', type=int, nargs='*', default=[7, 22])
    ap.add_argument('--levels', type=int, default=2)
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--repeat-host', type=int, default=2)
    ap.add_argument('--copies', type=int, default=50)
    ap.add_argument('--creases', action='store_true', help='measure every size with every grid line at sharpness inf, and with none')
    ap.add_argument('--scheme', default='loop', choices=('loop', 'catmull-clark'))
    args = ap.parse_args()
    for quads in args.quads:
        for creases in (('lines', 'none') if args.creases else (None,)):
            bench(quads, args.levels, args.repeat, args.repeat_host, args.copies, creases, args.scheme)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
'''
What a scatter costs, and what it saves (csrc/scatter.hip).  Two scenes:
  terrain  20 000 instances of a 64-face tuft on a displaced terrain of 131 072 faces (a cage of 8 x 8 quads at level 5, displaced
           along its normals by a 256 x 256 image); the edit is a change of the displacement's strength
  floor    2 000 instances of the tuft on the floor (2 faces) of the 978-triangle scene; the edit moves the floor
Per scene one JSON line with the median and the least wall time (ms, through mpt_compose's closing synchronise) of
  a  the first compose() with the scatter: weights + scan + selection + placement + the composition of everything
  b  the edit of the surface + compose(): placement + the composition of the surface and the instances
  c  the same edit on the interface without scatters: the instances are hand-added objects; the edit + compose(), the surface
     fetched with subdivided_to_numpy (terrain), the placement of tests/scatter_ref.py in numpy, set_world per instance, compose()
                                                                                                  (numpy on THIS host's CPU)
and beside them the HIP-event times of the scatter's launches (selection = weights, scan and records; placement) and of the
composition kernel in a and b.  The lines are also written to --out as a JSON list.

--min-distance R (or `auto`: the distance at which about half of the candidates are rejected, found by bisection through the test
door mpt_scatter_space_points) adds, per scene, a line for the SPACED scatter of the same count from M = 4 x count candidates
(csrc/scatter_space.hip) behind the plain scatter's line, which stands beside it as what spacing costs over:
  a  the first compose(): selection, elimination (grid, rounds, compaction: the rounds one scatter took and those launched, the
     host's waits) and placement by their HIP events, the elimination's being part of the selection's
  b  the edit + compose(): no elimination launch (asserted), to be compared with the plain scatter's b
  c  the host comparator: the M candidates' records and the surface fetched, their positions and the greedy elimination of
     tests/scatter_space_ref.py in numpy on this host's CPU, the placement in numpy and `count` set_world calls, compose()

    python tools/scatter_bench.py [--scenes terrain floor] [--repeat 10] [--repeat-host 3] [--min-distance R|auto] [--out FILE]
'''
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

from benchlib import median, wall_ms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import deform_ref                                                             # noqa: E402
import displace_ref                                                           # noqa: E402
import scatter_ref                                                            # noqa: E402
import scatter_space_ref                                                      # noqa: E402
import subdiv_ref                                                             # noqa: E402

SCALE = (0.01, 0.03)


def shift(x, y, z):
    m = np.eye(4)
    m[:3, 3] = [x, y, z]
    return m


def flat_cage(quads=8, side=4.0):
    '''[3k,8] f32 records of a flat grid of quads in the plane y = 0, each split in two, texcoords over the unit square'''
    x = np.linspace(-side / 2, side / 2, quads + 1)
    rec = []
    for j in range(quads):
        for i in range(quads):
            q = [(i, j), (i, j + 1), (i + 1, j + 1), (i + 1, j)]
            for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
                rec += [(x[a], 0.0, x[b], 0, 1, 0, a / quads, b / quads) for a, b in tri]
    return np.ascontiguousarray(rec, np.float32)


def fresh():
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import init_things, ModelPool
    reset_all()
    init_things()
    return ModelPool(), ctx()


def scene(pool, name):
    '''the surface and the rest of scene `name` in the pool: (surface object, its world, the edit as a function of a turn, the
    surface's mesh records or None where the device makes them)'''
    from ptina_amd import scenes
    from ptina_amd.things import ImagePool
    if name == 'terrain':
        ImagePool().load([displace_ref.random_image(1, 256, 256)])
        mesh = pool.add_mesh(*deform_ref.split(flat_cage()))
        pool.add_subdivision(mesh, 5)
        pool.add_displacement(mesh, 0, strength=0.1, midlevel=0.5, mode='normal', channel='mean')
        world = shift(0, 0.5, 0)
        surf = pool.add_object(mesh, world, 0)
        return surf, (lambda turn: world), (lambda turn: pool.set_displacement(mesh, 0.05 + 0.01 * (turn % 8))), None
    v, m, _, _ = scenes.scene_s978()
    floor = pool.add_object(pool.add_mesh(*deform_ref.split(v[:6])), np.eye(4), 0)
    for mtl in sorted(set(m[2:].tolist())):
        pick = np.repeat(m == mtl, 3)
        pick[:6] = False
        pool.add_object(pool.add_mesh(*deform_ref.split(v[pick])), np.eye(4), mtl)
    world = lambda turn: shift(0, 0.01 * (turn % 8), 0)                        # noqa: E731
    return floor, world, (lambda turn: pool.set_world(floor, world(turn))), v[:6]


def candidates_of(name, m):
    '''the positions [m,3] of the m candidates of the scene's scatter, as the host can get at them: a plain scatter of m small
    instances, its records and the surface fetched, the placement's point in numpy.  Also (pool, scatter, surface records, world)'''
    pool, c = fresh()
    surf, world, edit, rec = scene(pool, name)
    sid, _ = pool.add_scatter(surf, pool.add_mesh(*deform_ref.split(subdiv_ref.fixture('tetrahedron'))), m, seed=1, mtlid=1, scale=SCALE)
    pool.compose()

    def fetch():
        surface = pool.subdivided_to_numpy(surf) if rec is None else rec
        corners = scatter_ref.world_corners(surface, world(0))
        points = pool.scatter_to_numpy(sid)[0]
        return scatter_space_ref.positions(corners, points), corners, points
    return pool, c, fetch


def half_distance(name, m):
    '''the distance at which about half of the m candidates are rejected: bisection through the test door'''
    from ptina_amd import _lib
    pool, c, fetch = candidates_of(name, m)
    pos = fetch()[0]
    lo, hi = 0.0, float(np.ptp(pos, axis=0).max())
    for _ in range(24):
        r = 0.5 * (lo + hi)
        rejected = 1.0 - _lib.scatter_space_points(c, pos, r)[0].mean()
        if abs(rejected - 0.5) < 0.01:
            break
        lo, hi = (r, hi) if rejected < 0.5 else (lo, r)
    return r, rejected


def host_comparator(name, count, m, r, repeat_host):
    '''c of a spaced scatter: wall ms (median, min) of the elimination and placement on the host'''
    pool, c, fetch = candidates_of(name, m)
    tuft = subdiv_ref.fixture_subdivided('tetrahedron', 2)
    mesh = pool.add_mesh(*deform_ref.split(tuft))
    hand = [pool.add_object(mesh, np.eye(4), 1) for _ in range(count)]
    pool.compose()
    kept_total = []

    def road():
        pos, corners, points = fetch()
        kept = scatter_space_ref.greedy_of_points(pos, r)
        kept_total.append(int(kept.sum()))
        chosen = points[np.flatnonzero(kept)[:count]]
        for obj, w in zip(hand, scatter_ref.place(corners, chosen)):
            pool.set_world(obj, w)
        pool.compose()
    ms = []
    for _ in range(repeat_host):                                           # (seconds a call on the terrain: no warm-up calls)
        t0 = time.perf_counter()
        road()
        ms.append((time.perf_counter() - t0) * 1e3)
    return [round(median(ms), 4), round(min(ms), 4)], kept_total[-1]


def bench(name, count, repeat, repeat_host, spacing=None):
    tuft = subdiv_ref.fixture_subdivided('tetrahedron', 2)                     # 64 faces
    spaced = {} if spacing is None else dict(min_distance=spacing[0], candidates=spacing[1])
    out = {'metric': 'scatter_ms' if spacing is None else 'spaced_scatter_ms', 'scene': name, 'instances': count, 'tuft_faces': tuft.shape[0] // 3, 'repeat': repeat,
           'host': platform.processor() or platform.machine(), 'columns': ['wall median', 'wall min']}
    # ---- a: the first compose with the scatter (a fresh context each time: the pool, the arenas and the model are allocated in it)
    first, kernels = [], []
    for _ in range(3):
        pool, c = fresh()
        surf, world, edit, rec = scene(pool, name)
        pool.compose()
        sid, objs = pool.add_scatter(surf, pool.add_mesh(*deform_ref.split(tuft)), count, seed=1, mtlid=1, scale=SCALE, **spaced)
        c.timer('mpt_scatter_kernel_time', 2)
        c.timer('mpt_compose_kernel_time')
        c.timer('mpt_scatter_spacing_kernel_time')
        t0 = time.perf_counter()
        pool.compose()
        first.append((time.perf_counter() - t0) * 1e3)
        kernels.append(c.timer('mpt_scatter_kernel_time', 2)[:2] + c.timer('mpt_compose_kernel_time')[:1] + c.timer('mpt_scatter_spacing_kernel_time')[:1])
    out['faces'] = pool.nfaces
    out['surface_faces'] = pool._object_faces(pool._obj_mesh[surf])
    out['a first compose with the scatter'] = [round(median(first), 4), round(min(first), 4)]
    out['a kernels (ms: selection, placement, composition)'] = [round(median([k[s] for k in kernels]), 4) for s in range(3)]
    if spacing is not None:
        sp, st = pool.scatter_spacing_stats(), pool.scatter_stats()
        out['min_distance'], out['candidates'], out['kept'] = spacing[0], spacing[1], sp.kept
        out['a elimination (ms by HIP events, inside the selection: grid, rounds, waits, compaction)'] = round(median([k[3] for k in kernels]), 4)
        out['a elimination: rounds taken, round kernels launched, grid kernels, compaction kernels, host waits'] = [
            sp.rounds, sp.round_launches, sp.grid_launches, sp.compact_launches, sp.host_reads]
        out['a host_fetches of the scatter step'] = st.host_fetches
    # ---- b: the edit + compose, in the last context
    turn = [0]

    def device_road():
        turn[0] += 1
        edit(turn[0])
        pool.compose()
    device_road()
    c.timer('mpt_scatter_kernel_time', 2)
    c.timer('mpt_compose_kernel_time')
    ms, ks = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        device_road()
        ms.append((time.perf_counter() - t0) * 1e3)
        ks.append(c.timer('mpt_scatter_kernel_time', 2)[:2] + c.timer('mpt_compose_kernel_time')[:1])
    s, cs = pool.scatter_stats(), pool.compose_stats()
    assert (s.select_launches, s.place_launches, s.placed_instances) == (0, 1, count) and cs.dirty_objects == count + 1
    sp = pool.scatter_spacing_stats()
    assert (sp.scatters, sp.grid_launches, sp.round_launches, sp.compact_launches, sp.host_reads) == (0, 0, 0, 0, 0)   # no elimination in b
    out['b edit + compose'] = [round(median(ms), 4), round(min(ms), 4)]
    out['b kernels (ms: selection, placement, composition)'] = [round(median([k[s] for k in ks]), 4) for s in range(3)]
    points, worlds, _ = pool.scatter_to_numpy(sid)
    if spacing is not None:
        key = 'c records and surface fetched + numpy positions, greedy elimination and placement + set_world per instance + compose (host CPU: %s)' % out['host']
        out[key], kept = host_comparator(name, count, spacing[1], spacing[0], repeat_host)
        assert kept == out['kept'], (kept, out['kept'])                    # the host's pass keeps what the device kept
        print(json.dumps(out), flush=True)
        from ptina_amd.common import reset_all
        reset_all()
        return out
    # ---- c: the same on the interface without scatters
    pool, c = fresh()
    surf, world, edit, rec = scene(pool, name)
    mesh = pool.add_mesh(*deform_ref.split(tuft))
    hand = [pool.add_object(mesh, w, 1) for w in worlds]
    pool.compose()

    def host_road():
        turn[0] += 1
        edit(turn[0])
        if rec is None:
            pool.compose()
            surface = pool.subdivided_to_numpy(surf)
        else:
            surface = rec
        placed = scatter_ref.place(scatter_ref.world_corners(surface, world(turn[0])), points)
        for obj, w in zip(hand, placed):
            pool.set_world(obj, w)
        pool.compose()
    out['c edit + fetch + numpy placement + set_world per instance + compose (host CPU: %s)' % out['host']] = list(wall_ms(host_road, repeat_host))
    print(json.dumps(out), flush=True)
    from ptina_amd.common import reset_all
    reset_all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', nargs='*', default=['terrain', 'floor'])
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--repeat-host', type=int, default=3)
    ap.add_argument('--min-distance', default=None, help="a distance, or 'auto': the one that rejects about half of 4 x count candidates")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []
    for name in args.scenes:
        count = 20000 if name == 'terrain' else 2000
        lines.append(bench(name, count, args.repeat, args.repeat_host))
        if args.min_distance is None:
            continue
        if args.min_distance == 'auto':
            r, rejected = half_distance(name, 4 * count)
            print('%s: %.1f %% of %d candidates are rejected at the distance %.6g' % (name, 100 * rejected, 4 * count, r), flush=True)
        else:
            r = float(args.min_distance)
        lines.append(bench(name, count, args.repeat, args.repeat_host, (r, 4 * count)))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(lines, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
'''
What parent bindings cost (csrc/hierarchy.hip).  One JSON object, printed and written to
profiles/rNN_hierarchy_bench.json (NN: the last profile + 1), with the median and the least of --repeat runs of
  a  crowd with props: tools/anim_bench.py's crowd -- 1024 objects of one skinned tube of 384 faces and 64 joints bound to one clip --
     with a rigid prop of 8 faces on the top joint of every character (set_parent with a joint): set_time + compose() with and
     without the props (wall ms, through to a device synchronise), and the hierarchy kernel alone (HIP events);
  b  rigid tree: 1024 rigid objects of 8 faces, 4 levels deep (4, 16, 64 and 940 children) under one root moved by set_world:
     set_world(root) + compose() on the device road, against the host road of the same run -- numpy products down the tree, 1024
     set_world, compose() (numpy on THIS host's CPU) -- and their ratio.

    python tools/hierarchy_bench.py [--objects 1024] [--repeat 10] [--out FILE]
'''
import argparse
import glob
import json
import os
import platform
import re

import numpy as np

from benchlib import ROOT, median, wall_ms
from anim_bench import JOINTS, tube, rig


def drum():
    '''(p, n [8,3,3]): a small four-sided double pyramid'''
    top, bottom = np.array([0.0, 0.15, 0.0]), np.array([0.0, -0.15, 0.0])
    ring = [np.array([0.1 * np.cos(a), 0.0, 0.1 * np.sin(a)]) for a in np.arange(4) * np.pi / 2]
    tris = []
    for k in range(4):
        a, b = ring[k], ring[(k + 1) % 4]
        tris += [[a, top, b], [b, bottom, a]]
    p = np.array(tris)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return p, np.repeat(n[:, None, :], 3, axis=1)


def _roads(c, road, repeat, timer):
    out = {}
    c.timer(timer)
    out['wall ms'] = list(wall_ms(road, repeat))
    ms = []
    for _ in range(repeat):
        road()
        ms.append(c.timer(timer)[0])
    out['%s alone (ms, HIP events)' % timer[4:-5].replace('_', ' ')] = [round(median(ms), 4), round(min(ms), 4)]
    return out


def bench_crowd(nobj, repeat):
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import init_things, ModelPool
    from ptina_amd.tools.skin import attach
    reset_all()
    init_things()
    pool, c = ModelPool(), ctx()
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731
    p, n, jt, wt = tube()
    parents, t, r, s, ib, tracks = rig()
    dp, dn = drum()
    offsets = 4.0 * np.arange(nobj) / nobj
    local = np.eye(4)
    local[1, 3] = 0.2

    def scene(props):
        pool.clear_meshes()
        mesh = pool.add_mesh(p, n)
        pool.add_skin(mesh, jt, wt, JOINTS)
        pool.add_skeleton(mesh, parents, t, r, s, ib)
        clip = pool.add_clip(mesh, tracks)
        prop = pool.add_mesh(dp, dn)
        side = int(np.ceil(np.sqrt(nobj)))
        objs = []
        for o in range(nobj):
            w = np.eye(4)
            w[:3, 3] = [o % side, 0.0, o // side]
            objs.append(pool.add_object(mesh, w, 0))
            pool.set_animation(objs[-1], clip, offsets[o])
        held = [pool.add_object(prop, attach(ib[JOINTS - 1], local), 1) for _ in range(nobj)]     # (without props: the same faces, standing still)
        if props:
            for o in range(nobj):
                pool.set_parent(held[o], objs[o], JOINTS - 1)
        pool.compose()
        sync()
    out = {'metric': 'crowd_with_props_frame_ms', 'objects': nobj, 'faces_per_object': int(p.shape[0]), 'faces_per_prop': int(dp.shape[0]), 'joints': JOINTS,
           'repeat': repeat, 'columns': ['median', 'min']}
    clock = [0.0]

    def road():
        clock[0] += 0.0417
        pool.set_time(clock[0])
        pool.compose()
        sync()
    scene(False)
    out['without props: set_time + compose'] = _roads(c, road, repeat, 'mpt_anim_kernel_time')
    assert pool.hierarchy_stats().evaluated == 0
    scene(True)
    clock[0] = 0.0
    out['with props: set_time + compose'] = _roads(c, road, repeat, 'mpt_hierarchy_kernel_time')
    st = pool.hierarchy_stats()
    assert (st.evaluated, st.launches) == (nobj, 1 if nobj <= 1024 else st.levels)
    reset_all()
    return out


def bench_tree(nobj, repeat):
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import init_things, ModelPool
    reset_all()
    init_things()
    pool, c = ModelPool(), ctx()
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731
    dp, dn = drum()
    g = np.random.default_rng(8)
    # parents: the root is -1; 4 children of the root, 16 of those, 64 of those, the rest under the third level
    first = [0, 4, 20, 84]
    parent = np.empty(nobj, np.int64)
    for i in range(nobj):
        level = sum(i >= f for f in first) - 1
        parent[i] = -1 if level == 0 else (first[level - 1] + (i - first[level]) % (first[level] - first[level - 1]))
    locals_ = np.tile(np.eye(4), (nobj, 1, 1))
    locals_[:, :3, 3] = g.uniform(-1.0, 1.0, (nobj, 3))
    depth = np.zeros(nobj, np.int64)
    for i in range(nobj):
        depth[i] = 1 if parent[i] < 0 else depth[parent[i]] + 1
    assert depth.max() == 4

    def scene(bound):
        pool.clear_meshes()
        mesh = pool.add_mesh(dp, dn)
        root = pool.add_object(mesh, np.eye(4), 0)
        objs = [pool.add_object(mesh, locals_[i], 1) for i in range(nobj)]
        if bound:
            for i in range(nobj):
                pool.set_parent(objs[i], root if parent[i] < 0 else objs[parent[i]])
        pool.compose()
        sync()
        return root, objs
    out = {'metric': 'rigid_tree_frame_ms', 'objects': nobj, 'levels': 4, 'faces_per_object': int(dp.shape[0]), 'repeat': repeat,
           'host': platform.processor() or platform.machine(), 'columns': ['median', 'min']}
    clock = [0.0]

    def moved():
        clock[0] += 0.0417
        m = np.eye(4)
        m[:3, 3] = [np.sin(clock[0]), 0.0, np.cos(clock[0])]
        return m
    root, objs = scene(True)

    def device_road():
        pool.set_world(root, moved())
        pool.compose()
        sync()
    dev = _roads(c, device_road, repeat, 'mpt_hierarchy_kernel_time')
    out['a device road: set_world(root) + compose'] = dev
    st = pool.hierarchy_stats()
    assert (st.evaluated, st.levels) == (nobj, 4)
    out['launches per frame'] = int(st.launches)
    root, objs = scene(False)

    def host_road():
        w0 = moved()
        world = np.empty((nobj, 4, 4))
        for i in range(nobj):                                                  # (parents come before their children)
            world[i] = (w0 if parent[i] < 0 else world[parent[i]]) @ locals_[i]
        pool.set_world(root, w0)
        for i, obj in enumerate(objs):
            pool.set_world(obj, world[i])
        pool.compose()
        sync()
    host = list(wall_ms(host_road, repeat))
    out['b host road: numpy products + %d set_world + compose (wall ms; host CPU: %s)' % (nobj, out['host'])] = host
    out['ratio host / device (medians)'] = round(host[0] / dev['wall ms'][0], 2)
    reset_all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=1024)
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--out', default=None, help='the file to write (default: profiles/rNN_hierarchy_bench.json, NN the last profile + 1)')
    args = ap.parse_args()
    path = args.out
    if path is None:
        last = max([int(m.group(1)) for f in glob.glob(os.path.join(ROOT, 'profiles', 'r*')) for m in [re.match(r'r(\d+)_', os.path.basename(f))] if m] or [0])
        path = os.path.join(ROOT, 'profiles', 'r%02d_hierarchy_bench.json' % (last + 1))
    out = {'crowd': bench_crowd(args.objects, args.repeat), 'tree': bench_tree(args.objects, args.repeat)}
    print(json.dumps(out), flush=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
'''
What a frame of a crowd costs (csrc/anim.hip): 1024 objects of one skinned tube of 384 faces and 64 joints
(a chain), bound to one clip -- a LINEAR rotation track of 33 keys on every joint and a LINEAR translation track on the root -- at
offsets spread over the clip.  One JSON object, printed and written to profiles/rNN_anim_bench.json (NN: the last profile + 1), with
the median and the least of --repeat runs of
  a  set_time + compose()                                      wall ms, through to a device synchronise
  b  the road that exists without the feature: the tracks sampled for all objects at once in numpy (the rule of csrc/anim_rule.h,
     vectorised over the objects), tools.skin.joint_matrices per object, 1024 set_joints + compose()      (numpy on THIS host's CPU)
  the anim kernel alone (HIP events), the deform kernel of the same frames, and compose() with nothing changed.

    python tools/anim_bench.py [--objects 1024] [--repeat 10] [--out FILE]

--blend and --motion (written to profiles/rNN_anim_blend_bench.json) measure instead
  --blend   the same crowd with a second clip of 65 tracks on every object and cross-fades whose starts are spread over the crowd:
            set_time + compose and the anim kernel alone, against (a) the single-clip frame of the same run and (b) the host road: both
            clips sampled in numpy, the blend, joint_matrices, 1024 set_joints on unbound objects + compose()
  --motion  1024 rigid objects of the tube on object clips (T and R tracks of 33 keys): set_time + compose and the motion kernel alone,
            against the host road: numpy sampling, 1024 set_world + compose()
'''
import argparse
import glob
import json
import os
import platform
import re

import numpy as np

from benchlib import ROOT, median, wall_ms

JOINTS, RINGS, SIDES, KEYS, HEIGHT, RADIUS = 64, 12, 16, 33, 2.4, 0.2


def tube():
    '''(p, n [k,3,3], joints, weights [k,3,4]): rings of quads round the y axis, each corner bound to the two joints its height lies between'''
    y, a = np.linspace(0.0, HEIGHT, RINGS + 1), np.linspace(0.0, 2 * np.pi, SIDES + 1)
    yy, aa = np.meshgrid(y, a, indexing='ij')
    nrm = np.stack([np.cos(aa), np.zeros_like(aa), np.sin(aa)], axis=-1)
    pos = RADIUS * nrm + np.stack([np.zeros_like(yy), yy, np.zeros_like(yy)], axis=-1)
    at = np.clip(yy / HEIGHT * JOINTS - 0.5, 0.0, JOINTS - 1.0)
    j0 = np.floor(at).astype(np.int64)
    f = at - j0
    jt = np.stack([j0, np.minimum(j0 + 1, JOINTS - 1), np.zeros_like(j0), np.zeros_like(j0)], axis=-1)
    wt = np.stack([1.0 - f, f, np.zeros_like(f), np.zeros_like(f)], axis=-1)

    def tris(x):
        c = x[:-1, :-1], x[1:, :-1], x[1:, 1:], x[:-1, 1:]
        return np.concatenate([np.stack([c[0], c[1], c[2]], axis=-2).reshape(-1, 3, x.shape[-1]),
                               np.stack([c[0], c[2], c[3]], axis=-2).reshape(-1, 3, x.shape[-1])])
    return tris(pos), tris(nrm), tris(jt), tris(wt)


def rig():
    '''(parents, rest t r s, inverse_bind [nj,4,4], tracks): the chain up the tube and a clip that sways it'''
    from ptina_amd.tools.anim import quaternion, rest_pose, track
    g = np.random.default_rng(4)
    seg = HEIGHT / JOINTS
    t, r, s = rest_pose(JOINTS)
    t[1:, 1] = seg
    ib = np.tile(np.eye(4), (JOINTS, 1, 1))
    ib[:, 1, 3] = -seg * np.arange(JOINTS)
    times = np.linspace(0.0, 4.0, KEYS)
    sway = 1.5 * np.sin(2 * np.pi * times / 4.0) / JOINTS
    tracks = [track(j, 'R', times, [quaternion([g.normal(scale=0.1), 0, 1], a * g.uniform(0.5, 1.5)) for a in sway]) for j in range(JOINTS)]
    tracks.append(track(0, 'T', times, np.stack([0.1 * np.sin(times), 0.05 * np.abs(np.sin(3 * times)), 0.0 * times], axis=1)))
    return np.arange(JOINTS) - 1, t, r, s, ib, tracks


def host_trs(t, r, s, tracks, tau):
    '''(T [n,nj,3], R [n,nj,4], S [n,nj,3]) at the local times tau [n]: the tracks by the rule, vectorised over the objects'''
    n = tau.size
    T, R, S = (np.tile(x, (n, 1, 1)) for x in (t, r, s))
    for tr in tracks:                                                          # (LINEAR tracks: all this clip has)
        times, v = tr.times.astype(np.float64), tr.values.astype(np.float64)
        k = np.clip(np.searchsorted(times, tau, side='right') - 1, 0, times.size - 2)
        u = np.clip((tau - times[k]) / (times[k + 1] - times[k]), 0.0, 1.0)[:, None]
        a, b = v[k], v[k + 1]
        if tr.path == 1:
            d = (a * b).sum(axis=1, keepdims=True)
            b, d = np.where(d < 0, -b, b), np.abs(d)
            theta = np.arccos(np.minimum(d, 1.0))
            with np.errstate(invalid='ignore', divide='ignore'):
                q = np.where(d > 0.9995, a + u * (b - a), (np.sin((1 - u) * theta) * a + np.sin(u * theta) * b) / np.sin(theta))
            R[:, tr.target] = q / np.where(d > 0.9995, np.linalg.norm(q, axis=1, keepdims=True), 1.0)
        else:
            (T if tr.path == 0 else S)[:, tr.target] = a + u * (b - a)
    return T, R, S


def host_poses(parents, t, r, s, ib, tracks, tau):
    '''[n,nj,4,4] palettes at the local times tau [n]: host_trs, then joint_matrices per object'''
    from ptina_amd.tools.anim import local_matrices
    from ptina_amd.tools.skin import joint_matrices
    T, R, S = host_trs(t, r, s, tracks, tau)
    return np.stack([joint_matrices(parents, local_matrices(T[o], R[o], S[o]), ib) for o in range(tau.size)])


def host_blend(A, B, w):
    '''the blend of two sampled (T, R, S) by the weights w [n]: lerp, and for R the normalised lerp over the shorter arc'''
    w = w[:, None, None]
    d = (A[1] * B[1]).sum(axis=2, keepdims=True)
    q = A[1] + w * (np.where(d < 0, -B[1], B[1]) - A[1])
    return A[0] + w * (B[0] - A[0]), q / np.linalg.norm(q, axis=2, keepdims=True), A[2] + w * (B[2] - A[2])


def bench(nobj, repeat):
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import init_things, ModelPool
    reset_all()
    init_things()
    pool, c = ModelPool(), ctx()
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731
    p, n, jt, wt = tube()
    parents, t, r, s, ib, tracks = rig()

    def scene(bind):
        pool.clear_meshes()
        mesh = pool.add_mesh(p, n)
        pool.add_skin(mesh, jt, wt, JOINTS)
        pool.add_skeleton(mesh, parents, t, r, s, ib)
        clip = pool.add_clip(mesh, tracks)
        side = int(np.ceil(np.sqrt(nobj)))
        objs = []
        for o in range(nobj):
            w = np.eye(4)
            w[:3, 3] = [o % side, 0.0, o // side]
            objs.append(pool.add_object(mesh, w, 0))
            if bind:
                pool.set_animation(objs[-1], clip, offsets[o])
        pool.compose()
        sync()
        return objs
    offsets = 4.0 * np.arange(nobj) / nobj
    out = {'metric': 'crowd_frame_ms', 'objects': nobj, 'faces_per_object': int(p.shape[0]), 'joints': JOINTS, 'tracks': len(tracks), 'keys_per_track': KEYS,
           'repeat': repeat, 'host': platform.processor() or platform.machine(), 'columns': ['median', 'min']}
    clock = [0.0]

    def tick():
        clock[0] += 0.0417
        return clock[0]
    # a: the device road
    scene(True)

    def device_road():
        pool.set_time(tick())
        pool.compose()
        sync()
    c.timer('mpt_anim_kernel_time')
    c.timer('mpt_deform_kernel_time')
    out['a set_time + compose (wall ms)'] = list(wall_ms(device_road, repeat))
    assert pool.anim_stats().evaluated_objects == nobj
    anim, deform = [], []
    for _ in range(repeat):
        device_road()
        anim.append(c.timer('mpt_anim_kernel_time')[0])
        deform.append(c.timer('mpt_deform_kernel_time')[0])
    out['anim kernel alone (ms, HIP events)'] = [round(median(anim), 4), round(min(anim), 4)]
    out['deform kernel of the same frames (ms, HIP events)'] = [round(median(deform), 4), round(min(deform), 4)]

    def idle():
        pool.compose()
        sync()
    out['compose with nothing changed (wall ms)'] = list(wall_ms(idle, repeat))
    assert pool.anim_stats().evaluated_objects == 0
    # b: the host road
    objs = scene(False)
    parts = {'sampling + joint_matrices': [], 'set_joints': [], 'compose': []}
    import time

    def host_road():
        now = tick()
        t0 = time.perf_counter()
        pal = host_poses(parents, t, r, s, ib, tracks, np.mod(now - offsets, 4.0))
        t1 = time.perf_counter()
        for o, obj in enumerate(objs):
            pool.set_joints(obj, pal[o])
        t2 = time.perf_counter()
        pool.compose()
        sync()
        t3 = time.perf_counter()
        for key, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
            parts[key].append(dt * 1e3)
    out['b numpy sampling + joint_matrices + %d set_joints + compose (wall ms; host CPU: %s)' % (nobj, out['host'])] = list(wall_ms(host_road, repeat))
    for key, ms in parts.items():
        out['b, of which %s' % key] = [round(median(ms[2:]), 4), round(min(ms[2:]), 4)]
    host_pose = pool.pose_to_numpy(nobj // 3)[1]
    now = clock[0]
    pool2 = scene(True)
    pool.set_time(now)
    pool.compose()
    device_pose = pool.pose_to_numpy(pool2[nobj // 3])[1]
    out['largest |device palette - host palette| of one object at one time'] = float(np.abs(device_pose - host_pose).max())
    reset_all()
    return out


def _roads(c, device_road, repeat, timer):
    '''the rows the new modes share: the device road's wall time and its kernel's time'''
    out = {}
    c.timer(timer)
    out['set_time + compose (wall ms)'] = list(wall_ms(device_road, repeat))
    ms = []
    for _ in range(repeat):
        device_road()
        ms.append(c.timer(timer)[0])
    out['%s alone (ms, HIP events)' % timer[4:-5].replace('_', ' ')] = [round(median(ms), 4), round(min(ms), 4)]
    return out


def bench_blend(nobj, repeat):
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import init_things, ModelPool
    from ptina_amd.tools.anim import local_matrices, quaternion, track
    from ptina_amd.tools.skin import joint_matrices
    reset_all()
    init_things()
    pool, c = ModelPool(), ctx()
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731
    p, n, jt, wt = tube()
    parents, t, r, s, ib, walk = rig()
    g = np.random.default_rng(5)
    times = np.linspace(0.0, 2.0, KEYS)                                        # the second clip: half the span, twice the sway
    sway = 3.0 * np.sin(2 * np.pi * times / 2.0) / JOINTS
    run = [track(j, 'R', times, [quaternion([0, g.normal(scale=0.1), 1], a * g.uniform(0.5, 1.5)) for a in sway]) for j in range(JOINTS)]
    run.append(track(0, 'T', times, np.stack([0.2 * np.sin(2 * times), 0.1 * np.abs(np.sin(6 * times)), 0.0 * times], axis=1)))
    offsets, starts = 4.0 * np.arange(nobj) / nobj, 2.0 * np.arange(nobj) / nobj

    def scene(bind):
        pool.clear_meshes()
        mesh = pool.add_mesh(p, n)
        pool.add_skin(mesh, jt, wt, JOINTS)
        pool.add_skeleton(mesh, parents, t, r, s, ib)
        ca, cb = pool.add_clip(mesh, walk), pool.add_clip(mesh, run)
        side = int(np.ceil(np.sqrt(nobj)))
        objs = []
        for o in range(nobj):
            w = np.eye(4)
            w[:3, 3] = [o % side, 0.0, o // side]
            objs.append(pool.add_object(mesh, w, 0))
            if bind:
                pool.set_animation(objs[-1], ca, offsets[o])
            if bind == 2:
                pool.set_animation_blend(objs[-1], cb, 0.5 * offsets[o], weight=(0.0, 1.0), fade=(starts[o], 1.5))
        pool.compose()
        sync()
        return objs
    out = {'metric': 'crowd_blend_frame_ms', 'objects': nobj, 'faces_per_object': int(p.shape[0]), 'joints': JOINTS, 'tracks_per_clip': [len(walk), len(run)],
           'keys_per_track': KEYS, 'repeat': repeat, 'host': platform.processor() or platform.machine(), 'columns': ['median', 'min']}
    clock = [0.0]

    def tick():
        clock[0] += 0.0417
        return clock[0]

    def device_road():
        pool.set_time(tick())
        pool.compose()
        sync()
    scene(1)
    out['a single clip'] = _roads(c, device_road, repeat, 'mpt_anim_kernel_time')
    scene(2)
    clock[0] = 0.0
    out['two clips blended'] = _roads(c, device_road, repeat, 'mpt_anim_kernel_time')
    st = pool.anim_blend_stats()
    assert st.evaluated_blended == nobj and pool.anim_stats().evaluated_objects == nobj
    objs = scene(0)

    def host_road():
        now = tick()
        A = host_trs(t, r, s, walk, np.mod(now - offsets, 4.0))
        B = host_trs(t, r, s, run, np.mod(now - 0.5 * offsets, 2.0))
        T, R, S = host_blend(A, B, np.clip((now - starts) / 1.5, 0.0, 1.0))
        for o, obj in enumerate(objs):
            pool.set_joints(obj, joint_matrices(parents, local_matrices(T[o], R[o], S[o]), ib))
        pool.compose()
        sync()
    out['b numpy sampling of both clips + blend + joint_matrices + %d set_joints + compose (wall ms; host CPU: %s)' % (nobj, out['host'])] = list(wall_ms(host_road, repeat))
    reset_all()
    return out


def bench_motion(nobj, repeat):
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import init_things, ModelPool
    from ptina_amd.tools.anim import local_matrices, quaternion, track
    reset_all()
    init_things()
    pool, c = ModelPool(), ctx()
    sync = lambda: c.call('mpt_synchronize')                                   # noqa: E731
    p, n, _, _ = tube()
    g = np.random.default_rng(6)
    times = np.linspace(0.0, 4.0, KEYS)
    nclips = 8
    clips = [[track(0, 'T', times, np.stack([0.3 * np.sin(times + k), 0.1 * np.abs(np.sin(3 * times)), 0.3 * np.cos(times + k)], axis=1)),
              track(0, 'R', times, [quaternion([g.normal(scale=0.1), 1, 0], 0.4 * a) for a in times])] for k in range(nclips)]
    offsets = 4.0 * np.arange(nobj) / nobj
    side = int(np.ceil(np.sqrt(nobj)))
    bases = np.tile(np.eye(4), (nobj, 1, 1))
    bases[:, 0, 3], bases[:, 2, 3] = np.arange(nobj) % side, np.arange(nobj) // side

    def scene(bind):
        pool.clear_meshes()
        mesh = pool.add_mesh(p, n)
        ids = [pool.add_object_clip(tr) for tr in clips]
        objs = [pool.add_object(mesh, bases[o], 0) for o in range(nobj)]
        if bind:
            for o in range(nobj):
                pool.set_motion(objs[o], ids[o % nclips], offsets[o], base=bases[o])
        pool.compose()
        sync()
        return objs
    out = {'metric': 'moved_objects_frame_ms', 'objects': nobj, 'faces_per_object': int(p.shape[0]), 'object_clips': nclips, 'tracks_per_clip': 2, 'keys_per_track': KEYS,
           'repeat': repeat, 'host': platform.processor() or platform.machine(), 'columns': ['median', 'min']}
    clock = [0.0]

    def tick():
        clock[0] += 0.0417
        return clock[0]

    def device_road():
        pool.set_time(tick())
        pool.compose()
        sync()
    scene(True)
    out.update(_roads(c, device_road, repeat, 'mpt_motion_kernel_time'))
    assert pool.anim_blend_stats().evaluated_moved == nobj
    objs = scene(False)
    rest = (np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 1.0]]), np.ones((1, 3)))

    def host_road():
        now = tick()
        tau = np.mod(now - offsets, 4.0)
        world = np.empty((nobj, 4, 4))
        for k in range(nclips):
            T, R, S = host_trs(*rest, clips[k], tau[k::nclips])
            world[k::nclips] = bases[k::nclips] @ local_matrices(T[:, 0], R[:, 0], S[:, 0])
        for o, obj in enumerate(objs):
            pool.set_world(obj, world[o])
        pool.compose()
        sync()
    out['b numpy sampling + %d set_world + compose (wall ms; host CPU: %s)' % (nobj, out['host'])] = list(wall_ms(host_road, repeat))
    reset_all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=1024)
    ap.add_argument('--repeat', type=int, default=10)
    ap.add_argument('--out', default=None, help='the file to write (default: profiles/rNN_anim_bench.json, NN the last profile + 1; with --blend or --motion '
                    'rNN_anim_blend_bench.json)')
    ap.add_argument('--blend', action='store_true', help='two clips blended on every object of the crowd')
    ap.add_argument('--motion', action='store_true', help='rigid objects moved by object clips')
    args = ap.parse_args()
    path = args.out
    new = args.blend or args.motion
    if path is None:
        last = max([int(m.group(1)) for f in glob.glob(os.path.join(ROOT, 'profiles', 'r*')) for m in [re.match(r'r(\d+)_', os.path.basename(f))] if m] or [0])
        path = os.path.join(ROOT, 'profiles', 'r%02d_anim_%sbench.json' % (last + 1, 'blend_' if new else ''))
    if new:
        out = {}
        if args.blend:
            out['blend'] = bench_blend(args.objects, args.repeat)
        if args.motion:
            out['motion'] = bench_motion(args.objects, args.repeat)
    else:
        out = bench(args.objects, args.repeat)
    print(json.dumps(out), flush=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()

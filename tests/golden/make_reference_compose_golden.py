#!/usr/bin/env python3
'''The fixture of the device composition (ModelPool.load_meshes, csrc/compose.hip): the reference's own compose_multiple_meshes
(ptina/multimesh.py imports without Taichi) run on meshes whose sizes put the objects' boundaries inside waves and workgroups.

Run in the build container only (needs the reference tree; nothing here is needed at test time):
    python3 tests/golden/make_reference_compose_golden.py
writes tests/golden/reference_compose.npz -- the f32 inputs, the f64 world matrices, the material ids and the reference's f64
outputs, data only.  Every output value is asserted to lie more than compose_ref.MARGIN error bounds away from an f32 rounding
boundary (tests/compose_ref.py), so that its f32 bits do not depend on the order of an f64 evaluation; a seed that fails is skipped.'''
import contextlib
import io
import os
import sys

import numpy as np

REF = os.environ.get('PTINA_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path = [p for p in sys.path if os.path.abspath(p or '.') != os.path.dirname(os.path.dirname(HERE))]
sys.path.append(os.path.dirname(HERE))

from ptina import multimesh as M       # noqa: E402
import ptina                           # noqa: E402
assert os.path.abspath(ptina.__file__).startswith(os.path.abspath(REF)), ptina.__file__
import compose_ref                     # noqa: E402

MESH_FACES = (1, 21, 22, 85, 0, 86, 300)         # 63 / 66 vertices around a wave, 255 / 258 around a 256-lane workgroup; one empty
OBJ_MESH = (0, 1, 2, 3, 4, 1, 5, 3, 6)           # eight objects with faces, two pairs sharing a mesh, the empty one in mid-list: 621 faces
OBJ_MTL = (0, 2, None, 5, 1, 3, None, 63, 4)


def rotation(g):
    q = g.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def draw(seed):
    g = np.random.default_rng(seed)
    meshes = []
    for k in MESH_FACES:
        p = g.uniform(-1, 1, (k, 3, 3)).astype(np.float32)
        n = g.normal(size=(k, 3, 3))
        n = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
        t = g.uniform(0, 1, (k, 3, 2)).astype(np.float32)
        meshes.append((p, n, t))
    worlds = []
    for o in range(len(OBJ_MESH)):
        w = np.eye(4)
        w[:3, :3] = rotation(g) @ np.diag(g.uniform(0.4, 2.5, 3))
        w[:3, 3] = g.uniform(-3, 3, 3)
        worlds.append(w)
    worlds[3][3] = [0, 0, 0, 2]                       # a bottom row that is not (0, 0, 0, 1): the divide is real
    worlds[6][3] = [0.01, -0.02, 0.03, 1]             # mildly projective
    prims = [(*meshes[m], worlds[o], OBJ_MTL[o]) for o, m in enumerate(OBJ_MESH)]
    with contextlib.redirect_stdout(io.StringIO()):
        verts, mtlids = M.compose_multiple_meshes(prims)
    return meshes, worlds, prims, np.asarray(verts, np.float64), np.asarray(mtlids)


seed = 20261019
while True:
    meshes, worlds, prims, verts, mtlids = draw(seed)
    worst, closest, count = compose_ref.margin(prims, verts)
    print('seed %d: %d values, smallest distance to an f32 rounding boundary %.3g error bounds (%.3g f32 ulp)' % (seed, count, worst, closest))
    if worst > compose_ref.MARGIN and np.isfinite(verts).all():
        break
    seed += 1

out = {'seed': np.int64(seed), 'nmeshes': np.int64(len(meshes)), 'obj_mesh': np.array(OBJ_MESH, np.int64),
       'obj_world': np.array(worlds, np.float64), 'obj_mtl': np.array([-1 if m is None else m for m in OBJ_MTL], np.int64),
       'obj_mtl_none': np.array([m is None for m in OBJ_MTL]), 'out_verts': verts, 'out_mtlids': mtlids.astype(np.int64)}
for i, (p, n, t) in enumerate(meshes):
    out['mesh%d_p' % i], out['mesh%d_n' % i], out['mesh%d_t' % i] = p, n, t
assert verts.shape == (621 * 3, 8) and mtlids.shape == (621,)
path = os.path.join(HERE, 'reference_compose.npz')
np.savez_compressed(path, **out)
print('wrote', path, os.path.getsize(path), 'bytes')

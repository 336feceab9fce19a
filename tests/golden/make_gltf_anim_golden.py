#!/usr/bin/env python3
'''
Writes the fixture of the animated-glTF loader ("animated glTF into ModelPool"):

    tests/golden/animated_scene.gltf            a hand-made glTF 2.0 scene, its one buffer base64 inside the file (a few KB)
    tests/golden/animated_scene_expected.npz    what it must evaluate to at four times, and the arrays the reader must find in it

    python tests/golden/make_gltf_anim_golden.py

The scene: node 0 `base` (T LINEAR, R CUBICSPLINE) > node 1 `arm` (R LINEAR, S STEP) > node 2 `lamp`, a rigid triangle: a rigid node
under an animated node under an animated node; node 8 `pair` under `base`, a mesh of two primitives; node 3 `strip`, a skinned strip
of four triangles with one morph target (its own transform is there to be ignored) over skin 0 = joints 5 > 6 under node 4 `rig`
(joint 5: T STEP, joint 6: R LINEAR; a LINEAR `weights` track on the strip); node 7 `prop`, a rigid triangle under joint 6.

The expected values are evaluated HERE, by a walk of the node tree written from the glTF 2.0 specification (sections "Transformations",
"Skins", "Morph Targets", "Animations" and its appendix C, interpolation) in plain Python floats, one operation at a time; it shares
no code with ptina_amd or with the tests' *_ref.py files.  Where the specification leaves the order of a sum or the association of a
product open, this file takes the order the library documents in include/miptina.h (sums left to right, a child on a joint as
world(skinned) . (jointMatrix . (bind . local))), so that the comparison can be bit for bit.  Every transform is generic -- no zero
entries but a matrix's bottom row -- and the inverse bind matrices are translations by dyadic numbers, whose inverses are exact.  The
LINEAR rotation tracks keep neighbouring keys within 1.8 degrees of arc (the library's lerp branch): the other branch calls acos and
sin, which no two libraries round alike, and is held elsewhere (tests/test_hierarchy_gpu.py, tests/test_anim_gpu.py).
'''
import base64
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TIMES = [0.0, 1.25, 0.8, 3.0]                      # t = 0, a key time, between keys, behind the last key (clamped: play(loop=False))
KEYS = [0.0, 0.5, 1.25, 2.0]
f32 = np.float32


def quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return [float(x) for x in (*(math.sin(0.5 * angle) * a), math.cos(0.5 * angle))]


# ---------------------------------------------------------------- the scene
NODES = [
    dict(name='base', translation=[0.3, 0.2, -0.4], rotation=quat([1, 2, 3], 0.4), scale=[1.1, 0.9, 1.05], children=[1, 8]),
    dict(name='arm', translation=[0.5, -0.1, 0.2], rotation=quat([3, -1, 2], -0.7), scale=[0.95, 1.0625, 1.02], children=[2]),
    dict(name='lamp', translation=[-0.2, 0.35, 0.15], rotation=quat([1, 1, -2], 1.1), scale=[0.8, 0.85, 0.9], mesh=0),
    dict(name='strip', translation=[9.0, 9.0, 9.0], rotation=quat([1, 0, 0], 1.0), scale=[2.0, 2.0, 2.0], mesh=1, skin=0),
    dict(name='rig', translation=[-0.6, 0.1, 0.3], rotation=quat([2, 3, -1], 0.5), scale=[1.05, 0.97, 1.01], children=[5]),
    dict(name='joint0', translation=[0.125, 0.25, -0.5], rotation=quat([1, -2, 1], 0.3), scale=[1.02, 0.98, 1.03], children=[6]),
    dict(name='joint1', translation=[0.1, 0.6, 0.05], rotation=quat([2, 1, 1], -0.45), scale=[0.99, 1.04, 0.96], children=[7]),
    dict(name='prop', translation=[0.15, 0.2, -0.1], rotation=quat([-1, 2, 2], 0.8), scale=[0.5, 0.55, 0.6], mesh=0),
    dict(name='pair', translation=[-0.3, 0.45, 0.25], rotation=quat([2, -1, -3], -0.6), scale=[0.7, 0.75, 0.72], mesh=2),
]
IBM = [[-0.25, 0.5, 0.125], [0.5, -0.75, -0.25]]     # inverse bind matrices: translations (their inverses, the bind matrices, are exact)
g = np.random.default_rng(2024)


def near_rotations(n, step=0.02):
    '''n unit rotations, neighbours within `step` radians of rotation: half that of arc, d = cos(step / 2) > 0.9995'''
    q = [np.array(quat(g.normal(size=3), 0.9))]
    for _ in range(n - 1):
        d = np.array(quat(g.normal(size=3), step))
        a, b = q[-1], d
        q.append(np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                           a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]))
    return np.array(q, f32)


def cubic(values, scale=0.2):
    '''[n,3,C]: in-tangent, value, out-tangent'''
    v = np.asarray(values, f32)
    return np.stack([g.uniform(-scale, scale, v.shape).astype(f32), v, g.uniform(-scale, scale, v.shape).astype(f32)], axis=1)


CHANNELS = [      # (node, path, interpolation, times, values)
    (0, 'translation', 'LINEAR', KEYS, g.uniform(-0.5, 0.5, (4, 3)).astype(f32)),
    (0, 'rotation', 'CUBICSPLINE', KEYS, cubic(near_rotations(4, 0.6))),
    (1, 'rotation', 'LINEAR', KEYS, near_rotations(4)),
    (1, 'scale', 'STEP', KEYS[:3], g.uniform(0.8, 1.2, (3, 3)).astype(f32)),
    (5, 'translation', 'STEP', KEYS, g.uniform(-0.3, 0.3, (4, 3)).astype(f32)),
    (6, 'rotation', 'LINEAR', KEYS[1:], near_rotations(3)),
    (3, 'weights', 'LINEAR', KEYS, g.uniform(0.1, 0.9, (4, 1)).astype(f32)),
]

# the strip: six vertices, four triangles, indexed; each vertex on joints (0, 1) with weights that sum to 1 in f32
STRIP_P = np.array([[x, y, 0.03 * x * y] for y in (0.0, 0.5, 1.0) for x in (-0.2, 0.2)], f32)
STRIP_N = np.array([[0.1 * x, 0.05, 1.0] for y in (0.0, 0.5, 1.0) for x in (-0.2, 0.2)], f32)
STRIP_N /= np.linalg.norm(STRIP_N, axis=1, keepdims=True).astype(f32)
STRIP_T = np.array([[0.5 + 2.5 * x, y] for y in (0.0, 0.5, 1.0) for x in (-0.2, 0.2)], f32)
STRIP_J = np.array([[0, 1, 0, 0]] * 6, np.uint8)
STRIP_W = np.array([[1 - a, a, 0, 0] for a in (0.125, 0.125, 0.5, 0.5, 0.875, 0.875)], f32)
STRIP_I = np.array([0, 1, 2, 2, 1, 3, 2, 3, 4, 4, 3, 5], np.uint16)
STRIP_DP = g.uniform(-0.1, 0.1, (6, 3)).astype(f32)
STRIP_DN = g.uniform(-0.2, 0.2, (6, 3)).astype(f32)
TRI_P = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.05], [0.1, 0.25, -0.05]], f32)
TRI_N = np.tile(np.array([[0.0, 0.6, 0.8]], f32), (3, 1))
TRI2_P = TRI_P[::-1] * f32(0.5) + f32(0.1)


# ---------------------------------------------------------------- the walk (plain floats, one operation at a time)
def mul4(A, B):
    return [[((A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c]) + A[r][3] * B[3][c] for c in range(4)] for r in range(4)]


def trs_matrix(t, q, s):
    x, y, z, w = q
    R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
         [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
         [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]]
    return [[R[r][0] * s[0], R[r][1] * s[1], R[r][2] * s[2], t[r]] for r in range(3)] + [[0.0, 0.0, 0.0, 1.0]]


def translation(v):
    return [[1.0, 0.0, 0.0, v[0]], [0.0, 1.0, 0.0, v[1]], [0.0, 0.0, 1.0, v[2]], [0.0, 0.0, 0.0, 1.0]]


EYE = translation([0.0, 0.0, 0.0])


def unit(q):
    ln = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [c / ln for c in q]


def sample(path, interp, times, values, tau):
    '''appendix C: the value of a sampler at tau, clamped outside its keys'''
    T = [float(x) for x in times]
    V = np.asarray(values, np.float64).tolist()                               # (f32 widens exactly)
    val = (lambda k: V[k][1]) if interp == 'CUBICSPLINE' else (lambda k: V[k])
    if len(T) == 1 or not tau > T[0]:
        return val(0)
    if tau >= T[-1]:
        return val(len(T) - 1)
    k = max(i for i in range(len(T)) if T[i] <= tau)
    dt = T[k + 1] - T[k]
    u = (tau - T[k]) / dt
    v0, v1 = val(k), val(k + 1)
    if interp == 'STEP':
        return v0
    if interp == 'LINEAR':
        if path != 'rotation':
            return [a + u * (b - a) for a, b in zip(v0, v1)]
        d = ((v0[0] * v1[0] + v0[1] * v1[1]) + v0[2] * v1[2]) + v0[3] * v1[3]
        if d < 0.0:
            v1, d = [-c for c in v1], -d
        assert d > 0.9995, 'the fixture stays on the lerp branch'
        return unit([a + u * (b - a) for a, b in zip(v0, v1)])
    b0, a1 = V[k][2], V[k + 1][0]
    u2 = u * u
    u3 = u2 * u
    h00, h10, h01, h11 = (2.0 * u3 - 3.0 * u2) + 1.0, (u3 - 2.0 * u2) + u, 3.0 * u2 - 2.0 * u3, u3 - u2
    g10, g11 = h10 * dt, h11 * dt
    p = [((h00 * v0[c] + g10 * b0[c]) + h01 * v1[c]) + g11 * a1[c] for c in range(len(v0))]
    return unit(p) if path == 'rotation' else p


def evaluate(t):
    '''(world per node -- of the OBJECT the loader makes of it; None for a joint --, morph weights, palette, deformed records)'''
    trs = [dict(translation=list(n['translation']), rotation=list(n['rotation']), scale=list(n['scale'])) for n in NODES]
    weights = [0.0]
    for node, path, interp, times, values in CHANNELS:
        v = sample(path, interp, times, values, t)
        if path == 'weights':
            weights = v
        else:
            trs[node][path] = v
    local = [trs_matrix(x['translation'], x['rotation'], x['scale']) for x in trs]
    world = [None] * len(NODES)
    world[0] = local[0]
    world[1] = mul4(world[0], local[1])
    world[2] = mul4(world[1], local[2])
    world[8] = mul4(world[0], local[8])
    world[4] = local[4]
    # the skin: joint matrices in the space of the node above the skeleton's root, globalJoint . inverseBind
    G0 = local[5]
    G1 = mul4(G0, local[6])
    pal = [mul4(G0, translation(IBM[0])), mul4(G1, translation(IBM[1]))]
    world[3] = mul4(world[4], EYE)                                            # the skinned object stands at the rig; its node's transform is ignored
    bind1 = translation([-c for c in IBM[1]])
    world[7] = mul4(world[3], mul4(pal[1], mul4(bind1, local[7])))            # the prop follows joint 1 as a vertex skinned to it would
    # the strip's corners: morph, then linear-blend skinning, then the normal's length
    rec = []
    for i in STRIP_I.tolist():
        q = [float(x) for x in STRIP_P[i]]
        m = [float(x) for x in STRIP_N[i]]
        w = weights[0]
        if w != 0.0:
            q = [q[k] + w * float(STRIP_DP[i][k]) for k in range(3)]
            m = [m[k] + w * float(STRIP_DN[i][k]) for k in range(3)]
        a = [float(x) for x in STRIP_W[i]]
        j = [int(x) for x in STRIP_J[i]]
        qs, ms = [], []
        for r in range(3):
            M = [((a[0] * pal[j[0]][r][c] + a[1] * pal[j[1]][r][c]) + a[2] * pal[j[2]][r][c]) + a[3] * pal[j[3]][r][c] for c in range(4)]
            qs.append(((M[0] * q[0] + M[1] * q[1]) + M[2] * q[2]) + M[3])
            ms.append((M[0] * m[0] + M[1] * m[1]) + M[2] * m[2])
        ln = math.sqrt((ms[0] * ms[0] + ms[1] * ms[1]) + ms[2] * ms[2])
        rec.append([*qs, ms[0] / ln, ms[1] / ln, ms[2] / ln, float(STRIP_T[i][0]), float(STRIP_T[i][1])])
    nan = [[float('nan')] * 4] * 4
    return (np.array([nan if w is None else w for w in world]), np.array(weights), np.array([p[:3] for p in pal]), np.array(rec).astype(f32),
            np.array(local))


# ---------------------------------------------------------------- the file
def write_gltf(path):
    blob, views, accessors = bytearray(), [], []

    def add(arr, kind, minmax=False):
        arr = np.ascontiguousarray(arr)
        while len(blob) % 4:
            blob.append(0)
        views.append(dict(buffer=0, byteOffset=len(blob), byteLength=arr.nbytes))
        blob.extend(arr.tobytes())
        comp = {np.dtype(f32): 5126, np.dtype(np.uint16): 5123, np.dtype(np.uint8): 5121}[arr.dtype]
        acc = dict(bufferView=len(views) - 1, componentType=comp, count=int(arr.shape[0]), type=kind)
        if minmax:
            acc['min'], acc['max'] = [float(x) for x in np.atleast_1d(arr.min(axis=0))], [float(x) for x in np.atleast_1d(arr.max(axis=0))]
        accessors.append(acc)
        return len(accessors) - 1
    tri = dict(attributes=dict(POSITION=add(TRI_P, 'VEC3', True), NORMAL=add(TRI_N, 'VEC3')), material=0)
    tri2 = dict(attributes=dict(POSITION=add(TRI2_P, 'VEC3', True), NORMAL=add(TRI_N, 'VEC3')))
    strip = dict(attributes=dict(POSITION=add(STRIP_P, 'VEC3', True), NORMAL=add(STRIP_N, 'VEC3'), TEXCOORD_0=add(STRIP_T, 'VEC2'),
                                 JOINTS_0=add(STRIP_J, 'VEC4'), WEIGHTS_0=add(STRIP_W, 'VEC4')),
                 indices=add(STRIP_I, 'SCALAR'), targets=[dict(POSITION=add(STRIP_DP, 'VEC3', True), NORMAL=add(STRIP_DN, 'VEC3'))], material=1)
    ibm = np.array([np.array(translation(v)).T.reshape(16) for v in IBM], f32)               # column-major, as the file holds matrices
    samplers, channels = [], []
    for node, what, interp, times, values in CHANNELS:
        v = np.asarray(values, f32)
        out = add(v.reshape(-1) if what == 'weights' else v.reshape(-1, v.shape[-1]), 'SCALAR' if what == 'weights' else {3: 'VEC3', 4: 'VEC4'}[v.shape[-1]])
        samplers.append(dict(input=add(np.array(times, f32), 'SCALAR', True), output=out, interpolation=interp))
        channels.append(dict(sampler=len(samplers) - 1, target=dict(node=node, path=what)))
    doc = dict(asset=dict(version='2.0', generator='tests/golden/make_gltf_anim_golden.py'), scene=0, scenes=[dict(nodes=[0, 3, 4])], nodes=NODES,
               meshes=[dict(name='triangle', primitives=[tri]), dict(name='strip', primitives=[strip], weights=[0.0]),
                       dict(name='pair', primitives=[tri, tri2])],
               skins=[dict(joints=[5, 6], inverseBindMatrices=add(ibm, 'MAT4'), skeleton=5)],
               materials=[dict(pbrMetallicRoughness=dict(baseColorFactor=[0.8, 0.2, 0.2, 1.0])), dict(pbrMetallicRoughness=dict(baseColorFactor=[0.2, 0.8, 0.2, 1.0]))],
               animations=[dict(name='wave', samplers=samplers, channels=channels)], accessors=accessors, bufferViews=views,
               buffers=[dict(byteLength=len(blob), uri='data:application/octet-stream;base64,' + base64.b64encode(bytes(blob)).decode('ascii'))])
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


def main():
    write_gltf(os.path.join(HERE, 'animated_scene.gltf'))
    out = dict(times=np.array(TIMES), strip_p=STRIP_P[STRIP_I].reshape(4, 3, 3), strip_n=STRIP_N[STRIP_I].reshape(4, 3, 3), strip_t=STRIP_T[STRIP_I].reshape(4, 3, 2),
               strip_joints=STRIP_J[STRIP_I].reshape(4, 3, 4).astype(np.int64), strip_weights=STRIP_W[STRIP_I].reshape(4, 3, 4),
               strip_dp=STRIP_DP[STRIP_I].reshape(1, 4, 3, 3), strip_dn=STRIP_DN[STRIP_I].reshape(1, 4, 3, 3), tri_p=TRI_P.reshape(1, 3, 3), tri2_p=TRI2_P.reshape(1, 3, 3),
               inverse_bind=np.array([translation(v) for v in IBM]), parents=np.array([-1, 0, 1, -1, -1, 4, 5, 6, 0]),
               channel_nodes=np.array([c[0] for c in CHANNELS]), rotation_keys=np.asarray(CHANNELS[1][4], f32), weight_keys=np.asarray(CHANNELS[6][4], f32))
    for k, t in enumerate(TIMES):
        world, w, pal, rec, local = evaluate(t)
        out.update({'world_%d' % k: world, 'weights_%d' % k: w, 'palette_%d' % k: pal, 'deformed_%d' % k: rec})
        if k == 0:
            rest = [trs_matrix(n['translation'], n['rotation'], n['scale']) for n in NODES]
            out['local'] = np.array(rest)
    np.savez_compressed(os.path.join(HERE, 'animated_scene_expected.npz'), **out)


if __name__ == '__main__':
    main()

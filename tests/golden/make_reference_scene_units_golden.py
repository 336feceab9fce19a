#!/usr/bin/env python3
'''
Function-level vectors for the device functions that READ SCENE STATE: the reference's own `@ti.func` bodies --
LightPool.hit / .sample (light/__init__.py:51-121), Image.__call__ + bilerp (image.py:137-148, common.py:183-192),
WorldLight.at (light/world.py:22-29), MaterialPool.get (mtllib.py:30-38,79-95) + Disney.__init__ (disney.py:13-50),
Camera.generate (camera.py:34-39) and the normal flip of ModelPool.get_geometries (model.py:88-101) -- imported
from the reference with the pure-Python `taichi` stand-in of tests/golden/taichi_standin and run on ONE small scene
state that is built through the reference's own setters (LightPool.add, ImagePool.new, MaterialPool.load,
WorldLight.set, Camera.set_perspective).  The state is stored in the fixture as plain arrays, so that the tests
upload the identical state through ptina_amd's classes and through the oracle's C API.

Writes tests/golden/reference_scene_units.npz with keys f32/... and f64/... (one child process per precision;
the singletons' fields take the precision they are created with).  tests/test_reference_scene_units_cpu.py holds
the C oracle to it, tests/test_reference_scene_units_gpu.py the HIP device functions.

Build container only; no reference text is copied.  Inputs are exactly representable in f32 (the f64 run gets the
f32-rounded scene parameters the C APIs take, as in make_reference_path_golden.py).  What is emulated rather than
executed is the same compile-time machinery as there: kernel-scope int / float / min / max in ptina.common, the
`subscript` protocol of ImagePool / Image / ModelPool, and ImagePool.from_numpy's lvalue writes (texels are stored
into the field directly; ids and base offsets come from the reference's own allocators).

Per function, rows carry a `cls` code; `CLASSES` below names them and the generator ASSERTS the per-class row
counts before it writes (the CPU test re-asserts them from the fixture).

usage: python3 tests/golden/make_reference_scene_units_golden.py     (from the repo root; PTINA_REFERENCE names the reference)
'''

import os
import subprocess
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('PTINA_REFERENCE', '/root/reference')
MIN_ROWS = 8

# row classes (the `cls` arrays of the fixture)
CLASSES = {
    'light_hit': {0: 'first hit: light 0', 1: 'first hit: light 1', 2: 'first hit: light 2', 3: 'first hit: light 3',
                  4: 'first hit: light 4', 5: 'two lights on the ray, the nearer has the lower index',
                  6: 'two lights on the ray, the nearer has the higher index (it loses: the break)',
                  7: 'miss', 8: 'grazes a POINT sphere', 9: 'starts inside a POINT sphere',
                  10: 'crosses an AREA light from behind'},
    'light_sample': {0: 'bin centre', 1: 'bin edge k / count', 2: 'largest f32 below 1', 3: 'samp.z == 1.0 (record `count`: informational)',
                     4: 'hitpos behind an AREA light (cosine clamped to 0)', 5: 'hitpos close to the light'},
    'image_sample': {0: 'random in [-1.5, 2.5]', 1: 'exactly on a texel', 2: '0 / 1 / -1e-7 / 1 + 1e-7'},
    'world_at': {0: 'axis', 1: 'seam', 2: 'near a pole', 3: 'random'},
    'material_get': {0: 'inside a texel', 1: 'outside [0, 1]', 2: 'exactly on a texel'},
    'camera_generate': {0: 'corner', 1: 'centre', 2: 'grid / random'},
    'face_side': {0: 'dot(rd, n) < 0', 1: 'dot(rd, n) > 0', 2: '|dot(rd, n)| < 1e-6 (informational)'},
}

f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)     # noqa: E731


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) * c + s * K + (1 - c) * np.outer(a, a)


def world_of(lin, pos):
    w = np.eye(4)
    w[:3, :3] = f32(lin)
    w[:3, 3] = f32(pos)
    return w


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def scene_state():
    '''the one scene state, as plain arrays of f32-representable values'''
    sys.path.insert(0, ROOT)
    from ptina_amd import scenes
    from ptina_amd.tools.matrix import perspective, lookat
    rng = np.random.default_rng(20261016)
    up = np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]])            # axes @ z = +y: the light shines down
    lights = [      # (world, color, size, type): distinct colours tell which light won
        (world_of(up, (0.0, 3.0, 0.0)), (12.0, 11.0, 9.0), 0.75, 'AREA'),
        (world_of(np.eye(3), (0.25, 1.5, 0.125)), (20.0, 5.0, 24.0), 0.5, 'POINT'),       # in front of light 0 from below
        (world_of(rot((1, 2, 3), 40) @ rot((0, 1, 0), 25), (2.5, 1.0, -1.0)), (3.0, 14.0, 6.0), 0.625, 'AREA'),
        (world_of(np.eye(3), (-2.0, 0.5, 1.0)), (40.0, 41.0, 7.0), 0.0625, 'POINT'),
        (world_of(rot((1, 0, 0), 10), (-1.0, 2.0, -2.5)), (2.0, 8.0, 17.0), 0.5, 'AREA'),   # normal ~ +z: seen from behind from the origin
    ]
    images = [scenes.env_image(32, 16).astype(np.float32)]
    for nx, ny in ((5, 7), (1, 4), (4, 1)):
        images.append(rng.uniform(0.3, 1.0, (nx, ny, 4)).astype(np.float32))      # all four channels differ
    images[0][..., 3] = rng.uniform(0.3, 1.0, (32, 16)).astype(np.float32)
    # materials: 12 x (fac, tex); scalar factors of the textured material are 4-vectors whose components differ, so that
    # `.x of fac * texel` shows.  11 scalar parameters all read channel x of one of four images: they share images by
    # necessity, never a (factor, image) pair
    plain = [((0.7, 0.25, 0.125), -1), (0.25, -1), (0.5, -1), (0.75, -1), (0.625, -1), (0.375, -1), (0.5, -1), (0.875, -1),
             (0.75, -1), (0.25, -1), (0.125, -1), (1.5, -1)]
    facs = rng.uniform(0.4, 1.0, (12, 4))
    facs[11] += 1.0                                                 # ior stays well above 0
    full = [(f32(facs[k]).tolist(), (1, 2, 3, 0)[k % 4]) for k in range(12)]
    full[0] = (f32(facs[0][:3]).tolist(), 1)
    base_only = [((0.875, 0.75, 0.5), 1)] + [(p[0], -1) for p in plain[1:]]
    cams = [np.asarray(scenes.BENCH_CAMERA, np.float64),
            np.asarray(perspective(fov=50, aspect=1.6, near=0.1, far=50) @ lookat(pos=(0.3, 1.0, -0.2), back=(2.0, 1.5, 3.0)), np.float64)]
    return lights, images, [plain, full, base_only], cams


# ---------------------------------------------------------------------------------------------------- inputs
def light_geometry(lights):
    out = []
    for w, _, size, type in lights:
        pos, ax = w[:3, 3], w[:3, :3]
        out.append((type, pos, ax, size, ax @ np.array([0, 0, 1.0])))
    return out


def light_hit_rays(lights, rng):
    '''candidate rays (ro, rd, wanted class or -1); the class of a row is decided from the reference's per-light tests'''
    G = light_geometry(lights)
    rays = []

    def on_light(k, spread=0.8):
        type, pos, ax, size, nrm = G[k]
        if type == 'AREA':
            uv = rng.uniform(-spread, spread, 2)
            return pos + size * (ax @ np.array([uv[0], uv[1], 0.0]))
        return pos + size * 0.5 * spread * unit(rng, 1)[0]

    def front_origin(k, dist):
        type, pos, ax, size, nrm = G[k]
        side = unit(rng, 1)[0]
        if type == 'AREA':
            side = side - nrm * (side @ nrm) * 0.8 - nrm * 1.0      # the lit side is -normal (Area.intersect wants NoD > 0)
        return pos + dist * side / np.linalg.norm(side)
    for k in range(len(G)):
        for _ in range(40):
            o = front_origin(k, rng.uniform(1.0, 4.0))
            d = on_light(k) - o
            rays.append((o, d, -1))
    # two lights along one ray: through a point of light a towards a point of light b, started before a, and reversed
    for a in range(len(G)):
        for b in range(len(G)):
            if a == b:
                continue
            for _ in range(30):
                pa, pb = on_light(a, 0.6), on_light(b, 0.6)
                d = pb - pa
                rays.append((pa - d / np.linalg.norm(d) * rng.uniform(0.5, 2.0), d, -1))
    for _ in range(60):                                            # misses: away from every light
        rays.append((rng.uniform(-1, 1, 3) + np.array([0, -6.0, 0]), unit(rng, 1)[0] * np.array([1, 0.2, 1]) - np.array([0, 0.6, 0]), 7))
    type, pos, ax, size, _ = G[1]                                  # grazing the POINT sphere of light 1 (radius = size)
    for delta in (-1e-2, 1e-2, -3e-3, 3e-3, -1e-3, 1e-3) * 3:
        d = unit(rng, 1)[0]
        side = np.cross(d, unit(rng, 1)[0])
        side /= np.linalg.norm(side)
        rays.append((pos + side * size * (1 + delta) - d * rng.uniform(1.0, 3.0), d, 8))
    for k in (1, 3):                                               # starting inside a POINT sphere
        type, pos, ax, size, _ = G[k]
        for _ in range(8):
            rays.append((pos + unit(rng, 1)[0] * size * rng.uniform(0.05, 0.7), unit(rng, 1)[0], 9))
    for k in (0, 2, 4):                                            # through an AREA light's rectangle from behind
        type, pos, ax, size, nrm = G[k]
        for _ in range(8):
            p = on_light(k, 0.7)
            side = unit(rng, 1)[0]
            o = p + (nrm * 1.0 + 0.4 * side) * rng.uniform(0.5, 2.0)
            rays.append((o, p - o, 10))
    ro = f32(np.array([r[0] for r in rays]))
    rd = np.array([r[1] for r in rays])
    rd = f32(rd / np.linalg.norm(rd, axis=1, keepdims=True))
    return ro, rd, np.array([r[2] for r in rays])


def light_sample_rows(lights, rng):
    n = len(lights)
    below1 = float(np.nextafter(np.float32(1), np.float32(0)))
    G = light_geometry(lights)
    rows, cls = [], []

    def put(hp, z, c):
        xy = rng.uniform(0, 1, 2)
        rows.append([*hp, xy[0], xy[1], z])
        cls.append(c)
    far = lambda: rng.uniform(-2.5, 2.5, 3) + np.array([0, -1.0, 0])         # noqa: E731
    for k in range(max(n, 1)):
        for _ in range(6):
            put(far(), (k + rng.uniform(0.1, 0.9)) / max(n, 1), 0)
        for _ in range(4):
            put(far(), float(np.float32(k / max(n, 1))), 1)
    for _ in range(MIN_ROWS):
        put(far(), below1, 2)
        put(far(), 1.0, 3)
    for k, (type, pos, ax, size, nrm) in enumerate(G):
        z = (k + 0.5) / n
        lateral = lambda: ax @ np.array([*rng.uniform(-1.5, 1.5, 2), 0.0]) * size     # noqa: E731
        if type == 'AREA':
            for _ in range(6):
                put(pos - nrm * rng.uniform(0.5, 3.0) + lateral(), z, 0)              # lit side
                put(pos + nrm * rng.uniform(0.5, 3.0) + lateral(), z, 4)              # behind: dot_or_zero clamps
            for _ in range(3):
                put(pos - nrm * 0.015625 + lateral() * 0.3, z, 5)
        else:
            for _ in range(3):
                put(pos + unit(rng, 1)[0] * size * 1.0625, z, 5)
    return f32(rows), np.array(cls)


def image_rows(images, rng):
    rows, cls = [], []
    tiny = 1e-7
    for i, im in enumerate(images):
        nx, ny = im.shape[:2]
        for _ in range(24):
            rows.append([i, *rng.uniform(-1.5, 2.5, 2)])
            cls.append(0)
        gx = [a / (nx - 1) for a in range(nx)] if nx > 1 else [0.0, 0.5, 1.0]
        gy = [b / (ny - 1) for b in range(ny)] if ny > 1 else [0.0, 0.5, 1.0]
        for x in (gx if len(gx) <= 7 else gx[:3] + gx[-3:] + [gx[len(gx) // 2]]):
            for y in (gy if len(gy) <= 7 else gy[:3] + gy[-3:] + [gy[len(gy) // 2]]):
                rows.append([i, x, y])
                cls.append(1)
        for k in range(3):                                      # exact texel positions one period below and above [0, 1]
            rows.append([i, gx[k % len(gx)] - 1.0, gy[-1 - k % len(gy)] + 1.0])
            cls.append(1)
        edge = (0.0, 1.0, -tiny, 1.0 + tiny)
        for x in edge:
            for y in edge:
                rows.append([i, x, y])
                cls.append(2)
    return f32(rows), np.array(cls)


def world_rows(rng):
    rows, cls = [], []
    for a in range(3):
        for s in (1.0, -1.0):
            d = np.zeros(3)
            d[a] = s
            rows.append(d)
            cls.append(0)
    for y in (0.0, -0.0, 1e-6, -1e-6, 1e-3, -1e-3, 1e-2, -1e-2):      # the swap makes atan2(-dir.y, dir.x): seam at x < 0, y -> 0
        for z in (0.0, 0.4):
            rows.append([-1.0, y, z])
            cls.append(1)
    for zs in (1.0, -1.0):                                           # after the swap dir.z is the pole axis
        for e in ((1e-4, 1e-4), (-1e-3, 2e-3), (1e-2, -1e-2), (0.0, 1e-5), (3e-3, 0.0)):
            rows.append([e[0], e[1], zs])
            cls.append(2)
    for d in unit(rng, 48) * rng.uniform(0.2, 3.0, (48, 1)):
        rows.append(d)
        cls.append(3)
    return f32(rows), np.array(cls)


def material_rows(images, rng):
    rows, cls = [], []
    for m in (0, 1, 2, -1):
        for _ in range(10):
            rows.append([m, *rng.uniform(0.02, 0.98, 2)])
            cls.append(0)
        for _ in range(10):
            t = rng.uniform(-1.5, 2.5, 2)
            k = int(rng.integers(2))
            if 0.0 <= t[k] <= 1.0:
                t[k] += 1.25 if t[1 - k] > 0.5 else -1.25
            rows.append([m, *t])
            cls.append(1)
        for a, b in ((0, 0), (1, 2), (2, 5), (4, 6), (3, 3), (2, 0), (0, 6), (4, 0), (1, 1), (3, 4)):     # texels of the 5 x 7 image
            rows.append([m, a / 4, b / 6])
            cls.append(2)
    return f32(rows), np.array(cls)


def camera_rows(rng):
    rows, cls = [], []
    for x in (-1.0, 1.0):
        for y in (-1.0, 1.0):
            for _ in range(2):
                rows.append([x, y])
                cls.append(0)
    for _ in range(MIN_ROWS):
        rows.append([0.0, 0.0])
        cls.append(1)
    for x in (-1.0, -0.5, 0.0, 0.5, 1.0):
        for y in (-1.0, -0.25, 0.0, 0.75, 1.0):
            rows.append([x, y])
            cls.append(2)
    for xy in rng.uniform(-1, 1, (16, 2)):
        rows.append(xy)
        cls.append(2)
    return f32(rows), np.array(cls)


def face_rows(rng):
    rows = []
    for k in range(48):
        n = unit(rng, 1)[0]
        vn = n + 0.3 * rng.normal(size=(3, 3))
        st = rng.uniform(0, 0.5, 2)
        rows.append([*unit(rng, 1)[0], *vn.reshape(-1), *st])
    for k in range(MIN_ROWS):                                       # rd within 1e-6 of perpendicular to the shading normal
        n = unit(rng, 1)[0]
        t = np.cross(n, unit(rng, 1)[0])
        t /= np.linalg.norm(t)
        rd = t + n * (2e-7 if k % 2 else -2e-7)
        rows.append([*rd, *n, *n, *n, 0.25, 0.25])
    return f32(rows)


# ---------------------------------------------------------------------------------------------------- the reference
def child(prec):
    T = np.float64 if prec == 'f64' else np.float32
    sys.path.insert(0, os.path.join(HERE, 'taichi_standin'))
    sys.path.insert(0, REF)
    warnings.filterwarnings('ignore', category=RuntimeWarning)
    import taichi as ti
    assert 'taichi_standin' in ti.__file__
    ti.set_default_fp(T)
    import ptina.common as C
    import ptina.geometries as GEO
    from ptina.light import LightPool
    from ptina.light.world import WorldLight
    from ptina.image import ImagePool, Image
    from ptina.mtllib import MaterialPool
    from ptina.camera import Camera
    from ptina.model import ModelPool
    import ptina.tools.matrix  # noqa: F401  (Camera() imports it lazily: it must star-import common before the names below exist)
    C.int, C.float, C.min, C.max = ti.ti_int, ti.ti_float, ti.min, ti.max       # kernel-scope builtins of ifloor / clamp / bilerp
    ModelPool.__getitem__ = lambda self, i: self.subscript(i)
    ImagePool.__getitem__ = lambda self, ix: self.subscript(*ix)
    Image.__getitem__ = lambda self, I: self.subscript(*I)

    lights, images, materials, cams = scene_state()
    rng = np.random.default_rng(20261017)
    out = {}
    put = lambda k, a, dt=np.float64: out.__setitem__(k, np.asarray(a, dt))     # noqa: E731
    vec = lambda a: C.V(*[T(x) for x in a])                                     # noqa: E731
    arr = lambda v: [float(e) for e in v.entries] if isinstance(v, ti.Matrix) else float(v)   # noqa: E731

    def f32_values(*fields):
        if prec == 'f64':
            for fld in fields:
                fld.data[...] = fld.data.astype(np.float32).astype(np.float64)

    # ---- the scene state, through the reference's setters
    pool = ImagePool(2**12, 2**3)
    pool.mman.reset()
    pool.idman.reset()
    for k, im in enumerate(images):
        iid = pool.new(im.shape[0], im.shape[1])
        base = int(pool.base[iid])
        assert iid == k
        pool.root.data[base:base + im.shape[0] * im.shape[1]] = im.astype(np.float32).reshape(-1, 4)
        put(f'state/image{k}', im, np.float32)
    mp = MaterialPool(2**3)
    mp.load(materials)
    f32_values(*[getattr(mp, n).fac for n in ('basecolor', 'metallic', 'roughness', 'specular', 'specularTint', 'subsurface',
                                               'sheen', 'sheenTint', 'clearcoat', 'clearcoatGloss', 'transmission', 'ior')])
    fac = np.zeros((len(materials), 12, 4))
    tex = np.zeros((len(materials), 12), np.int64)
    for i, m in enumerate(materials):
        for k, (f, t) in enumerate(m):
            f = np.asarray(f, np.float64)
            fac[i, k] = np.full(4, float(f)) if f.ndim == 0 else (np.concatenate([f, [1.0]]) if f.shape[0] == 3 else f)
            tex[i, k] = t
    put('state/material_fac', f32(fac))
    put('state/material_tex', tex, np.int64)
    put('state/light_world', np.array([l[0] for l in lights]))
    put('state/light_color', np.array([l[1] for l in lights]))
    put('state/light_size', np.array([l[2] for l in lights]))
    put('state/light_type', np.array([LightPool.TYPES[l[3]] for l in lights]), np.int64)
    put('state/camera_pers', np.array(cams))
    lp = LightPool(2**3)
    wl = WorldLight()
    cam = Camera()
    ModelPool(2**4)

    def set_lights(ls):
        lp.clear()
        for fld in (lp.color, lp.pos, lp.axes, lp.size, lp.type):
            fld.data[...] = 0                   # record `count` is a zero-filled record of type 0, as in a fresh pool
        for l in ls:
            lp.add(l[0], np.asarray(l[1], np.float64), l[2], l[3])
        f32_values(lp.color, lp.pos, lp.axes, lp.size)

    # ---- light_hit / light_sample on the three light states
    ro, rd, want = light_hit_rays(lights, rng)
    for name, ls in (('five', lights), ('one', lights[2:3]), ('none', [])):
        set_lights(ls)
        if name != 'five':
            ro, rd, want = ro[::5], rd[::5], want[::5]
        res, cls = [], []
        for o, d, w in zip(ro, rd, want):
            ray = GEO.Ray(vec(o), vec(d))
            h = lp.hit(ray)
            res.append([float(h.hit), float(h.dis), float(h.pdf), *arr(h.color)])
            # which lights the ray meets, by the reference's own per-light tests
            ts = []
            for i, l in enumerate(ls):
                if l[3] == 'POINT':
                    t = float(GEO.Sphere(lp.pos[i], lp.size[i]**2).intersect(ray))
                else:
                    ah = GEO.Area(lp.pos[i], lp.axes[i] @ C.V(lp.size[i], 0.0, 0.0), lp.axes[i] @ C.V(0.0, lp.size[i], 0.0)).intersect(ray)
                    t = float(ah.depth) if ah.hit else 0.0
                ts.append(t)
            met = [i for i, t in enumerate(ts) if 0 < t < 1e6]
            if w in (8, 9, 10):
                c = w
            elif not met:
                c = 7
            elif len(met) == 1:
                c = met[0] if name == 'five' else 0
            else:
                near = min(met, key=lambda i: ts[i])
                c = 5 if near == met[0] else 6
            cls.append(c)
        res, cls = np.array(res), np.array(cls)
        if name == 'five':
            keep = np.zeros(len(cls), bool)            # at most 16 rows per class
            for c in sorted(set(cls.tolist())):
                keep[np.nonzero(cls == c)[0][:16]] = True
            sel = (ro[keep], rd[keep], res[keep], cls[keep])
            for c in CLASSES['light_hit']:
                assert (sel[3] == c).sum() >= MIN_ROWS, f'{prec} light_hit: {int((sel[3] == c).sum())} rows of class {c} ({CLASSES["light_hit"][c]})'
            colors = {tuple(l[1]): i for i, l in enumerate(ls)}
            won = np.array([colors.get(tuple(r[3:6]), -1) for r in sel[2]])
            assert (won[sel[3] == 6] >= 0).all() and (sel[2][sel[3] == 10][:, 0] == 0).sum() >= 1
        else:
            sel = (ro, rd, res, cls)
            if name == 'one':
                assert (res[:, 0] == 1).sum() >= MIN_ROWS and (res[:, 0] == 0).sum() >= MIN_ROWS, 'the one-light state needs hits and misses of its light'
        put(f'{prec}/light_hit/{name}/in', np.column_stack([sel[0], sel[1]]))
        put(f'{prec}/light_hit/{name}/out', sel[2])
        put(f'{prec}/light_hit/{name}/cls', sel[3], np.int64)

        rows, cls = light_sample_rows(ls, np.random.default_rng(7 + len(ls)))
        res = []
        for r in rows:
            s = lp.sample(vec(r[0:3]), vec(r[3:6]))
            res.append([float(s.dis), *arr(s.dir), float(s.pdf), *arr(s.color)])
        res = np.array(res)
        if name == 'five':
            for c in CLASSES['light_sample']:
                assert (cls == c).sum() >= MIN_ROWS, f'light_sample: class {c}'
            assert (res[cls == 4][:, 5:8] == 0).all(), 'behind an AREA light the cosine must clamp to 0'
            assert (res[cls == 5][:, 5:8].max(axis=1) > 50).any(), 'no hitpos close enough for a large 1 / pdf'
        put(f'{prec}/light_sample/{name}/in', rows)
        put(f'{prec}/light_sample/{name}/out', res)
        put(f'{prec}/light_sample/{name}/cls', cls, np.int64)

    # ---- image_sample
    rows, cls = image_rows(images, rng)
    res = [arr(Image(int(r[0]))(T(r[1]), T(r[2]))) for r in rows]
    for c in CLASSES['image_sample']:
        for i in range(len(images)):
            assert ((cls == c) & (rows[:, 0] == i)).sum() >= MIN_ROWS, f'image_sample: class {c}, image {i}'
    put(f'{prec}/image_sample/in', rows)
    put(f'{prec}/image_sample/out', res)
    put(f'{prec}/image_sample/cls', cls, np.int64)

    # ---- world_at: without and with the environment image
    rows, cls = world_rows(rng)
    for c in CLASSES['world_at']:
        assert (cls == c).sum() >= (6 if c == 0 else MIN_ROWS)
    put('state/world_fac', f32([[0.25, 0.5, 0.125, 0.75], [1.0, 0.875, 0.75, 0.5]]))
    for name, (fac_, tex_) in (('plain', (out['state/world_fac'][0], -1)), ('env', (out['state/world_fac'][1], 0))):
        wl.set([float(x) for x in fac_], tex_)
        put(f'{prec}/world_at/{name}/in', rows)
        put(f'{prec}/world_at/{name}/out', [arr(wl.at(vec(r))) for r in rows])
        put(f'{prec}/world_at/{name}/cls', cls, np.int64)

    # ---- material_get: the twelve parameters (14 floats), speccolor, sheencolor, alpha, clearcoatAlpha
    rows, cls = material_rows(images, rng)
    res = []
    for r in rows:
        m = mp.get(int(r[0]), vec(r[1:3]))
        res.append([*arr(m.basecolor), *[float(getattr(m, k)) for k in (
            'metallic', 'roughness', 'specular', 'specularTint', 'subsurface', 'sheen', 'sheenTint', 'clearcoat', 'clearcoatGloss',
            'transmission', 'ior')], *arr(m.speccolor), *arr(m.sheencolor), float(m.alpha), float(m.clearcoatAlpha)])
    for c in CLASSES['material_get']:
        for m in (0, 1, 2, -1):
            assert ((cls == c) & (rows[:, 0] == m)).sum() >= MIN_ROWS, f'material_get: class {c}, material {m}'
    put(f'{prec}/material_get/in', rows)
    put(f'{prec}/material_get/out', res)
    put(f'{prec}/material_get/cls', cls, np.int64)

    # ---- camera_generate on both cameras
    rows, cls = camera_rows(rng)
    for c in CLASSES['camera_generate']:
        assert (cls == c).sum() >= MIN_ROWS
    v2w = []
    for k, pers in enumerate(cams):
        cam.set_perspective(pers)
        f32_values(cam._V2W, cam._W2V)
        v2w.append(cam._V2W.to_numpy().astype(np.float32))
        res = []
        for x, y in rows:
            ray = cam.generate(T(x), T(y))
            res.append([*arr(ray.o), *arr(ray.d)])
        put(f'{prec}/camera_generate/cam{k}/in', rows)
        put(f'{prec}/camera_generate/cam{k}/out', res)
        put(f'{prec}/camera_generate/cam{k}/cls', cls, np.int64)
    put('state/camera_v2w', np.array(v2w), np.float32)

    # ---- the normal flip of get_geometries: one face, mtlid -1, per row
    rows = face_rows(rng)
    model = ModelPool()
    model.nfaces[None] = 1
    model.mtlids.data[...] = -1
    res = []
    for r in rows:
        v = np.zeros((3, 8))
        v[:, 0:3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
        v[:, 3:6] = r[3:12].reshape(3, 3)
        model.vertices.data[:24] = v.reshape(-1)
        hit = C.namespace(hit=1, depth=T(1.0), index=0, uv=vec(r[12:14]))
        _, normal, sign, _ = model.get_geometries(hit, GEO.Ray(vec([0.0, 0.0, 0.0]), vec(r[0:3])))
        res.append([*arr(normal), float(sign)])
    res = np.array(res)
    cls = np.where(np.abs(res[:, 3]) < 1e-6, 2, np.where(res[:, 3] > 0, 0, 1))     # sign = -dot(rd, n)
    for c in CLASSES['face_side']:
        assert (cls == c).sum() >= (6 if c == 2 else MIN_ROWS), f'face_side: class {c}: {(cls == c).sum()}'
    put(f'{prec}/face_side/in', rows)
    put(f'{prec}/face_side/out', res)
    put(f'{prec}/face_side/cls', cls, np.int64)
    np.savez_compressed(os.path.join(HERE, f'_reference_scene_units_{prec}.npz'), **out)


def main():
    if len(sys.argv) > 1:
        return child(sys.argv[1])
    procs = [(p, subprocess.Popen([sys.executable, os.path.abspath(__file__), p])) for p in ('f32', 'f64')]
    for p, proc in procs:
        if proc.wait() != 0:
            raise SystemExit(f'{p} run failed')
    merged = {}
    for p, _ in procs:
        f = os.path.join(HERE, f'_reference_scene_units_{p}.npz')
        z = np.load(f)
        for k in z.files:
            if k.startswith('state/') and k in merged:
                assert np.array_equal(merged[k], z[k]), f'{k}: the two runs were given different scene states'
            merged[k] = z[k]
        os.remove(f)
    # the two runs got the same rows, took the same discrete decisions on every row that is not informational
    for k in [k for k in merged if k.startswith('f32/') and k.endswith('/in')]:
        assert np.array_equal(merged[k], merged['f64' + k[3:]]), f'{k}: inputs differ between the runs'
        assert np.array_equal(merged[k[:-2] + 'cls'], merged['f64' + k[3:-2] + 'cls']), f'{k}: classes differ between the runs'
    for s in ('five', 'one', 'none'):
        a, b = merged[f'f32/light_hit/{s}/out'], merged[f'f64/light_hit/{s}/out']
        assert np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(a[:, 3:], b[:, 3:]), f'light_hit/{s}: a hit decided differently by the two runs'
    merged['classes'] = np.array([f'{f}:{c}:{t}' for f, d in CLASSES.items() for c, t in d.items()])
    dst = os.path.join(HERE, 'reference_scene_units.npz')
    np.savez_compressed(dst, **merged)
    print('wrote', dst, os.path.getsize(dst), 'bytes,', len(merged), 'arrays')


if __name__ == '__main__':
    main()

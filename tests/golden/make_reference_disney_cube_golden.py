#!/usr/bin/env python3
'''
Disney.brdf and Disney.bounce over the WHOLE parameter cube: the reference's own function bodies (materials/disney.py:13-233,
Choice of materials/__init__.py:37-48), imported from the reference with the pure-Python `taichi` stand-in of
tests/golden/taichi_standin and evaluated in single and in double precision on rows drawn class by class, written to
tests/golden/reference_disney_cube.npz.  tests/test_reference_disney_cube_cpu.py holds the C oracle to these vectors,
tests/test_reference_disney_cube_gpu.py the HIP device functions of both builds (tests/disney_cube.py: the shared checks).

tests/golden/reference_l1.npz holds ten preset materials x 40 random direction triples; this fixture is the complement.  A row
is the product of three axes, each drawn with the fixed seed from the classes below (MATERIALS / DIRECTIONS / SAMPLES name
them; the fixture stores one class word per row per axis and the names):
  materials   every parameter uniform | each of the ten scalars metallic .. transmission pinned at exactly 0, and at exactly 1 |
              the plain mask (clearcoat = transmission = 0) | the lean rule (sheen = subsurface = 0 as well, -0.0 among them) |
              base colour black, luminance just above / below eps (the tint branch of Disney.__init__) | ior 1, 1.0001, 0.8 |
              roughness 0, sqrt(0.001) (the alpha clamp), 1
  directions  general | cosi in [1e-6, 1e-2] | indir == normal, and within 1e-4 of it | outdir below the surface | outdir grazing |
              outdir the mirror of indir | outdir == -indir (the half vector is normalized(0)) | sign = -1 at the critical angle (where the
              row's material has ior > 1; with ior <= 1 there is none and the incidence stays general)
  samples     uniform | samp.z in {0, 2^-24, nextafter(1, 0)} | samp.z at a Choice threshold of that row x (1 +- 1e-4), the
              thresholds read from the spy in a double precision run | samp.x, samp.y in {0, nextafter(1, 0)}

Inputs are stored as f32 (the f64 run takes the same values widened), the f32 outputs as f32, the f64 outputs as f64, and per
run the branch word of the Choice spy (the decisions as bits under a leading 1).  A row on which the two runs take different
branches is kept and FLAGGED (branch32 != branch64); at most FLAG_CAP of the rows may be.  A row is WELL-CONDITIONED when it is
not flagged and 4 x |f32 - f64| is below the base bound (relative 5e-5 + absolute 2e-6 of the f32 value) on every one of its ten
outputs, a non-finite value counting as equal to the same non-finite value.  Asserted before writing: every class of every
axis and every leaf of the Choice tree has MIN_ROWS rows, MIN_ROWS of them well-conditioned; the critical-angle class has
MIN_ROWS well-conditioned rows that do have a critical angle; and the threshold class sits at the threshold of every one of the
four Choice calls (coat, spec, trans, refl) on either side on MIN_ROWS unflagged rows each -- `threshold` stores, per row of that
class, 1 + the call and the side (0, 0 elsewhere, and where the rate is exactly 0 or 1, or so near 1 that samp.z < 1 clips the
upper side away).
Material classes 2 and 29 are both "roughness = 0": the list above names it twice, as one of the ten scalars and as one of the
three roughness values, and both are drawn, so the class has twice the rows.

Build container only: neither the reference nor the stand-in is needed at test time.  It reads the reference; it copies none of
it.  The archive is written with fixed time stamps, so the same seed gives the same bytes.

usage: python3 tests/golden/make_reference_disney_cube_golden.py   (from the repo root; PTINA_REFERENCE names the reference,
       PTINA_GOLDEN_OUT another file to write, for comparing with the committed one byte by byte)
'''

import io
import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('PTINA_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.join(HERE, 'taichi_standin'))
sys.path.insert(0, REF)
warnings.filterwarnings('ignore', category=RuntimeWarning)        # 0 / 0, sqrt of negatives: wanted

import taichi as ti                                    # noqa: E402  (the stand-in)
import ptina.common as C                               # noqa: E402
import ptina.materials as MAT                          # noqa: E402
import ptina.materials.disney as DIS                   # noqa: E402

assert 'taichi_standin' in ti.__file__

SEED = 20261020
ROWS = 1200
MIN_ROWS = 8
FLAG_CAP = 0.01
BASE_REL, BASE_ABS = 5e-5, 2e-6          # Disney.brdf's bound in tests/test_reference_l1_cpu.py
OFFSET = 1e-4                            # samp.z = threshold x (1 +- OFFSET)
EPS = 1e-6                               # common.py:32

SCALARS = ('metallic', 'roughness', 'specular', 'specularTint', 'subsurface', 'sheen', 'sheenTint', 'clearcoat', 'clearcoatGloss',
           'transmission')              # columns 3 .. 12 of a row; ior is column 13
MATERIALS = (['interior'] + [f'{k} = 0' for k in SCALARS] + [f'{k} = 1' for k in SCALARS] +
             ['plain mask: clearcoat = transmission = 0', 'lean rule: sheen = subsurface = +-0 as well', 'base colour black',
              'luminance just above eps', 'luminance just below eps', 'ior = 1', 'ior = 1.0001', 'ior = 0.8', 'roughness = 0',
              'roughness = sqrt(0.001)', 'roughness = 1'])
M_PLAIN, M_LEAN = 21, 22
# the plain and the lean class feed the function-level test of the plain / lean instantiations: four shares each; roughness 0
# (alpha = 0.001: GTR2 cancels) needs two to reach MIN_ROWS well-conditioned rows
M_WEIGHTS = np.array([2.0] + [1.0] * 20 + [4.0, 4.0] + [1.0] * 9)
M_WEIGHTS[[2, 29]] = 2.0
DIRECTIONS = ['general hemisphere', 'cosi in [1e-6, 1e-2]', 'indir == normal', 'indir within 1e-4 of normal', 'outdir below the surface',
              'outdir grazing', 'outdir the mirror of indir', 'outdir == -indir', 'sign = -1, incidence within 1e-3 of the critical angle']
D_WEIGHTS = np.array([3.0, 1.0, 1.0, 1.0, 1.5, 1.0, 1.0, 0.5, 1.0])
SAMPLES = ['uniform', 'samp.z in {0, 2^-24, nextafter(1, 0)}', 'samp.z at a Choice threshold x (1 +- 1e-4)',
           'samp.x, samp.y in {0, nextafter(1, 0)}']
S_WEIGHTS = np.array([3.0, 1.0, 3.0, 1.0])
LEAVES = {0b11: 'coat', 0b100: 'diffuse', 0b101: 'spec, dies', 0b1010: 'spec', 0b10111: 'trans-reflect', 0b10110: 'refract'}
BELOW1 = np.nextafter(np.float32(1), np.float32(0))
CHOICES = ('coat', 'spec', 'trans', 'refl')          # Disney.bounce's Choice calls in the order it makes them


def vec(a, T):
    return C.V(*[T(x) for x in a])


def arr(v):
    if isinstance(v, ti.Matrix):
        return [float(e) for e in v.entries]
    return [float(v)] * 3                       # a scalar assigned to a vec3 field broadcasts


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def upper(rng, n):
    v = unit(rng)
    return v if v @ n >= 0 else -v


def at_cos(rng, n, c):
    '''a unit vector whose cosine to n is c'''
    t = np.cross(n, unit(rng))
    t /= np.linalg.norm(t)
    return t * np.sqrt(max(0.0, 1 - c * c)) + n * c


def draw_material(rng, cls):
    p = rng.uniform(0, 1, 14)
    p[13] = rng.uniform(1, 2)
    if 1 <= cls <= 10:
        p[2 + cls] = 0.0
    elif 11 <= cls <= 20:
        p[cls - 8] = 1.0
    elif cls in (M_PLAIN, M_LEAN):
        p[10] = p[12] = 0.0
        if cls == M_LEAN:
            p[7], p[8] = rng.choice([0.0, -0.0], 2)
    elif cls == 23:
        p[:3] = 0.0
    elif cls in (24, 25):
        lum = p[:3] @ [0.3, 0.6, 0.1]
        p[:3] *= EPS * (1 + (1 if cls == 24 else -1) * 10.0 ** rng.uniform(-3, -1)) / lum
    elif cls in (26, 27, 28):
        p[13] = {26: 1.0, 27: 1.0001, 28: 0.8}[cls]
    elif cls in (29, 30, 31):
        p[4] = {29: 0.0, 30: np.sqrt(0.001), 31: 1.0}[cls]
    return p.astype(np.float32)


def draw_directions(rng, cls, ior):
    '''normal, sign, indir, outdir in f32; every relation the class states holds between the ROUNDED values where it says exactly'''
    n = unit(rng).astype(np.float32)
    nd = n.astype(np.float64)
    sign = -1.0 if rng.random() < 0.15 else 1.0
    ind = upper(rng, nd)
    outd = upper(rng, nd)
    if cls == 1:
        ind = at_cos(rng, nd, 10.0 ** rng.uniform(-6, -2))
    elif cls == 2:
        ind = nd
    elif cls == 3:
        ind = nd + 1e-4 * rng.uniform(0.1, 1) * unit(rng)
        ind /= np.linalg.norm(ind)
    elif cls == 4:
        outd = -outd
    elif cls == 5:
        outd = at_cos(rng, nd, 10.0 ** rng.uniform(-6, -2))
    elif cls == 8:
        sign = -1.0
        if ior > 1:                         # sign < 0: eta = ior, total internal reflection from sin = 1 / ior on
            ind = at_cos(rng, nd, np.cos(np.arcsin(1 / ior) + rng.uniform(-1e-3, 1e-3)))
    ind = ind.astype(np.float32)
    if cls in (6, 8):
        i64 = ind.astype(np.float64)
        outd = 2 * (i64 @ nd) * nd - i64
    if cls == 7:
        outd = -ind
    return n, np.float32(sign), ind, outd.astype(np.float32)


class Spy:
    '''which way every Choice went, and against which rate (materials/__init__.py:37-48)'''

    def __init__(self):
        self.trace, self.rates = [], []
        self.orig = MAT.Choice.__call__

    def __enter__(self):
        spy = self

        def call(self, r):
            ret = spy.orig(self, r)
            spy.trace.append(int(ret))
            spy.rates.append(float(r))
            return ret
        MAT.Choice.__call__ = call
        return self

    def __exit__(self, *a):
        MAT.Choice.__call__ = self.orig

    def clear(self):
        del self.trace[:], self.rates[:]

    def word(self):
        return int('1' + ''.join(map(str, self.trace)), 2)

    def thresholds(self):
        '''the rates of the decisions taken, as values of samp.z: Choice maps the interval it is in onto [0, 1) each time'''
        lo, hi, out = 0.0, 1.0, []
        for r, ret in zip(self.rates, self.trace):
            t = lo + r * (hi - lo)
            out.append(t)
            lo, hi = (lo, t) if ret else (t, hi)
        return out


def bounce_of(p, n, sign, ind, samp, T):
    m = DIS.Disney(vec(p[:3], T), *[T(x) for x in p[3:]])
    return m, m.bounce(vec(n, T), T(sign), vec(ind, T), vec(samp, T))


def inputs():
    rng = np.random.default_rng(SEED)
    mc = rng.choice(len(MATERIALS), ROWS, p=M_WEIGHTS / M_WEIGHTS.sum())
    dc = rng.choice(len(DIRECTIONS), ROWS, p=D_WEIGHTS / D_WEIGHTS.sum())
    sc = rng.choice(len(SAMPLES), ROWS, p=S_WEIGHTS / S_WEIGHTS.sum())
    # every class of every axis MIN_ROWS times at least, whatever the draw: the first rows walk through them
    for k in range(MIN_ROWS * len(MATERIALS)):
        mc[k] = k % len(MATERIALS)
    for k in range(MIN_ROWS * len(DIRECTIONS)):
        dc[ROWS - 1 - k] = k % len(DIRECTIONS)
    for k in range(MIN_ROWS * len(SAMPLES)):
        sc[ROWS // 2 + k] = k % len(SAMPLES)
    rows = np.zeros((ROWS, 27), np.float32)
    thr = np.zeros((ROWS, 2), np.int8)       # rows of the threshold class: 1 + the Choice whose threshold samp.z sits at, and the side
    T = np.float64
    ti.set_default_fp(T)
    with Spy() as spy:
        for k in range(ROWS):
            p = draw_material(rng, mc[k])
            n, sign, ind, outd = draw_directions(rng, dc[k], float(p[13]))
            samp = rng.uniform(0, 1, 3).astype(np.float32)
            samp = np.minimum(samp, BELOW1)
            if sc[k] == 1:
                samp[2] = rng.choice([np.float32(0), np.float32(2.0 ** -24), BELOW1])
            elif sc[k] == 3:
                samp[:2] = rng.choice([np.float32(0), BELOW1], 2)
            elif sc[k] == 2:
                spy.clear()
                bounce_of(p, n, sign, ind, samp, T)
                ts = spy.thresholds()
                inner = [t for t in ts if 0 < t < 1]
                t = rng.choice(inner if inner else ts)
                side = rng.choice([-1, 1])
                samp[2] = min(np.float32(t * (1 + side * OFFSET)), BELOW1)
                if inner and (samp[2] > t) == (side > 0):       # a rate of exactly 0 or 1 has no two sides; nor a threshold within 1e-4 of 1, once clipped
                    thr[k] = 1 + ts.index(t), side
            rows[k] = np.concatenate([p, n, [sign], ind, outd, samp])
    return rows, np.column_stack([mc, dc, sc]).astype(np.int8), thr


def evaluate(rows, T):
    ti.set_default_fp(T)
    out, branch = np.zeros((len(rows), 10), T), np.zeros(len(rows), np.int32)
    with Spy() as spy:
        for k, x in enumerate(rows):
            x = x.astype(T)
            spy.clear()
            m, b = bounce_of(x[:14], x[14:17], x[17], x[18:21], x[24:27], T)
            branch[k] = spy.word()
            brdf = m.brdf(vec(x[14:17], T), T(x[17]), vec(x[18:21], T), vec(x[21:24], T))
            out[k] = [*arr(brdf), *arr(b.outdir), float(b.pdf), *arr(b.color)]
    return out, branch


def well_conditioned(o32, o64, b32, b64):
    a, b = o32.astype(np.float64), o64.astype(np.float64)
    same = (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & (a == b))
    with np.errstate(all='ignore'):
        sp = np.where(same, 0.0, 4.0 * np.abs(a - b))
        ok = np.where(np.isfinite(sp), sp, np.inf) <= BASE_REL * np.abs(np.where(np.isfinite(a), a, 0.0)) + BASE_ABS
    return ok.all(axis=1) & (b32 == b64)


def write_npz(dst, arrays):
    '''np.savez_compressed with fixed time stamps: the same arrays give the same bytes'''
    with zipfile.ZipFile(dst, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    rows, cls, thr = inputs()
    o32, b32 = evaluate(rows, np.float32)
    o64, b64 = evaluate(rows, np.float64)
    flagged = b32 != b64
    well = well_conditioned(o32, o64, b32, b64)
    print(f'{ROWS} rows, {int(well.sum())} well-conditioned ({well.mean():.1%}), {int(flagged.sum())} flagged ({flagged.mean():.2%})')
    assert flagged.mean() <= FLAG_CAP, 'move OFFSET, not the cap'
    for axis, names in enumerate((MATERIALS, DIRECTIONS, SAMPLES)):
        for c, name in enumerate(names):
            sel = cls[:, axis] == c
            print(f'  axis {axis} class {c:2d} rows {int(sel.sum()):4d} well-conditioned {int((sel & well).sum()):4d}  {name}')
            assert sel.sum() >= MIN_ROWS and (sel & well).sum() >= MIN_ROWS, name
    for word, name in LEAVES.items():
        sel = (b32 == word) & ~flagged
        print(f'  leaf {name:14s} rows {int(sel.sum()):4d} well-conditioned {int((sel & well).sum()):4d} live {int((sel & (o32[:, 6] != 0)).sum()):4d}')
        assert sel.sum() >= MIN_ROWS and (sel & well).sum() >= MIN_ROWS, name
    assert set(b32) | set(b64) <= set(LEAVES), sorted(set(b32) | set(b64))
    for c, name in enumerate(CHOICES):
        for side in (-1, 1):
            sel = (thr[:, 0] == 1 + c) & (thr[:, 1] == side) & ~flagged
            print(f'  threshold of {name:5s} x (1 {side:+d}e-4): rows {int(sel.sum()):4d} well-conditioned {int((sel & well).sum()):4d}')
            assert sel.sum() >= MIN_ROWS, (name, side)       # decided rows; refractions are rarely well-conditioned, so no such count here
    crit = (cls[:, 1] == 8) & (rows[:, 13] > 1)
    print(f'  critical angle: {int(crit.sum())} rows with ior > 1 (well-conditioned {int((crit & well).sum())}), {int(((cls[:, 1] == 8) & ~crit).sum())} with ior <= 1, which have none')
    assert (crit & well).sum() >= MIN_ROWS
    lean = cls[:, 0] == M_LEAN
    assert (np.signbit(rows[lean, 7]) | np.signbit(rows[lean, 8])).sum() >= MIN_ROWS, 'the lean class needs -0.0 rows'
    out = {'in': rows, 'f32/out': o32, 'f64/out': o64, 'f32/branch': b32, 'f64/branch': b64, 'cls': cls, 'threshold': thr,
           'classes': np.array([f'{axis}:{c}:{t}' for axis, names in zip(('material', 'direction', 'sample'), (MATERIALS, DIRECTIONS, SAMPLES))
                                for c, t in enumerate(names)]),
           'leaves': np.array([f'{w}:{t}' for w, t in LEAVES.items()])}
    dst = os.environ.get('PTINA_GOLDEN_OUT') or os.path.join(HERE, 'reference_disney_cube.npz')
    write_npz(dst, out)
    size, cap = os.path.getsize(dst), os.path.getsize(os.path.join(HERE, 'reference_l1.npz'))
    print('wrote', dst, size, 'bytes (the largest fixture so far, reference_l1.npz:', cap, 'bytes)')
    assert size <= cap


if __name__ == '__main__':
    main()

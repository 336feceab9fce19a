'''
Shared by tests/test_reference_scene_units_cpu.py (the C oracle) and tests/test_reference_scene_units_gpu.py (the HIP device
functions): the fixture tests/golden/reference_scene_units.npz -- vectors computed by the reference's own function bodies on
one small scene state, made by tests/golden/make_reference_scene_units_golden.py -- its scene state as the setters take it,
and ONE set of checks that both files run on their implementation through a small evaluator object:

    ev.light_hit(rows)  ev.light_sample(rows)  ev.image_sample(rows)  ev.world_at(rows)  ev.material_get(rows)
    ev.camera_generate(rows)  ev.face_side(rows)                      -> [n, out columns] arrays

`mode` is 'f64' (the oracle's double build against the f64/ vectors), 'f32' (its float build) / 'strict' (the HIP strict
build) -- the same bounds, both against the f32/ vectors -- or 'fast' (the production build, against f32/ as well).

Bounds.  None is tuned to what an implementation returns:
  f64      relative 1e-12 (absolute 1e-12 where the f32 bound has an absolute part): tests/test_reference_l1_cpu.py's convention;
  f32      the per-function bounds that file holds the same arithmetic to (BOUNDS below names the function each is taken from),
           plus k = 4 x |f32 run - f64 run| of the reference itself per output (helpers.spread) where an input is
           ill-conditioned, and nothing else;
  fast     relative 1e-5 plus the same slack (tests/test_reference_units_gpu.py's convention), with the per-function
           exceptions that file already states for the same instructions (named in BOUNDS).
Discrete outputs -- the hit flag, which light won (its colour), the sampled light (the direction), the mtlid = -1 defaults,
whether the normal was flipped -- must be the reference's exactly.  Informational rows (excluded by an explicit mask with
a stated cap, never by a looser bound): light_sample with samp.z == 1.0, which reads record `count` (sobol.py:20-29 never
produces 1.0), and face_side with |dot(rd, n)| < 1e-6.
'''

import os

import numpy as np

from helpers import close, report, spread

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'reference_scene_units.npz')
LIGHT_STATES = {'five': slice(0, 5), 'one': slice(2, 3), 'none': slice(0, 0)}
TYPE_NAMES = {1: 'POINT', 2: 'AREA'}
MIN_ROWS = 8

# (strict / f32 relative, absolute, production relative, absolute)
BOUNDS = {
    # Sphere.intersect 2e-5 and Area.intersect 2e-5 + 2e-6 in test_reference_l1_cpu.py; production: Sphere 1e-4 (b - sqrt(det)
    # cancels; v_sqrt), Area 5e-5 + 5e-6 in test_reference_units_gpu.py
    'light_hit.dis': (2e-5, 2e-6, 1e-4, 5e-6),
    # pdf = dis^2 / area: held to the bound of dis itself
    'light_hit.pdf': (2e-5, 0.0, 1e-4, 0.0),
    # light_sample: spherical (2e-6 + 5e-7), tanspace / refract grade vector arithmetic (4e-6 + 4e-7), a square root and divisions:
    # test_reference_l1_cpu.py's 4e-6 for every output, its 4e-7 absolute part for the direction; production: the convention's 1e-5
    # (v_rsq / v_rcp in light_sample_one give 1-2 ulp each, inside it).  Ill-conditioned rows (hitpos close to the light) get the
    # reference's own spread and nothing more
    'light_sample.dis': (4e-6, 0.0, 1e-5, 0.0),
    'light_sample.dir': (4e-6, 4e-7, 1e-5, 1e-6),
    'light_sample.pdf': (4e-6, 0.0, 1e-5, 0.0),
    'light_sample.color': (4e-6, 0.0, 1e-5, 0.0),
    # four products of three factors and three additions of positive terms
    'image_sample': (2e-6, 0.0, 1e-5, 0.0),
    # dir2tex 2e-6 + 2e-7 in front of image_sample (the texel gradient amplifies it: spread), one product with fac
    'world_at': (4e-6, 0.0, 1e-5, 0.0),
    # fac x texel (image_sample + one rounding), Disney.__init__'s lerps: tanspace / refract grade, 4e-6 (+ 4e-7)
    'material_get': (4e-6, 4e-7, 1e-5, 1e-6),
    'camera_generate': (4e-6, 4e-7, 1e-5, 1e-6),
    # Face.normal without needle triangles: a weighted sum and a normalisation
    'face_side': (4e-6, 4e-7, 1e-5, 1e-6),
}


def bound(name, mode):
    s_rel, s_abs, f_rel, f_abs = BOUNDS[name]
    if mode == 'f64':
        return 1e-12, (1e-12 if s_abs else 0.0)
    return (f_rel, f_abs) if mode == 'fast' else (s_rel, s_abs)


def tag_of(mode):
    return 'f64' if mode == 'f64' else 'f32'


def slack(gold, key, mode):
    return None if mode == 'f64' else spread(gold, key)


def held(got, want, name, what, mode, sl):
    '''close() at BOUNDS[name] for `mode` plus the slack `sl` (the reference's 4 x f32-vs-f64 spread, or None), after a report line
    that states what the bound is made of: the measured worst error in units of the BASE bound alone, and the largest slack in
    the same units (a figure above 1 in the first with a pass means the spread was needed on that row)'''
    rel, abs_ = bound(name, mode)
    g, w = np.asarray(got, np.float64).reshape(len(got), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    fin = np.isfinite(g) & np.isfinite(w)
    base = np.maximum(rel * np.abs(np.where(fin, w, 0.0)) + abs_, 1e-300)
    err = np.where(fin, np.abs(g - w), 0.0)
    s2 = np.zeros_like(w) if sl is None else np.nan_to_num(np.asarray(sl, np.float64).reshape(w.shape), nan=0.0, posinf=0.0, neginf=0.0)
    report(f'{what}: base bound rel {rel:g} abs {abs_:g}; measured worst error {float((err / base).max()) if err.size else 0.0:.3f} x the base bound; '
           f'largest spread slack {float((np.where(fin, s2, 0.0) / base).max()) if err.size else 0.0:.3f} x the base bound '
           f'(4 x |f32 - f64| of the reference; rows where it exceeds the base bound: {int(((s2 > base) & fin).any(axis=1).sum())} of {len(w)})')
    close(got, want, rel, what, abs_, slack=sl)


def load():
    return np.load(GOLD)


def lights_of(gold, state):
    '''[(world, color, size, type name)] as LightPool.add takes them'''
    s = LIGHT_STATES[state]
    return [(w, c, float(z), TYPE_NAMES[int(t)]) for w, c, z, t in zip(gold['state/light_world'][s], gold['state/light_color'][s],
                                                                       gold['state/light_size'][s], gold['state/light_type'][s])]


def images_of(gold):
    return [gold[f'state/image{k}'] for k in range(4)]


def materials_of(gold):
    '''[[(fac, tex)] * 12] as MaterialPool.load takes them: base colour as three components, the scalars as four'''
    fac, tex = gold['state/material_fac'], gold['state/material_tex']
    return [[((fac[i, k, :3] if k == 0 else fac[i, k]).tolist(), int(tex[i, k])) for k in range(12)] for i in range(fac.shape[0])]


def worlds_of(gold):
    return {'plain': (gold['state/world_fac'][0], -1), 'env': (gold['state/world_fac'][1], 0)}


# ---------------------------------------------------------------------------------------------------- coverage
def check_coverage(gold):
    '''the per-class row counts the generator asserts, again from the fixture'''
    names = {}
    for s in gold['classes']:
        f, c, t = str(s).split(':', 2)
        names.setdefault(f, {})[int(c)] = t
    for tag in ('f32', 'f64'):
        cls = gold[f'{tag}/light_hit/five/cls']
        out = gold[f'{tag}/light_hit/five/out']
        for c in names['light_hit']:
            assert (cls == c).sum() >= MIN_ROWS, f'light_hit: class {c} ({names["light_hit"][c]})'
        colors = gold['state/light_color']
        won = np.array([next((i for i, col in enumerate(colors) if np.array_equal(col, r[3:6])), -1) for r in out])
        for k in range(5):
            assert ((cls == k) & (won == k)).sum() >= MIN_ROWS, f'light {k} is hit first by fewer than {MIN_ROWS} rays'
        assert (won[cls == 6] >= 0).all() and (won[cls == 5] >= 0).all()
        assert (out[cls == 7][:, 0] == 0).all() and (out[cls == 9][:, 0] == 1).all()
        assert 0 < (out[cls == 8][:, 0] == 1).sum() < (cls == 8).sum(), 'grazing rays must fall on both sides'
        for state in ('one', 'none'):
            assert len(gold[f'{tag}/light_hit/{state}/in']) >= MIN_ROWS and len(gold[f'{tag}/light_sample/{state}/in']) >= MIN_ROWS
        assert (gold[f'{tag}/light_hit/none/out'][:, 0] == 0).all()
        one = gold[f'{tag}/light_hit/one/out']
        assert (one[:, 0] == 1).sum() >= MIN_ROWS and (one[:, 0] == 0).sum() >= MIN_ROWS, 'the one-light state needs hits and misses of its light'
        assert (one[one[:, 0] == 1][:, 3:6] == gold['state/light_color'][2]).all()
        cls, rows, out = (gold[f'{tag}/light_sample/five/{k}'] for k in ('cls', 'in', 'out'))
        for c in names['light_sample']:
            assert (cls == c).sum() >= MIN_ROWS, f'light_sample: class {c}'
        bins = np.floor(rows[:, 5] * 5).astype(int)
        for k in range(5):
            assert ((bins == k) & (cls != 3)).sum() >= 4 and np.float32(k / 5) in rows[:, 5].astype(np.float32), f'light_sample: bin {k}'
        assert np.nextafter(np.float32(1), np.float32(0)) in rows[:, 5].astype(np.float32)
        assert (out[cls == 4][:, 5:8] == 0).all() and (out[cls == 0][:, 5:8].max(axis=1) > 0).sum() >= MIN_ROWS
        cls, rows = gold[f'{tag}/image_sample/cls'], gold[f'{tag}/image_sample/in']
        assert rows[:, 1:].min() < -1.4 and rows[:, 1:].max() > 2.4
        for c in names['image_sample']:
            for i in range(4):
                assert ((cls == c) & (rows[:, 0] == i)).sum() >= MIN_ROWS, f'image_sample: class {c}, image {i}'
        for state in ('plain', 'env'):
            cls = gold[f'{tag}/world_at/{state}/cls']
            assert (cls == 0).sum() == 6 and all((cls == c).sum() >= MIN_ROWS for c in (1, 2, 3))
        cls, rows = gold[f'{tag}/material_get/cls'], gold[f'{tag}/material_get/in']
        for c in names['material_get']:
            for m in (0, 1, 2, -1):
                assert ((cls == c) & (rows[:, 0] == m)).sum() >= MIN_ROWS, f'material_get: class {c}, material {m}'
        for k in (0, 1):
            cls = gold[f'{tag}/camera_generate/cam{k}/cls']
            assert all((cls == c).sum() >= MIN_ROWS for c in names['camera_generate'])
        cls = gold[f'{tag}/face_side/cls']
        assert (cls == 0).sum() >= MIN_ROWS and (cls == 1).sum() >= MIN_ROWS and 6 <= (cls == 2).sum() <= 8
    tex = gold['state/material_tex']
    assert (tex[0] == -1).all() and (tex[1] != -1).all() and tex[2, 0] != -1 and (tex[2, 1:] == -1).all()
    assert [gold[f'state/image{k}'].shape[:2] for k in range(4)] == [(32, 16), (5, 7), (1, 4), (4, 1)]
    for k in range(4):
        im = gold[f'state/image{k}']
        assert all(not np.array_equal(im[..., a], im[..., b]) for a in range(4) for b in range(a))
    assert [int(t) for t in gold['state/light_type']] == [2, 1, 2, 1, 2]


# ---------------------------------------------------------------------------------------------------- checks
def check_light_hit(ev, gold, mode, state):
    tag = tag_of(mode)
    key = f'light_hit/{state}'
    rows, want = gold[f'{tag}/{key}/in'], gold[f'{tag}/{key}/out']
    got = ev.light_hit(rows)
    assert np.array_equal(got[:, 0], want[:, 0]), f'{key} [{mode}]: hit flags differ in rows {np.nonzero(got[:, 0] != want[:, 0])[0][:8]}'
    assert np.array_equal(got[:, 3:6], want[:, 3:6].astype(got.dtype)), f'{key} [{mode}]: another light won (colour differs)'
    sl = slack(gold, f'{key}/out', mode)
    for name, col in (('dis', 1), ('pdf', 2)):
        held(got[:, col], want[:, col], f'light_hit.{name}', f'lights_hit {name} [{mode}, {state}]', mode, None if sl is None else sl[:, col])


def check_light_sample(ev, gold, mode, state):
    tag = tag_of(mode)
    key = f'light_sample/{state}'
    rows, want, cls = (gold[f'{tag}/{key}/{k}'] for k in ('in', 'out', 'cls'))
    got = ev.light_sample(rows)
    info = cls == 3
    assert info.sum() <= MIN_ROWS
    report(f'lights_sample [{mode}, {state}]: {int(info.sum())} rows with samp.z == 1.0 (record `count`, informational): '
           f'{int((~np.isclose(got[info], want[info], rtol=1e-4, equal_nan=True)).any(axis=1).sum())} differ from the reference')
    rows, want, got, cls = rows[~info], want[~info], got[~info], cls[~info]
    if state == 'none':
        assert np.array_equal(got, want.astype(got.dtype)), f'{key} [{mode}]: no light must give (inf, 0, 0, 0)'
        return
    # the sampled light is a discrete decision: another index gives an O(1) different direction
    assert (np.abs(got[:, 1:4] - want[:, 1:4]).max(axis=1) <= 1e-3).all(), f'{key} [{mode}]: another light was sampled'
    sl = slack(gold, f'{key}/out', mode)
    for name, cols in (('dis', slice(0, 1)), ('dir', slice(1, 4)), ('pdf', slice(4, 5)), ('color', slice(5, 8))):
        held(got[:, cols], want[:, cols], f'light_sample.{name}', f'lights_sample {name} [{mode}, {state}]', mode,
             None if sl is None else sl[~info][:, cols])
    behind = cls == 4
    if behind.any():
        assert (got[behind][:, 5:8] == 0).all(), f'{key} [{mode}]: behind an AREA light the cosine must clamp the colour to exactly 0'


def check_image_sample(ev, gold, mode):
    tag = tag_of(mode)
    rows, want = gold[f'{tag}/image_sample/in'], gold[f'{tag}/image_sample/out']
    held(ev.image_sample(rows), want, 'image_sample', f'image_sample [{mode}]', mode, slack(gold, 'image_sample/out', mode))


def check_world_at(ev, gold, mode, state):
    tag = tag_of(mode)
    rows, want = gold[f'{tag}/world_at/{state}/in'], gold[f'{tag}/world_at/{state}/out']
    got = ev.world_at(rows)
    if state == 'plain':
        assert np.array_equal(got, want.astype(got.dtype)), f'world_at [{mode}]: tex = -1 must return fac.xyz itself'
        return
    held(got, want, 'world_at', f'world_at [{mode}, {state}]', mode, slack(gold, f'world_at/{state}/out', mode))


def check_material_get(ev, gold, mode):
    tag = tag_of(mode)
    rows, want = gold[f'{tag}/material_get/in'], gold[f'{tag}/material_get/out']
    got = ev.material_get(rows)
    dflt = rows[:, 0] == -1
    assert np.array_equal(got[dflt][:, :14], want[dflt][:, :14].astype(got.dtype)), f'material_get [{mode}]: the twelve defaults of mtlid = -1'
    plain = rows[:, 0] == 0
    assert np.array_equal(got[plain][:, :14], want[plain][:, :14].astype(got.dtype)), f'material_get [{mode}]: an untextured material returns its factors'
    held(got, want, 'material_get', f'material_get [{mode}]', mode, slack(gold, 'material_get/out', mode))


def check_camera_generate(ev, gold, mode, k):
    tag = tag_of(mode)
    rows, want = gold[f'{tag}/camera_generate/cam{k}/in'], gold[f'{tag}/camera_generate/cam{k}/out']
    held(ev.camera_generate(rows), want, 'camera_generate', f'camera_generate [{mode}, camera {k}]', mode, slack(gold, f'camera_generate/cam{k}/out', mode))


def check_face_side(ev, gold, mode):
    tag = tag_of(mode)
    rows, want, cls = (gold[f'{tag}/face_side/{k}'] for k in ('in', 'out', 'cls'))
    got = ev.face_side(rows)
    info = cls == 2
    assert info.sum() <= MIN_ROWS
    report(f'face_side [{mode}]: {int(info.sum())} rows with |dot(rd, n)| < 1e-6 (informational): {int((got[info, 3] != (want[info, 3] < 0)).sum())} flipped the other way')
    got, want = got[~info], want[~info]
    assert np.array_equal(got[:, 3], (want[:, 3] < 0).astype(got.dtype)), f'face_side [{mode}]: the normal is flipped exactly when -dot(rd, n) < 0'
    sl = slack(gold, 'face_side/out', mode)
    held(got[:, :3], want[:, :3], 'face_side', f'face_side normal [{mode}]', mode, None if sl is None else sl[~info][:, :3])

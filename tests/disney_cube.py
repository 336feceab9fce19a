'''
Shared by tests/test_reference_disney_cube_cpu.py (the C oracle) and tests/test_reference_disney_cube_gpu.py (the HIP device functions of
both builds): the fixture tests/golden/reference_disney_cube.npz -- Disney.brdf and Disney.bounce evaluated by the reference's own
function bodies over the whole parameter cube, row classes on three axes (materials, directions, samples), made by
tests/golden/make_reference_disney_cube_golden.py -- and ONE set of checks that both files run on what their implementation returns:

    check(got_brdf [n, 3], got_bounce [n, 7], gold, mode, what)

`mode` is 'f64' (the oracle's double build against the f64 vectors), 'f32' (its float build) / 'strict' (the HIP strict build) --
the same bounds, both against the f32 vectors -- or 'fast' (the production build, against the f32 vectors as well).

Bounds.  None is tuned to what an implementation returns on these rows:
  f64            relative 1e-10 + absolute 1e-13 on every output (Disney.brdf's in tests/test_reference_l1_cpu.py)
  f32 / strict   relative 5e-5 + absolute 2e-6 on every output (the same test's f32 bound: the BASE bound of the fixture)
  fast           brdf relative 3e-5 + absolute 2e-6; bounce 1.1e-5 in the metric |got - want| / (|want| + 1e-3) -- what
                 tests/test_reference_units_gpu.py states for the two functions on reference_l1.npz
A row is FLAGGED when the reference's f32 and f64 runs took different Choice branches: it is kept, counted (at most FLAG_CAP of
the rows) and left out of the value comparisons.  A row is WELL-CONDITIONED when it is not flagged and 4 x |f32 run - f64 run| of
the reference (helpers.spread) is below the base bound on every one of its ten outputs; such a row is held to the mode's bound
alone, every other unflagged row to the bound plus that spread (f64: no slack at all).  The fixture's coverage is asserted with
the f32 base bound (873 rows); the production build's bounds are tighter than that, so for it the same rule is applied with ITS
base bound (760 rows): a row whose spread, 4 x the difference of the reference's own two runs, exceeds the bound it is held to is
not well-conditioned for that bound, whatever it is for a looser one.  (On 9 of the 113 rows between the two counts that
difference itself, without the 4, is above the production bound: the f32 vector the build is compared with is no nearer to the
exact value than that.  Holding all 873 to the production bound alone leaves 13 rows outside after the exceptions below.)
The production build has stated exceptions on top (production_exceptions): seven conditioning classes computed from the inputs,
each the cost of approximate instructions in front of a cancellation, each at 1.3 x what was measured against these vectors, each
factor with a floor, so that no term adds more than ALLOW_REL (relative) or ALLOW_DIR (direction) to a bound -- asserted, and what
each term allows is reported row count by row count.
Discrete outcomes must be the reference's exactly on every unflagged row: which rows are dead (outdir == 0), where a value is
NaN or infinite, and the branch -- read through the outgoing direction, which another lobe moves by O(1).
'''

import os

import numpy as np

from helpers import report, spread

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'reference_disney_cube.npz')
MIN_ROWS = 8
FLAG_CAP = 0.01
BASE = (5e-5, 2e-6)
M_PLAIN, M_LEAN = 21, 22          # material classes: the plain mask, the lean rule
AXES = ('material', 'direction', 'sample')
CHOICES = ('coat', 'spec', 'trans', 'refl')       # Disney.bounce's Choice calls in the order it makes them: the bits of a branch word
BRDF, BOUNCE, DIR = slice(0, 3), slice(3, 10), slice(3, 6)


def load():
    return np.load(GOLD)


def rows_brdf(gold):
    '''MPT_UNIT_DISNEY_BRDF's 24 columns: 14 parameters, normal, sign, indir, outdir'''
    return np.ascontiguousarray(gold['in'][:, :24])


def rows_bounce(gold):
    '''MPT_UNIT_DISNEY_BOUNCE's 24 columns: 14 parameters, normal, sign, indir, samp'''
    x = gold['in']
    return np.ascontiguousarray(np.column_stack([x[:, :21], x[:, 24:27]]))


def class_names(gold):
    names = {a: {} for a in AXES}
    for s in gold['classes']:
        a, c, t = str(s).split(':', 2)
        names[a][int(c)] = t
    return names


def leaf_names(gold):
    return {int(str(s).split(':', 1)[0]): str(s).split(':', 1)[1] for s in gold['leaves']}


def flagged(gold):
    return gold['f32/branch'] != gold['f64/branch']


def _spread(gold):
    '''helpers.spread with a non-finite value equal to the same non-finite value counted as no spread, any other as infinite'''
    a, b = gold['f32/out'].astype(np.float64), gold['f64/out']
    same = (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & (a == b))
    with np.errstate(all='ignore'):
        sp = np.where(same, 0.0, spread(gold, 'out'))
    return np.where(np.isfinite(sp), sp, np.inf)


def well_conditioned(gold, rel=None, abs_=None):
    '''rows whose spread is below the base bound on every output.  rel, abs_ (scalars or [n, 10] arrays): the base bound the rows
    are to be held to; default the fixture's own, BASE, which is what the generator asserts its coverage with'''
    a = gold['f32/out'].astype(np.float64)
    rel, abs_ = (BASE[0] if rel is None else rel), (BASE[1] if abs_ is None else abs_)
    base = rel * np.abs(np.where(np.isfinite(a), a, 0.0)) + abs_
    return (_spread(gold) <= base).all(axis=1) & ~flagged(gold)


def check_coverage(gold):
    '''what the generator asserts, again from the file: every class of every axis and every leaf of the Choice tree with MIN_ROWS
    rows, MIN_ROWS of them well-conditioned; at most FLAG_CAP of the rows flagged; a critical angle on MIN_ROWS well-conditioned rows of
    its class; every Choice call's threshold from either side on MIN_ROWS unflagged rows'''
    cls, fl, well = gold['cls'], flagged(gold), well_conditioned(gold)
    n = len(cls)
    assert gold['in'].dtype == np.float32 and gold['f32/out'].dtype == np.float32 and gold['f64/out'].dtype == np.float64
    assert gold['in'].shape == (n, 27) and gold['f32/out'].shape == (n, 10) and gold['f64/out'].shape == (n, 10)
    report(f'disney cube: {n} rows, {int(well.sum())} well-conditioned ({well.mean():.1%}), {int(fl.sum())} flagged ({fl.mean():.2%}, cap {FLAG_CAP:.0%})')
    assert fl.mean() <= FLAG_CAP
    names = class_names(gold)
    assert [len(names[a]) for a in AXES] == [32, 9, 4]
    for k, a in enumerate(AXES):
        for c, t in sorted(names[a].items()):
            sel = cls[:, k] == c
            report(f'disney cube: {a} class {c} ({t}): {int(sel.sum())} rows, {int((sel & well).sum())} well-conditioned, {int((sel & fl).sum())} flagged')
            assert sel.sum() >= MIN_ROWS and (sel & well).sum() >= MIN_ROWS, f'{a} class {c} ({t})'
    leaves = leaf_names(gold)
    assert sorted(leaves.values()) == sorted(['coat', 'diffuse', 'spec, dies', 'spec', 'trans-reflect', 'refract'])
    assert set(gold['f32/branch']) | set(gold['f64/branch']) <= set(leaves)
    for w, t in leaves.items():
        sel = (gold['f32/branch'] == w) & ~fl
        report(f'disney cube: leaf {t}: {int(sel.sum())} rows, {int((sel & well).sum())} well-conditioned')
        assert sel.sum() >= MIN_ROWS and (sel & well).sum() >= MIN_ROWS, f'leaf {t}'
    # the classes are what they say (the values a kernel takes another path on)
    x = gold['in']
    m = cls[:, 0]
    for c in range(1, 11):
        assert (x[m == c, 2 + c] == 0).all() and (x[m == 10 + c, 2 + c] == 1).all()
    assert (x[np.isin(m, [M_PLAIN, M_LEAN])][:, [10, 12]] == 0).all() and (x[m == M_LEAN][:, [7, 8]] == 0).all()
    assert (np.signbit(x[m == M_LEAN, 7]) | np.signbit(x[m == M_LEAN, 8])).sum() >= MIN_ROWS, 'the lean class holds -0.0 rows'
    lum = x[:, :3].astype(np.float64) @ [0.3, 0.6, 0.1]
    assert (x[m == 23, :3] == 0).all() and (lum[m == 24] > 1e-6).all() and (lum[m == 24] < 1.2e-6).all()
    assert (lum[m == 25] < 1e-6).all() and (lum[m == 25] > 0.8e-6).all()
    assert (x[m == 26, 13] == 1).all() and (x[m == 27, 13] == np.float32(1.0001)).all() and (x[m == 28, 13] == np.float32(0.8)).all()
    assert (x[m == 29, 4] == 0).all() and (x[m == 30, 4] == np.float32(np.sqrt(0.001))).all() and (x[m == 31, 4] == 1).all()
    d = cls[:, 1]
    nrm, ind, outd = x[:, 14:17].astype(np.float64), x[:, 18:21].astype(np.float64), x[:, 21:24].astype(np.float64)
    cosi, coso = (nrm * ind).sum(axis=1), (nrm * outd).sum(axis=1)
    assert (cosi[d == 1] > 0).all() and (cosi[d == 1] < 1.1e-2).all()
    assert (x[d == 2, 14:17] == x[d == 2, 18:21]).all()
    assert (np.abs(ind - nrm)[d == 3].max(axis=1) <= 1.1e-4).all() and (x[d == 3, 14:17] != x[d == 3, 18:21]).any(axis=1).all()
    assert (coso[d == 4] < 0).all() and (np.abs(coso[d == 5]) < 1.1e-2).all()
    assert (np.abs(2 * cosi[:, None] * nrm - ind - outd)[np.isin(d, [6, 8])] <= 2e-7).all()
    assert (x[d == 7, 21:24] == -x[d == 7, 18:21]).all() and (x[d == 8, 17] == -1).all()
    assert ((x[:, 17] == -1) & (d != 8)).sum() >= MIN_ROWS and set(x[:, 17]) == {-1.0, 1.0}
    s = cls[:, 2]
    below1 = np.nextafter(np.float32(1), np.float32(0))
    assert set(x[s == 1, 26]) == {np.float32(0), np.float32(2.0 ** -24), below1}
    assert np.isin(x[s == 3, 24:26], [0, below1]).all() and len({tuple(r) for r in x[s == 3, 24:26]}) == 4
    assert (x[:, 24:27] < 1).all() and (x[:, 24:27] >= 0).all()
    # the critical-angle class has one where ior > 1 (sign = -1: total internal reflection from sin = 1 / ior on); a row with ior <= 1 has
    # none and keeps a general incidence
    ior = x[:, 13].astype(np.float64)
    crit = (d == 8) & (ior > 1)
    angle = np.arccos(np.clip(cosi, -1, 1)) - np.arcsin(1 / np.maximum(ior, 1))
    report(f'disney cube: critical angle: {int(crit.sum())} rows with ior > 1 ({int((crit & well).sum())} well-conditioned), incidence within '
           f'{np.abs(angle[crit]).max():.2e} of it; {int(((d == 8) & ~crit).sum())} rows with ior <= 1 have none')
    assert (np.abs(angle[crit]) <= 1.01e-3).all() and (crit & well).sum() >= MIN_ROWS
    # the threshold class: each of the four Choice calls' thresholds from either side, and samp.z decides that call the way its side says
    thr = gold['threshold']
    assert ((thr[:, 0] != 0) <= (s == 2)).all() and (thr[s == 2, 0] != 0).mean() > 0.9
    for c, name in enumerate(CHOICES):
        for side in (-1, 1):
            sel = (thr[:, 0] == 1 + c) & (thr[:, 1] == side) & ~fl
            report(f'disney cube: samp.z at the threshold of the {name} Choice x (1 {side:+d}e-4): {int(sel.sum())} rows, {int((sel & well).sum())} well-conditioned')
            assert sel.sum() >= MIN_ROWS, (name, side)
            took = np.array([int(bin(int(w))[3:][c]) for w in gold['f64/branch'][sel]])       # the call's bit under the leading 1
            assert (took == (side < 0)).all(), f'{name}, side {side}: samp.z does not decide the call'


def admitted(gold, variant):
    '''the test's own admission rule, per row: 'plain' -- clearcoat and transmission exactly zero (-0.0 is zero), what
    shade_feat_material leaves without its CLEARCOAT and TRANSMISSION bits; 'lean' -- sheen and subsurface exactly zero as well
    (shade_lean_material).  tests/test_reference_disney_cube_cpu.py holds the rule to the header's functions on every row.'''
    x = gold['in']
    plain = (x[:, 10] == 0) & (x[:, 12] == 0)
    return plain if variant == 'plain' else plain & (x[:, 7] == 0) & (x[:, 8] == 0)


def material_tables(gold):
    '''fac [n][12][4] of the rows' materials as mpt_load_materials receives them (shade_feat.h: parameter k's factor in fac[k][0],
    the base colour in fac[0][0..2]; untextured)'''
    x = gold['in']
    fac = np.zeros((len(x), 12, 4), np.float32)
    fac[:, 0, :3] = x[:, :3]
    fac[:, 1:, 0] = x[:, 3:14]
    return fac


def _bounds(mode):
    '''(relative, absolute) for the brdf columns and for the bounce columns'''
    if mode == 'f64':
        return (1e-10, 1e-13), (1e-10, 1e-13)
    if mode == 'fast':
        return (3e-5, 2e-6), (1.1e-5, 1.1e-5 * 1e-3)       # |err| / (|want| + 1e-3) <= 1.1e-5, written as rel + abs
    return BASE, BASE


def _rows(got_brdf, got_bounce, gold, mode, what):
    want = gold['f64/out' if mode == 'f64' else 'f32/out'].astype(np.float64)
    got = np.column_stack([np.asarray(got_brdf, np.float64), np.asarray(got_bounce, np.float64)])
    assert got.shape == want.shape, what
    return got, want


def check(got_brdf, got_bounce, gold, mode, what):
    '''the discrete and the value checks of the module docstring'''
    check_discrete(got_brdf, got_bounce, gold, mode, what)
    return check_values(got_brdf, got_bounce, gold, mode, what)


def check_discrete(got_brdf, got_bounce, gold, mode, what):
    '''on every unflagged row, exactly the reference's: the NaN / infinity pattern, which samples are dead, and the lobe sampled'''
    got, want = _rows(got_brdf, got_bounce, gold, mode, what)
    cls, use = gold['cls'], ~flagged(gold)
    # ---- discrete outcomes, exactly, on every unflagged row
    for name, g, w in (('NaN', np.isnan(got), np.isnan(want)), ('infinity', np.isinf(got), np.isinf(want))):
        bad = np.flatnonzero((g != w).any(axis=1) & use)
        assert bad.size == 0, f'{what}: the {name} pattern differs in {bad.size} rows, first {bad[:8]}'
    inf = np.isinf(want)
    assert (got[inf & use[:, None]] == want[inf & use[:, None]]).all(), f'{what}: an infinity has the other sign'
    dead_g, dead_w = (got[:, DIR] == 0).all(axis=1), (want[:, DIR] == 0).all(axis=1)
    bad = np.flatnonzero((dead_g != dead_w) & use)
    assert bad.size == 0, f'{what}: {bad.size} samples die in one implementation only, first rows {bad[:8]}, classes {cls[bad[:8]].tolist()}'
    assert (got[dead_w & use][:, BOUNCE] == 0).all(), f'{what}: a dead sample carries a pdf or a colour'
    sp = np.zeros_like(want) if mode == 'f64' else _spread(gold)
    sp_fin = np.where(np.isfinite(sp), sp, 0.0)
    live = use & ~dead_w
    ddir = np.abs(got[:, DIR] - want[:, DIR])
    off = (ddir > 1e-3 + sp_fin[:, DIR]).any(axis=1) & live
    assert not off.any(), f'{what}: another lobe was sampled in rows {np.flatnonzero(off)[:8]} (direction off by {ddir[off].max():.2e})'
    report(f'{what}: NaN / infinity pattern, dead samples ({int((dead_w & use).sum())}) and lobes ({int(live.sum())} live samples) are the reference\'s on all {int(use.sum())} unflagged rows')


SPEC, TRANS_REFLECT, REFRACT, DIFFUSE = 0b1010, 0b10111, 0b10110, 0b100       # branch words of the live leaves
D_GRAZING = 1                                                                 # direction class: cosi in [1e-6, 1e-2]
T_CLASS, S_CLASS = 0.04, 0.01


def production_exceptions(gold):
    '''The stated exceptions of the production build: conditioning classes computed from the fixture's INPUTS (and, for the cosine of
    the sampled direction, from the reference's f64 output) in double precision -- never from what the kernel returns -- each with the
    columns it touches, the factor a cancellation multiplies an input error by, the reason, and a constant K = 1.3 x the value
    MEASURED on an MI355X against the reference's vectors, written beside it.  A term adds K x factor (x |want| for a relative one) to
    the bound of its rows and columns, on top of the mode's bound and the row's spread; a row outside its class gets nothing.

    The production build enters every one of these cancellations with a few ulp more than the reference's f32 run does (v_rcp,
    v_rsq and v_sqrt at 1 ulp each where the reference divides and takes roots correctly rounded; v_sin / v_cos at 1e-6 absolute in
    spherical(); FMA contraction), so 4 x |f32 - f64| of the reference does not cover what the cancellation makes of them:
      t    GTR2's  t = 1 + (alpha^2 - 1) cosh^2  (and GTR1's, with clearcoatAlpha, where clearcoat != 0): D = alpha^2 / (pi t^2), an
           error d of cosh^2 is 2 d / t in D.  Class t < 0.04: there 2 x 4 ulp / t reaches the 1.1e-5 of the bound.
      s2   spherical()'s sqrt(1 - h^2) behind sample_GTR2's h:  s2 = 1 - h^2 = u alpha^2 / (1 - u (1 - alpha^2)); an error d of h^2 is
           d / (2 sqrt(s2)) in the two tangential components of the direction, and through cosoh and coso in the colour.  Class
           0 < s2 < 0.01: there 1 ulp / (2 x 0.1) reaches the direction's bound.  (u == 0 gives s2 == 0 exactly, in the kernel as
           well: nothing is amplified, and those rows get no term.)
      grazing incidence, cosi <= 1e-2 (the fixture's direction class): Choice's pdf *= 1 - specrate with specrate = 1 - O(cosi) -- Fi =
           (1 - cosi)^5 -- is an ulp / cosi in the diffuse lobe's colour; reflect(-indir, h) = 2 (i.h) h - i cancels in the specular
           lobes, an absolute error in the direction and, through coso, 1 / |coso| in the colour.
    Every factor has a floor (T_FLOOR, S_FLOOR, C_FLOOR below, with their reasons) and so a largest value, which the table states.'''
    x = gold['in'].astype(np.float64)
    br, cls = gold['f32/branch'], gold['cls']
    nrm, ind, outd = x[:, 14:17], x[:, 18:21], x[:, 21:24]
    a2 = np.maximum(0.001, x[:, 4] ** 2) ** 2
    h = ind + outd
    h = h / np.maximum(np.linalg.norm(h, axis=1, keepdims=True), 1e-300)
    ch2 = np.maximum(0.0, (h * nrm).sum(axis=1)) ** 2
    ac2 = (0.1 * (1 - x[:, 11]) + 0.001 * x[:, 11]) ** 2
    t_brdf = np.where(x[:, 10] != 0, np.minimum(1 + (a2 - 1) * ch2, 1 + (ac2 - 1) * ch2), 1 + (a2 - 1) * ch2)
    u = x[:, 24]
    hz2 = (1 - u) / (1 - u * (1 - a2))
    t_bounce, s2 = 1 + (a2 - 1) * hz2, 1 - hz2
    ggx = np.isin(br, [SPEC, TRANS_REFLECT, REFRACT])
    cosi = (nrm * ind).sum(axis=1)
    coso = np.abs((gold['f64/out'][:, DIR] * nrm).sum(axis=1))       # a refraction leaves below the surface: |coso|
    grazing = cls[:, 1] == D_GRAZING
    # s2 == 0 exactly (samp.x == 0: h is the normal, the kernel's sqrt(1 - h^2) is exactly 0 as well) amplifies nothing: not in the class
    small_s2 = ggx & (s2 > 0) & (s2 < S_CLASS)
    # (name, rows, columns, relative?, factor, the largest factor the class admits, K, measured, reason)
    return [
        ('brdf, t < 0.04', t_brdf < T_CLASS, BRDF, True, 1 / np.maximum(t_brdf, T_FLOOR), 1 / T_FLOOR, K_BRDF_T, M_BRDF_T, 'GTR2 / GTR1: 2 d / t'),
        ('bounce pdf, t < 0.04', ggx & (t_bounce < T_CLASS), slice(6, 7), True, 1 / np.maximum(t_bounce, T_FLOOR), 1 / T_FLOOR, K_PDF_T, M_PDF_T, 'GTR2: 2 d / t'),
        ('bounce direction, s2 < 0.01', small_s2, DIR, False, 1 / np.sqrt(np.maximum(s2, S_FLOOR)), S_FLOOR ** -0.5, K_DIR_S, M_DIR_S, 'sqrt(1 - h^2): d / (2 sqrt(s2))'),
        ('bounce colour, s2 < 0.01', small_s2, slice(7, 10), True, 1 / np.sqrt(np.maximum(s2, S_FLOOR)), S_FLOOR ** -0.5, K_COL_S, M_COL_S, 'the same through cosoh, coso'),
        ('diffuse colour, grazing', grazing & (br == DIFFUSE), slice(7, 10), True, 1 / np.maximum(cosi, C_FLOOR), 1 / C_FLOOR, K_COL_G, M_COL_G, '1 - specrate: ulp / cosi'),
        ('specular direction, grazing', grazing & ggx, DIR, False, np.ones(len(x)), 1.0, K_DIR_G, M_DIR_G, 'reflect(-indir, h) cancels'),
        ('specular colour, grazing', grazing & ggx, slice(7, 10), True, 1 / np.maximum(coso, C_FLOOR), 1 / C_FLOOR, K_COL_R, M_COL_R, 'the same through |coso|'),
    ]


# Floors of the factors, none from what a kernel returns: below them the cancellation no longer grows as 1 / x, and no exception may.
#   T_FLOOR  t >= alpha^2 >= 0.001^2, the clamp of alpha in Disney.__init__ (clearcoatAlpha >= 0.001 likewise): the least t there is
#   S_FLOOR  h^2 is a float near 1 and carries an error d of about an ulp of 1, 2^-23 = 1.2e-7: where s2 < d the root is off by
#            sqrt(d) at most, not by d / (2 sqrt(s2))
#   C_FLOOR  the least cosine the grazing class draws, 1e-6; a sampled |coso| below it is smaller than the direction's own error
# ALLOW_REL / ALLOW_DIR: what K x factor may reach at most, asserted for every term: a relative allowance stays below 1 (a lobe weight
# that is missing or doubled fails on every row), the direction's below the 1e-3 of the lobe check.
T_FLOOR, S_FLOOR, C_FLOOR = 1e-6, 1e-7, 1e-6
ALLOW_REL, ALLOW_DIR = 1.0, 1e-3

# measured (MI355X; the largest excess over the mode's bound + spread in the class, divided by the factor) and K = 1.3 x measured
M_BRDF_T, M_PDF_T, M_DIR_S, M_COL_S, M_COL_G, M_DIR_G, M_COL_R = 3.49e-7, 5.21e-7, 9.88e-8, 4.09e-7, 1.24e-8, 2.79e-7, 3.15e-7
K_BRDF_T, K_PDF_T, K_DIR_S, K_COL_S, K_COL_G, K_DIR_G, K_COL_R = (1.3 * m for m in (M_BRDF_T, M_PDF_T, M_DIR_S, M_COL_S, M_COL_G, M_DIR_G, M_COL_R))


def check_values(got_brdf, got_bounce, gold, mode, what):
    '''every unflagged row within the mode's bound (module docstring), a well-conditioned row within the bound alone; the production
    build ('fast') with the terms of production_exceptions on top, each reported with what it measures now.  Prints the worst error
    per class in units of the base bound; returns the worst error per row in units of the bound that row was held to.'''
    got, want = _rows(got_brdf, got_bounce, gold, mode, what)
    cls, fl = gold['cls'], flagged(gold)
    use = ~fl
    sp = np.zeros_like(want) if mode == 'f64' else _spread(gold)
    sp_fin = np.where(np.isfinite(sp), sp, 0.0)
    fin = np.isfinite(want) & np.isfinite(got)
    (rb, ab), (rs, as_) = _bounds(mode)
    rel = np.concatenate([np.full(3, rb), np.full(7, rs)])[None, :].repeat(len(want), axis=0)
    abs_ = np.concatenate([np.full(3, ab), np.full(7, as_)])[None, :].repeat(len(want), axis=0)
    # a row is well-conditioned FOR THE BOUND IT IS HELD TO: the production bounds are tighter than the fixture's base bound, and a row
    # whose reference runs differ by more than the bound cannot be held to it without that spread
    well = well_conditioned(gold, rel, abs_) if mode == 'fast' else well_conditioned(gold)
    base = rel * np.abs(np.where(fin, want, 0.0)) + abs_
    err = np.where(fin, np.abs(got - want), 0.0)
    bound = base + np.where(well[:, None], 0.0, sp_fin)
    if mode == 'fast':
        # the coverage the generator asserts with the base bound holds with the tighter one as well
        assert min(int(((cls[:, k] == c) & well).sum()) for k in range(3) for c in set(cls[:, k])) >= MIN_ROWS
        assert min(int(((gold['f32/branch'] == b) & well).sum()) for b in set(gold['f32/branch'])) >= MIN_ROWS
        report(f'{what}: {int(well.sum())} rows are well-conditioned for the production bounds ({int(well_conditioned(gold).sum())} for the base bound)')
        extra = np.zeros_like(bound)
        live = use & ~(want[:, DIR] == 0).all(axis=1)
        for name, rows, cols, relative, factor, cap, K, measured, reason in production_exceptions(gold):
            rows = rows & use
            allow = K * factor[rows & (live if cols != BRDF else use)]            # per row: what the term adds, relative (or absolute: direction)
            assert (factor[rows] <= cap).all() and K * cap <= (ALLOW_REL if relative else ALLOW_DIR), f'exception "{name}" is not bounded: K x factor up to {K * cap:.3g}'
            report(f'{what}: exception "{name}" allows K x factor up to {allow.max() if allow.size else 0.0:.3g} (at most {K * cap:.3g}) on {allow.size} live rows: '
                   f'above 1e-4 on {int((allow > 1e-4).sum())}, above 1e-3 on {int((allow > 1e-3).sum())}, above 1e-2 on {int((allow > 1e-2).sum())}, above 1e-1 on {int((allow > 1e-1).sum())}')
            scale = np.abs(np.where(fin, want, 0.0))[:, cols] if relative else np.ones_like(want[:, cols])
            excess = np.where(rows[:, None], np.maximum(err[:, cols] - bound[:, cols], 0.0) / np.maximum(scale * factor[:, None], 1e-300), 0.0)
            excess = np.where(scale > 0, excess, 0.0)
            extra[:, cols] += np.where(rows[:, None], K * factor[:, None] * scale, 0.0)
            report(f'{what}: exception "{name}" ({reason}): {int(rows.sum())} rows, K = {K:.3g} = 1.3 x {measured:.3g}; measured now {excess.max():.3g}')
        bound = bound + extra
    ratio = np.where(use[:, None], err / bound, 0.0)
    in_base = np.where(use[:, None], err / base, 0.0)
    names = class_names(gold)
    for k, a in enumerate(AXES):
        for c, t in sorted(names[a].items()):
            sel = cls[:, k] == c
            report(f'{what}: {a} class {c} ({t}): worst error {in_base[sel & well].max():.3f} x the base bound on {int((sel & well).sum())} '
                   f'well-conditioned rows (brdf {in_base[sel & well][:, BRDF].max():.3f}, bounce {in_base[sel & well][:, BOUNCE].max():.3f}), '
                   f'{in_base[sel & use & ~well].max() if (sel & use & ~well).any() else 0.0:.3f} x on the {int((sel & use & ~well).sum())} others '
                   f'({ratio[sel & use & ~well].max() if (sel & use & ~well).any() else 0.0:.3f} x the bound with their spread)')
    leaves = leaf_names(gold)
    for w, t in leaves.items():
        sel = (gold['f32/branch'] == w) & well
        report(f'{what}: leaf {t}: worst error {in_base[sel].max():.3f} x the base bound on {int(sel.sum())} well-conditioned rows')
    row_bad = np.flatnonzero((ratio > 1.0).any(axis=1))
    worst = int(np.argmax(ratio.max(axis=1)))
    report(f'{what}: worst error {ratio.max():.3f} x the bound (row {worst}, classes {cls[worst].tolist()}, column {int(np.argmax(ratio[worst]))}, '
           f'well-conditioned {bool(well[worst])}); rows outside {row_bad.size} of {int(use.sum())}')
    assert row_bad.size == 0, (f'{what}: {row_bad.size} rows outside the bound, worst {ratio.max():.2f} x in row {worst} (classes {cls[worst].tolist()}, '
                               f'column {int(np.argmax(ratio[worst]))}, well-conditioned {bool(well[worst])}): got {got[worst]}, want {want[worst]}; '
                               f'first rows {row_bad[:8]}')
    return ratio.max(axis=1)

'''
GPU (-m gpu): the HIP Disney.brdf and Disney.bounce of BOTH builds (pt_device.h disney_brdf / disney_bounce through mpt_unit_eval's
kinds 'disney_brdf' / 'disney_bounce') held to tests/golden/reference_disney_cube.npz -- the reference's own function bodies over the
whole parameter cube (tests/golden/make_reference_disney_cube_golden.py) -- by the checks of tests/disney_cube.py, which states the
bounds: the strict build at the f32 bounds the C oracle is held to, the production build at the bounds
tests/test_reference_units_gpu.py states for the two functions, well-conditioned rows at the bound alone, the others with the
reference's own f32-vs-f64 spread on top, and seven stated exceptions (conditioning classes, each at 1.3 x its measured value, each
with a floor under its factor and an asserted limit on what it may add);
dead / alive, NaN / infinity and the lobe exactly.

And the two other instantiations of the production build at function level: kinds 'disney_brdf_plain' / 'disney_bounce_plain'
(disney_brdf<MPT_FEAT_PLAIN, false>) and '..._lean' (<MPT_FEAT_PLAIN, true>) must return the generic kind's output WORD FOR WORD on every
row their mask admits -- the plain class and the lean class of the fixture, -0.0 rows included -- with one licence, +0 against -0,
which the comments in pt_device.h claim and a film cannot see; its count is reported.  (That the admission rule used here is the
host's -- shade_feat.h -- is tests/test_reference_disney_cube_cpu.py's part: it needs a C compiler and no GPU.)
'''

import numpy as np
import pytest

import disney_cube as dc
from helpers import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return dc.load()


def context(mode):
    from ptina_amd import _lib
    from ptina_amd.things import init_things
    from ptina_amd.common import ctx
    init_things()
    ctx().set_option('mode', _lib.MODE_STRICT if mode == 'strict' else _lib.MODE_FAST)
    return ctx()


@pytest.fixture(scope='module')
def evaluated(gold):
    """both builds' disney_brdf and disney_bounce on the fixture's rows, evaluated once for the tests below"""
    from ptina_amd.common import reset_all
    out = {}
    for mode in ('strict', 'fast'):
        reset_all()
        c = context(mode)
        out[mode] = (c.unit_eval('disney_brdf', dc.rows_brdf(gold)), c.unit_eval('disney_bounce', dc.rows_bounce(gold)))
    reset_all()
    return out


@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_discrete_outcomes_over_the_cube(gold, evaluated, mode):
    """NaN / infinity pattern, dead samples and the lobe sampled are the reference's on every unflagged row, in both builds.

    (What this found in the production build: row 318 -- luminance just above eps, cosi 1.6e-2, samp.z the last float below 1 -- came
    back alive from the DIFFUSE lobe with an infinite colour where the reference's sample dies in the specular lobe.  Behind the
    clearcoat Choice w = (w - r) * v_rcp(1 - r) rounded up to exactly 1.0, "1 < specrate = 1" failed, and pdf *= 1 - 1 divided the
    colour by zero.  Choice now takes a rate of 1 always -- pt_device.h.)"""
    dc.check_discrete(*evaluated[mode], gold, mode, f'Disney cube [{mode}]')


def test_strict_build_values_over_the_cube(gold, evaluated):
    dc.check_values(*evaluated['strict'], gold, 'strict', 'Disney cube [strict]')


def test_production_build_values_over_the_cube(gold, evaluated):
    """The production build at the bounds tests/test_reference_units_gpu.py states for the two functions on reference_l1.npz (brdf
    relative 3e-5 + absolute 2e-6; bounce 1.1e-5 in |got - want| / (|want| + 1e-3)), a row that is well-conditioned for those bounds at
    the bound alone, every other row with the reference's own 4 x |f32 - f64| on top -- and the seven stated exceptions of
    disney_cube.production_exceptions, which names for each the cancellation, the class (computed from the inputs), the factor, the
    value measured and K = 1.3 x it.  No term is unbounded: each factor has a floor, K x factor stays below 1 relative (0.68 at
    most, the pdf at roughness 0) and below 1e-3 on the direction, which is asserted, and the report says on how many rows each term
    allows more than 1e-4, 1e-3, 1e-2 and 1e-1.  A row with samp.x == 0 (s2 == 0 exactly) gets no s2 term at all.

    Without the exceptions 50 of the 1200 rows are outside (MI355X), worst 45.8 x the bound: row 203, the pdf of a refraction at
    roughness 0.099, GTR2's t = 1.06e-3, relative error 5.0e-4.  Traced, row by row:
      * 43 rows have GTR2's t = 1 + (alpha^2 - 1) cosh^2 below 0.04 in the function that fails, or sample_GTR2's s2 = 1 - h^2 below 0.01
        behind it: pdf and brdf off by up to 5.2e-7 / t (cosh^2 carries up to 4 ulp: v_rsq / v_rcp / v_sqrt at 1 ulp each where the
        reference divides and takes roots correctly rounded, v_sin / v_cos at 1e-6 absolute in spherical()), the direction's
        tangential components by up to 9.9e-8 / sqrt(s2) and the colour with them.  At roughness 0 (t = 1e-6) that is a relative error
        of 0.2 to 0.35, where the reference's own two runs differ by as much;
      * rows 11, 259, 352, 667: the same in GTR1, the clearcoat term at a mirror direction (clearcoatAlpha^2 down to 7e-6);
      * rows 837, 950, 1198, grazing incidence: Choice's 1 - specrate with specrate = 1 - O(cosi) (the diffuse colour off by
        1.2e-8 / cosi at cosi = 1.9e-6), and reflect(-indir, h) cancelling (2.8e-7 absolute in the direction, 3.2e-7 / coso in the colour).
    None of them is a wrong weight or a wrong branch (the discrete outcomes above are exact, and the strict build -- the same
    statements with IEEE division, roots and libm -- is inside on every row at 0.08 x its bound)."""
    dc.check_values(*evaluated['fast'], gold, 'fast', 'Disney cube [fast]')


def words_differ(a, b):
    '''(rows where a word differs other than NaN against NaN or +0 against -0, the number of +0 / -0 words)'''
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    diff = a.view(np.uint32) != b.view(np.uint32)
    zeros = diff & (a == 0) & (b == 0)
    nans = diff & np.isnan(a) & np.isnan(b)
    return np.flatnonzero((diff & ~zeros & ~nans).any(axis=1)), int(zeros.sum())


@pytest.mark.parametrize('variant', ['plain', 'lean'])
def test_plain_and_lean_instantiations_return_the_generic_words(gold, fresh, variant):
    c = context('fast')
    admitted = dc.admitted(gold, variant)
    cls = gold['cls'][:, 0]
    want_cls = [dc.M_PLAIN, dc.M_LEAN] if variant == 'plain' else [dc.M_LEAN]
    assert admitted[np.isin(cls, want_cls)].all() and admitted.sum() >= 90
    if variant == 'lean':
        x = gold['in'][admitted]
        assert (np.signbit(x[:, 7]) | np.signbit(x[:, 8])).sum() >= dc.MIN_ROWS, 'the -0.0 rows are among the admitted ones'
    zeros = 0
    for fn, rows in (('disney_brdf', dc.rows_brdf(gold)), ('disney_bounce', dc.rows_bounce(gold))):
        generic = c.unit_eval(fn, rows[admitted])
        special = c.unit_eval(f'{fn}_{variant}', rows[admitted])
        assert np.array_equal(np.isnan(generic), np.isnan(special)), f'{fn}_{variant}: the NaN pattern differs'
        bad, z = words_differ(special, generic)
        zeros += z
        report(f'{fn}_{variant}: {int(admitted.sum())} admitted rows, {bad.size} differ from the generic kind in a word, {z} words are +0 against -0')
        first = np.flatnonzero(admitted)[bad[:4]]
        assert bad.size == 0, (f'{fn}_{variant}: {bad.size} of {int(admitted.sum())} admitted rows differ from the generic instantiation, first fixture rows '
                               f'{first} (classes {gold["cls"][first].tolist()}): {special[bad[:2]]} vs {generic[bad[:2]]}')
    report(f'Disney {variant} instantiation: +0 against -0 in {zeros} words in all')


def test_strict_build_refuses_the_instantiation_kinds(gold, fresh):
    c = context('strict')
    for name in ('disney_brdf_plain', 'disney_bounce_plain', 'disney_brdf_lean', 'disney_bounce_lean'):
        with pytest.raises(RuntimeError, match='strict build has none'):
            c.unit_eval(name, dc.rows_brdf(gold)[:4])

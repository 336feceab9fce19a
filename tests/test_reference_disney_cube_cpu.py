'''
The C oracle's Disney.brdf and Disney.bounce (orc_disney_brdf / orc_disney_bounce, both precisions) held to
tests/golden/reference_disney_cube.npz: the reference's own function bodies (materials/disney.py:13-233) evaluated over the whole
parameter cube -- parameters pinned at exactly 0 and 1, the plain mask and the lean rule with -0.0, the tint branch, ior at and
around 1, the alpha clamp; grazing, normal, mirror, opposite and below-surface directions, the critical angle; samples at 0, below
1 and at every Choice threshold (tests/golden/make_reference_disney_cube_golden.py draws them class by class).

tests/disney_cube.py holds the checks and states the bounds; tests/test_reference_disney_cube_gpu.py runs the same ones on the HIP
device functions.  The report lines (helpers.report: printed, -s, and appended to the parity report file) give per class the rows, the well-conditioned rows, the
flagged share and the worst error in units of the base bound.

The GPU file also holds the plain and the lean instantiation of the production build to the generic one on the rows their mask
admits.  Which rows those are is decided by a rule written in tests/disney_cube.py; here that rule is held to the host's own --
shade_feat_material and shade_lean_material of ptina_amd/csrc/shade_feat.h, compiled into a scratch shared object as
tests/test_shade_lean_cpu.py does -- on every row of the fixture, the rows it does not admit included.
'''

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import disney_cube as dc


@pytest.fixture(scope='module')
def gold():
    return dc.load()


def test_fixture_covers_every_class_and_every_leaf(gold):
    dc.check_coverage(gold)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_oracle_disney_brdf_and_bounce_over_the_cube(gold, oracle_mod, prec):
    f64 = prec == 'f64'
    lib = oracle_mod.load(f64=f64)
    T, ct = (np.float64, C.c_double) if f64 else (np.float32, C.c_float)

    def P(a):
        return a.ctypes.data_as(C.POINTER(ct))
    rows = gold['in'].astype(T)                   # stored as f32: the f64 build takes the same values widened
    got_brdf, got_b = np.zeros((len(rows), 3), T), np.zeros((len(rows), 7), T)
    for k, x in enumerate(rows):
        p, n, ind, outd, samp = (np.ascontiguousarray(x[s]) for s in (slice(0, 14), slice(14, 17), slice(18, 21), slice(21, 24), slice(24, 27)))
        lib.orc_disney_brdf(P(p), P(n), ct(x[17]), P(ind), P(outd), P(got_brdf[k]))
        lib.orc_disney_bounce(P(p), P(n), ct(x[17]), P(ind), P(samp), P(got_b[k]))
    dc.check(got_brdf, got_b, gold, prec, f'oracle Disney cube [{prec}]')
    if not f64:
        checks_see_a_wrong_row_and_skip_a_flagged_one(got_brdf, got_b, gold)


def checks_see_a_wrong_row_and_skip_a_flagged_one(got_brdf, got_b, gold):
    '''The fixture has no flagged row, so the flagged path of the shared checks is walked here: on a copy of the fixture in which the
    f64 run of a few rows is given another branch, those rows may hold anything and the checks still pass; the same values on rows
    that are not flagged fail the discrete and the value checks.'''
    rows = np.flatnonzero((gold['f32/out'][:, 6] != 0) & dc.well_conditioned(gold))[:4]
    bent = {k: gold[k] for k in gold.files}
    bent['f64/branch'] = gold['f64/branch'].copy()
    bent['f64/branch'][rows] ^= 1
    assert dc.flagged(bent)[rows].all() and dc.flagged(bent).sum() == rows.size and not dc.well_conditioned(bent)[rows].any()
    wrong_b, wrong_brdf = got_b.copy(), got_brdf.copy()
    wrong_b[rows[:2]] = np.nan                      # a NaN pattern, a lobe
    wrong_b[rows[2:], 4:] *= 1.5                    # pdf and colour
    wrong_brdf[rows] *= 1.5
    dc.check(wrong_brdf, wrong_b, bent, 'f32', 'oracle Disney cube [f32, 4 rows flagged and wrong]')
    with pytest.raises(AssertionError, match='NaN pattern'):
        dc.check_discrete(wrong_brdf, wrong_b, gold, 'f32', 'oracle Disney cube [f32, wrong rows]')
    wrong_b[rows[:2]] = got_b[rows[:2]]
    with pytest.raises(AssertionError, match='4 rows outside'):
        dc.check_values(wrong_brdf, wrong_b, gold, 'f32', 'oracle Disney cube [f32, wrong rows]')


SHIM = '''
#include "shade_feat.h"
int t_feat(const float *fac, const int32_t *tex) { return shade_feat_material(fac, tex); }
int t_lean(const float *fac, const int32_t *tex) { return shade_lean_material(fac, tex); }
'''
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ptina_amd', 'csrc')
CLEARCOAT, TRANSMISSION = 2, 4                     # shade_feat.h MPT_FEAT_*


def test_admission_rule_is_the_hosts(gold, tmp_path):
    src, so = str(tmp_path / 'shim.c'), str(tmp_path / 'shim.so')
    with open(src, 'w') as f:
        f.write(SHIM)
    cc = os.environ.get('CC') or shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or '/opt/rocm/lib/llvm/bin/clang'
    subprocess.run([cc, '-std=c99', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so], check=True)
    lib = C.CDLL(so)
    lib.t_feat.argtypes = lib.t_lean.argtypes = [C.c_void_p, C.c_void_p]
    fac = dc.material_tables(gold)
    tex = np.full(12, -1, np.int32)
    feat = np.array([lib.t_feat(f.ctypes.data, tex.ctypes.data) for f in fac])
    lean = np.array([lib.t_lean(f.ctypes.data, tex.ctypes.data) for f in fac])
    plain = dc.admitted(gold, 'plain')
    assert np.array_equal(plain, feat == 0) and np.array_equal(plain, (feat & (CLEARCOAT | TRANSMISSION)) == 0)
    assert np.array_equal(dc.admitted(gold, 'lean'), plain & (lean == 1))
    cls = gold['cls'][:, 0]
    assert plain[np.isin(cls, [dc.M_PLAIN, dc.M_LEAN])].all() and dc.admitted(gold, 'lean')[cls == dc.M_LEAN].all()
    dc.report(f'disney cube: the plain mask admits {int(plain.sum())} rows, the lean rule {int(dc.admitted(gold, "lean").sum())}; '
              f'not admitted: {int((~plain).sum())} and {int((~dc.admitted(gold, "lean")).sum())} (sheen or subsurface set on {int((plain & (lean == 0)).sum())} plain rows)')
    assert (plain & (lean == 0)).sum() >= dc.MIN_ROWS and (~plain).sum() >= dc.MIN_ROWS

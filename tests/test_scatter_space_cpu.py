'''
CPU tests of the spacing of a scatter: mpt_scatter_space_rule -- the elimination on the host from
ptina_amd/csrc/scatter_rule.h -- against tests/scatter_space_ref.py, flags and synchronous rounds, on the point sets the GPU test
sends through the door; the preconditions of those sets; the refusals that need no device; and tools/scatter_rule_check.cpp's
elimination checks built with the host sanitizers and run.  No GPU.
'''

import os
import shutil
import subprocess

import numpy as np
import pytest

import scatter_space_ref as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cases():
    return {name: (pts, r, *ss.eliminate(pts, r)) for name, pts, r in ss.door_cases()}


def test_rule_equals_the_restatement_flags_and_rounds(cases):
    from ptina_amd import _lib
    for name, (pts, r, kept, rounds) in cases.items():
        rc, got, took = _lib.scatter_space_rule(pts, r)
        assert rc == 0 and got.dtype == np.uint8 and np.array_equal(got.astype(bool), kept), name
        assert took == rounds, (name, took, rounds)
        assert np.array_equal(ss.greedy_of_points(pts, r), kept), name    # (the form tools/scatter_bench.py runs on large sets)


def test_point_sets_are_what_their_names_say(cases):
    one = cases['one point']
    assert one[2].tolist() == [True] and one[3] == 1
    pts, r, kept, rounds = cases['two points exactly r apart']
    d = pts[1] - pts[0]
    assert ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2]) == r * r and kept.tolist() == [True, True]
    pts, r, kept, rounds = cases['two points an ulp of d2 below r']
    d = pts[1] - pts[0]
    assert ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2]) == np.nextafter(r * r, 0.0) and kept.tolist() == [True, False]
    assert cases['64 coincident points'][2].tolist() == [True] + [False] * 63
    for name in ('a chain of 40, 0.6 r apart', 'the chain in reverse'):
        assert cases[name][2].tolist() == [True, False] * 20 and cases[name][3] == 40
    pts, r, kept, rounds = cases['pairs across cell borders']
    h = r * (1.0 + 2.0 ** -20)
    assert (pts.min(axis=0) == 0).all() and kept[0] and kept[1::2].all() and not kept[2::2].any()
    cells = np.floor(pts / h)
    for k in range(12):                                                   # each pair lies in two cells, 1, 2 and 1000 edges out
        a, b = cells[1 + 2 * k], cells[2 + 2 * k]
        along = (a != b)
        assert along.sum() == (3 if k % 4 == 3 else 1) and (b - a)[along].tolist() == [1.0] * int(along.sum()) and b[along][0] == (1, 2, 1000)[k // 4]
    pts, r, kept, rounds = cases['an extent of 2^30 r']
    assert (pts.max(axis=0) - pts.min(axis=0)).max() == 2.0 ** 30 * r and kept.tolist() == [True, False, True, False, True]
    pts, r, kept, rounds = cases['a 10 x 10 x 10 lattice 1.5 r apart']
    assert kept.all() and np.unique(np.floor(pts / (r * (1.0 + 2.0 ** -20))), axis=0).shape[0] == 1000
    pts, r, kept, rounds = cases['a NaN coordinate among 63 points']
    bad = int(np.flatnonzero(np.isnan(pts).any(axis=1))[0])
    rest = np.delete(pts, bad, axis=0)
    assert kept[bad] and np.array_equal(np.delete(kept, bad), ss.eliminate(rest, r)[0])
    for name in ('257 uniform points', '1000 uniform points'):
        assert 0.25 <= 1.0 - cases[name][2].mean() <= 0.75, name


def test_rule_refusals_and_edges():
    from ptina_amd import _lib
    pts = np.zeros((3, 3))
    assert _lib.scatter_space_rule(pts, 0.0)[:2][0] == 0 and _lib.scatter_space_rule(pts, 0.0)[1].tolist() == [1, 1, 1]   # r = 0: nothing conflicts
    assert _lib.scatter_space_rule(pts, float('inf'))[1].tolist() == [1, 0, 0]
    assert _lib.scatter_space_rule(pts, -1.0)[0] == 1 and _lib.scatter_space_rule(pts, float('nan'))[0] == 1
    rc, kept, rounds = _lib.scatter_space_rule(np.zeros((0, 3)), 1.0)
    assert (rc, kept.size, rounds) == (0, 0, 0)
    lib = _lib.load_library()
    assert lib.mpt_scatter_space_rule(None, 2, 1.0, None, None) == 1 and lib.mpt_scatter_space_rule(None, -1, 1.0, None, None) == 1
    # the keywords of ModelPool.add_scatter, checked before the library is asked
    assert _lib.scatter_spacing(10) == (0.0, 40) and _lib.scatter_spacing(10, 0.5, 12) == (0.5, 12) and _lib.scatter_spacing(10, 0, 3) == (0.0, 3)
    for bad in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='negative or not finite'):
            _lib.scatter_spacing(10, bad)
    for bad in (9, 2 ** 24 + 1):
        with pytest.raises(ValueError, match=r'%d candidates outside \[10, 16777216\]' % bad):
            _lib.scatter_spacing(10, 0.5, bad)


def test_restatement_by_hand():
    '''three points 0.5 apart at r = 0.75: the middle one is rejected in round 2, when the first is kept, and frees the last in round 3'''
    c = ss.conflicts(np.array([[0, 0, 0], [0.5, 0, 0], [1.0, 0, 0]]), 0.75)
    assert c.tolist() == [[True, True, False], [True, True, True], [False, True, True]]
    assert ss.greedy(c).tolist() == [True, False, True]
    kept, rounds = ss.rounds(c)
    assert kept.tolist() == [True, False, True] and rounds == 3


def test_rule_check_program_runs_the_elimination_under_the_sanitizers(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'scatter_rule_check')
    subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'scatter_rule_check.cpp'),
                    '-o', exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, 'space'], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and 'scatter_rule_check space: ok' in run.stdout, run.stderr[-2000:]

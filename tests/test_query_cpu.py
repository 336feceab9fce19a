'''
CPU tests of the batch ray queries' yardstick (tests/query_ref.py) and boundary: the classification against a per-ray brute
force written as a plain loop, shown to fail when a triangle is moved or two faces are swapped in an answer, its caps on every
scene tests/test_query_gpu.py uses, the oracle's own LinearBVH.intersect against it on every decided ray (which also measures
the depth / u / v deviation of the reference's f32 arithmetic that the GPU tolerance is derived from: 4 x, per scene, over the
same rays), and the C ABI of mpt_query_*.
'''

import math
import os
import re

import numpy as np
import pytest

import query_ref as qr
from test_visibility_ref_cpu import WORLD, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY_CALLS = ('mpt_query_closest', 'mpt_query_occluded', 'mpt_query_kernel_time')
GPU_CASES = ('n2', 'n3', 'n33', 'n300', 'n1025', 'n5000', 'moved', 'x1024', 'flat', 'deep')

_refs = {}


def reference(name):
    '''(o, d, verdicts) of a case's rays, computed once per process'''
    if name not in _refs:
        c = case(name)
        o, d = qr.rays(c.pos, c.n)
        _refs[name] = (o, d, qr.classify(c.pos, o, d))
    return _refs[name]


# ---------------------------------------------------------------- against a plain loop
def _loop_nearest(pos, o, d):
    '''one ray, triangle by triangle, scalar float64 Moller-Trumbore: [(t, face)] of every hit, nearest first'''
    o = [float(x) for x in o]
    d = [float(x) for x in d]
    ln = math.sqrt(sum(x * x for x in d))
    d = [x / ln for x in d]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]   # noqa: E731
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]                                                   # noqa: E731
    hits = []
    for f in range(pos.shape[0]):
        v0, v1, v2 = (pos[f, k].tolist() for k in range(3))
        e1, e2 = [v1[k] - v0[k] for k in range(3)], [v2[k] - v0[k] for k in range(3)]
        p = cross(d, e2)
        det = dot(e1, p)
        if det == 0.0:
            continue
        s = [o[k] - v0[k] for k in range(3)]
        u = dot(s, p) / det
        q = cross(s, e1)
        v = dot(d, q) / det
        t = dot(e2, q) / det
        if u >= 0 and v >= 0 and u + v <= 1 and t > 0:
            hits.append((t, f, u, v))
    return sorted(hits)


@pytest.mark.parametrize('name', ['n2', 'n33'])
def test_query_ref_agrees_with_a_per_ray_loop(name):
    c = case(name)
    o, d, ref = reference(name)
    seen_hit = seen_miss = 0
    for r in np.flatnonzero(ref['decided']):
        hits = _loop_nearest(c.pos, o[r], d[r])
        if ref['hit'][r]:
            assert hits and hits[0][1] == ref['index'][r], f'{name}: ray {r}: the loop finds {hits[:2]}, the reference face {ref["index"][r]}'
            assert abs(hits[0][0] - ref['t'][r]) <= 1e-12 * max(1.0, ref['t'][r])
            assert abs(hits[0][2] - ref['u'][r]) <= 1e-9 and abs(hits[0][3] - ref['v'][r]) <= 1e-9
            assert len(hits) == 1 or hits[1][0] > hits[0][0] * (1 + qr.DEPTH_GAP)
            seen_hit += 1
        else:
            assert not hits, f'{name}: ray {r}: the loop finds {hits[:2]}, the reference a miss'
            seen_miss += 1
    assert seen_hit > 100 and seen_miss > 100


# ---------------------------------------------------------------- the check can fail
def _truth(ref):
    '''an answer that is the reference's own'''
    return dict(hit=ref['hit'].copy(), index=ref['index'].astype(np.int32), depth=ref['t'].astype(np.float32), u=ref['u'].astype(np.float32),
                v=ref['v'].astype(np.float32), object=np.full(ref['hit'].size, -1, np.int32))


def test_the_reference_passes_itself():
    _, _, ref = reference('n300')
    assert qr.errors(ref, _truth(ref), 'truth', tol_depth=1e-5, tol_uv=1e-6) == []


def test_a_moved_triangle_fails():
    '''the answers of the model with one triangle moved out of the way, held to the model as it is'''
    c = case('n300')
    o, d, ref = reference('n300')
    victim = int(np.bincount(ref['index'][ref['decided'] & ref['hit']]).argmax())
    moved = c.pos.copy()
    moved[victim] += 100.0
    bad = qr.errors(ref, _truth(qr.classify(moved, o, d)), 'one triangle moved')
    assert bad and all(f'reference hit True face {victim}' in b for b in bad), bad[:4]


def test_two_swapped_faces_fail():
    _, _, ref = reference('n300')
    got = _truth(ref)
    faces = np.unique(ref['index'][ref['decided'] & ref['hit']])
    a, b = int(faces[0]), int(faces[1])
    got['index'] = np.where(ref['index'] == a, b, np.where(ref['index'] == b, a, ref['index'])).astype(np.int32)
    bad = qr.errors(ref, got, 'two faces swapped')
    assert bad and all(f'face {a}' in x and f'face {b}' in x for x in bad), bad[:4]


def test_a_wrong_object_and_a_wrong_depth_fail():
    _, _, ref = reference('n300')
    got = _truth(ref)
    r = int(np.flatnonzero(ref['decided'] & ref['hit'])[0])
    got['object'][r] = 0
    got['depth'][r] *= np.float32(1.01)
    bad = qr.errors(ref, got, 'wrong', tol_depth=1e-5, tol_uv=1e-6)
    assert len(bad) == 2 and 'object 0' in bad[0] and 'depth' in bad[1], bad
    first = np.array([0, 100, 200])
    want = _truth(ref)
    want['object'] = np.where(ref['hit'], np.searchsorted(first, ref['index'], side='right') - 1, -1).astype(np.int32)
    assert qr.errors(ref, want, 'objects', first=first) == []
    assert qr.errors(ref, got, 'objects', first=first)


# ---------------------------------------------------------------- the caps
@pytest.mark.parametrize('name', GPU_CASES)
def test_caps_hold_on_every_case_the_gpu_tests_use(name):
    _, _, ref = reference(name)
    qr.caps(name, ref)
    assert not (ref['hit'] & ~ref['decided']).any() and np.all((ref['index'] >= 0) == ref['hit'])


def test_avoiding_the_nearest_face_leaves_enough_decided_rays():
    for name in ('n300', 'n1025'):
        c = case(name)
        o, d, ref = reference(name)
        sel = np.flatnonzero(ref['decided'] & ref['hit'])
        without = qr.classify(c.pos, o[sel], d[sel], avoid=ref['index'][sel])
        share = float(without['decided'].mean())
        print(f'{name}: {share:.3f} of the decided hits are decided without their nearest face')
        assert share >= 0.5
        assert not (without['index'] == ref['index'][sel]).any()


# ---------------------------------------------------------------- the oracle's own walk
@pytest.mark.parametrize('name', GPU_CASES)
def test_the_oracles_intersect_agrees_on_every_decided_ray(oracle_mod, name):
    '''... and how far the reference's f32 Face.intersect is from the f64 values on these rays: the kernels are allowed 4 x that'''
    from helpers import setup_oracle
    c = case(name)
    o, d, ref = reference(name)
    qr.caps(name, ref)
    orc = setup_oracle(oracle_mod, c.scene, c.nx, c.ny, camera=c.camera, lights=[], world=WORLD)
    got = qr.oracle_answers(orc, o, d)
    bad = qr.errors(ref, got, f'oracle {name}')
    assert not bad, f'{len(bad)} wrong rays; ' + '; '.join(bad[:4])
    dev_depth, dev_uv = qr.deviation(ref, got)
    print(f'{name}: the oracle\'s f32 intersect is within {dev_depth:.3g} in depth and {dev_uv:.3g} in u, v of the f64 values '
          f'over {int((ref["decided"] & ref["hit"]).sum())} decided hits')
    assert 0 < dev_depth < np.inf and 0 < dev_uv < np.inf
    # with the nearest face avoided the oracle names the next one
    sel = np.flatnonzero(ref['decided'] & ref['hit'])[:256]
    without = qr.classify(c.pos, o[sel], d[sel], avoid=ref['index'][sel])
    bad = qr.errors(without, qr.oracle_answers(orc, o[sel], d[sel], avoid=ref['index'][sel]), f'oracle {name} avoiding')
    assert not bad, '; '.join(bad[:4])


# ---------------------------------------------------------------- the C ABI
def test_header_and_ctypes_table_carry_the_query_calls():
    from ptina_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'miptina.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(mpt_[a-z0-9_]+)\s*\(', src))
    for name in QUERY_CALLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name


def test_library_exports_the_query_calls():
    from ptina_amd import _lib
    lib = _lib.load_library()
    for name in QUERY_CALLS:
        assert hasattr(lib, name), name


def test_bad_arguments_fail_with_a_message():
    from ptina_amd import _lib
    lib = _lib.load_library()
    o = np.zeros((4, 3), np.float32)
    hit, occ = np.zeros(4, np.int32), np.zeros(4, np.int32)
    none = None
    assert lib.mpt_query_closest(None, 4, _lib.fptr(o), _lib.fptr(o), none, _lib.iptr(hit), none, none, none, none, none, 0) != 0
    assert 'null context' in _lib.last_error()
    assert lib.mpt_query_occluded(None, 4, _lib.fptr(o), _lib.fptr(o), none, none, _lib.iptr(occ), 0) != 0
    assert 'null context' in _lib.last_error()
    assert lib.mpt_query_kernel_time(None, None, None) != 0
    assert 'null context' in _lib.last_error()
    assert lib.mpt_query_closest(None, -1, _lib.fptr(o), _lib.fptr(o), none, _lib.iptr(hit), none, none, none, none, none, 0) != 0
    assert 'mpt_query_closest' in _lib.last_error() and 'n -1' in _lib.last_error()
    assert lib.mpt_query_occluded(None, -3, _lib.fptr(o), _lib.fptr(o), none, none, _lib.iptr(occ), 0) != 0
    assert 'mpt_query_occluded' in _lib.last_error() and 'n -3' in _lib.last_error()
    assert lib.mpt_query_closest(None, 4, _lib.fptr(o), _lib.fptr(o), none, _lib.iptr(hit), none, none, none, none, none, -5) != 0
    assert 'chunk -5' in _lib.last_error()


def test_python_doors_exist_and_shape_their_arguments():
    from ptina_amd.tree import lbvh
    from ptina_amd import worker
    for name in ('intersect', 'occluded', 'pick'):
        assert callable(getattr(lbvh.LinearBVH, name)) and callable(getattr(worker, name))
    o, d, n = lbvh._rays([0, 0, 1], np.ones((5, 3)))
    assert n == 5 and o.shape == d.shape == (5, 3) and o.dtype == d.dtype == np.float32 and o.flags.c_contiguous
    assert lbvh._rays(np.zeros((0, 3)), np.zeros((0, 3)))[2] == 0
    assert lbvh._per_ray(7, 3, np.int32, 'avoid').tolist() == [7, 7, 7] and lbvh._per_ray(None, 3, np.int32, 'avoid') is None
    with pytest.raises(ValueError):
        lbvh._rays(np.zeros((4, 2)), np.zeros((4, 3)))
    with pytest.raises(ValueError):
        lbvh._per_ray([1, 2], 3, np.int32, 'avoid')

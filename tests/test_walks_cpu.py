'''
CPU tests of the ray sets tests/test_walks_gpu.py sends through the production walks (BVHTree.walk_trace, csrc/walk_eval.hip): that
they are what they claim to be, that tests/query_ref.py decides enough of them -- the caps, asserted here on every case the GPU
tests use -- and that the oracle's own f32 LinearBVH.intersect is right on every decided ray of every set, which also measures
the depth / u / v deviation of the reference's arithmetic on these rays (the GPU bounds on u and v are multiples of it); and the
C ABI and Python shape of the door.

  A  query_ref.rays as the query tests use it: origins in and around the box, every direction octant
  B  bounce rays: origins ON the faces A's decided hits found (the f64 hit point rounded to f32), avoid = that face
  C  axis rays: one or two direction components exactly zero, half of them -0.0
  far  rays aimed at (and past) the model from 4 and 64 bounding radii
'''

import os
import re

import numpy as np
import pytest

import query_ref as qr
from test_query_cpu import GPU_CASES, reference
from test_visibility_ref_cpu import WORLD, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ('A', 'B', 'C')

_sets = {}


def sets(name):
    '''{set: (o, d, avoid or None, verdicts)} of a case, computed once per process and never changed; no set B for `flat`'''
    if name not in _sets:
        c = case(name)
        o, d, ref = reference(name)
        out = {'A': (o, d, None, ref)}
        if name != 'flat':
            ob, db, av = qr.bounce_rays(c.pos, o, d, ref, c.n + 1)
            out['B'] = (ob, db, av, qr.classify(c.pos, ob, db, avoid=av))
        oc, dc = qr.axis_rays(c.pos, c.n + 2)
        out['C'] = (oc, dc, None, qr.classify(c.pos, oc, dc))
        _sets[name] = out
    return _sets[name]


_far = {}


def far(name, radii):
    if (name, radii) not in _far:
        c = case(name)
        o, d = qr.far_rays(c.pos, radii, c.n + 3)
        _far[(name, radii)] = (o, d, qr.classify(c.pos, o, d))
    return _far[(name, radii)]


def assert_caps(name):
    '''the caps of every set of a case, before anything a kernel computed is read'''
    s = sets(name)
    qr.caps(name, s['A'][3])
    per = np.bincount(qr.octant(qr.normalized32(s['A'][1]))[s['A'][3]['decided']], minlength=8)
    print(f'{name} set A: decided rays per direction octant {per.tolist()}')
    assert per.min() >= 100, (name, per.tolist())
    for which in ('B', 'C'):
        if which in s:
            qr.caps_of_set(name, which, s[which][3])
    return s


# ---------------------------------------------------------------- the sets are what they claim
@pytest.mark.parametrize('name', GPU_CASES)
def test_caps_and_octants_hold_on_every_case(name):
    s = assert_caps(name)
    for which, (o, d, avoid, ref) in s.items():
        assert o.dtype == d.dtype == np.float32 and o.shape == d.shape == (ref['decided'].size, 3)
        assert not (ref['hit'] & ~ref['decided']).any() and np.all((ref['index'] >= 0) == ref['hit'])
        if avoid is not None:
            assert not (ref['index'] == avoid).any(), f'{name} set {which}: a ray hits the face it avoids'


@pytest.mark.parametrize('name', ['n3', 'n300', 'moved', 'x1024'])
def test_bounce_rays_start_on_the_face_they_avoid(name):
    c = case(name)
    o, d, avoid, ref = sets(name)['B']
    _, _, refa = reference(name)
    assert np.array_equal(avoid, refa['index'][refa['decided'] & refa['hit']])
    tri = c.pos[avoid]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    off = np.abs(((o.astype(np.float64) - tri[:, 0]) * nrm).sum(axis=1))
    size = np.abs(c.pos).max()
    assert off.max() <= 8 * 2.0 ** -24 * size, f'{name}: an origin is {off.max():.3g} off its face (f32 rounding of the point: {2.0 ** -24 * size:.3g})'
    # ... and without `avoid` most of them would meet that very face at t ~ 0: the set needs the filter
    plain = qr.classify(c.pos, o, d)
    assert float(plain['decided'].mean()) < 0.5, name


@pytest.mark.parametrize('name', ['n300', 'flat'])
def test_axis_rays_have_their_zeros(name):
    o, d, _, _ = sets(name)['C']
    zeros = (d == 0).sum(axis=1)
    assert d.shape == (qr.AXIS_RAYS, 3) and np.all(zeros >= 1) and np.all(zeros[1::2] == 2) and np.all(zeros[0::2] == 1)
    minus = int((np.signbit(d) & (d == 0)).sum())
    assert minus == int((d == 0).sum()) // 2
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = np.float32(1) / d
        oinv = o * inv
    assert np.isposinf(inv).any() and np.isneginf(inv).any() and np.isinf(oinv).any()
    assert np.all(np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1) < 1e-6)


def test_far_rays_are_far_and_decided():
    for radii in (4, 64):
        c = case('n300')
        o, d, ref = far('n300', radii)
        lo, hi = c.pos.reshape(-1, 3).min(axis=0), c.pos.reshape(-1, 3).max(axis=0)
        dist = np.linalg.norm(o - (lo + hi) / 2, axis=1) / (np.linalg.norm(hi - lo) / 2)
        assert np.all(np.abs(dist - radii) < 1e-3 * radii)
        dec, hits, misses = float(ref['decided'].mean()), float((ref['decided'] & ref['hit']).mean()), float((ref['decided'] & ~ref['hit']).mean())
        print(f'n300 from {radii} radii: decided {dec:.3f}, hits {hits:.3f}, misses {misses:.3f}')
        assert dec >= 0.90 and hits >= 0.20 and misses >= 0.20


# ---------------------------------------------------------------- the oracle's own walk on every set
_oracle_dev = {}


def faces_the_oracles_tree_holds(orc, n):
    """bool [n]: the faces some leaf of the oracle's LBVH names.  The reference sorts 30-bit Morton codes without a tie-break and
    its hierarchy (lbvh.py:93-146) can leave leaves with equal codes out of every node; the product's builds sort
    (code, index) keys and hold every face (tests/tree_checks.py).  Of the cases here only `deep` has equal codes: the sixteen
    copies of one triangle, and the chain's last triangles, whose centres differ below the code's 10 bits per axis"""
    tree = orc.get_tree(n)
    held = np.zeros(n, bool)
    kids = tree['child'].reshape(-1)
    held[tree['leaf'][kids[kids < n]]] = True
    return held


def oracle_deviation(oracle_mod, name, which):
    '''(depth, uv): how far the oracle's f32 LinearBVH.intersect is from the f64 values on the decided hits of a set; asserts
    that it is right on every decided ray first.  One rule takes rays out: a ray whose nearest face the
    oracle's own tree does not hold -- the reference cannot find what it never stored, and the kernels, whose trees hold every
    face, get no such allowance'''
    if (name, which) not in _oracle_dev:
        from helpers import setup_oracle
        c = case(name)
        o, d, avoid, ref = sets(name)[which]
        orc = setup_oracle(oracle_mod, c.scene, c.nx, c.ny, camera=c.camera, lights=[], world=WORLD)
        held = faces_the_oracles_tree_holds(orc, c.n)
        assert held.all() or name == 'deep', f'{name}: the oracle\'s tree holds {int(held.sum())} of {c.n} faces'
        lost = ref['hit'] & ~held[np.maximum(ref['index'], 0)]
        got = qr.oracle_answers(orc, o, d, avoid)
        assert not (got['hit'] & ~held[np.maximum(got['index'], 0)]).any()
        if lost.any():
            print(f'{name} set {which}: {int(lost.sum())} decided rays left out of the oracle comparison: the reference tree does not hold their nearest face')
            assert lost.sum() <= 0.02 * lost.size
        kept = dict(ref, decided=ref['decided'] & ~lost)
        bad = qr.errors(kept, got, f'oracle {name} set {which}')
        assert not bad, f'{len(bad)} wrong rays; ' + '; '.join(bad[:4])
        _oracle_dev[(name, which)] = qr.deviation(kept, got)
    return _oracle_dev[(name, which)]


@pytest.mark.parametrize('name', GPU_CASES)
def test_the_oracles_intersect_agrees_on_every_decided_ray_of_every_set(oracle_mod, name):
    for which in assert_caps(name):
        dev_depth, dev_uv = oracle_deviation(oracle_mod, name, which)
        ref = sets(name)[which][3]
        print(f'{name} set {which}: the oracle\'s f32 intersect is within {dev_depth:.3g} in depth and {dev_uv:.3g} in u, v of the f64 values '
              f'over {int((ref["decided"] & ref["hit"]).sum())} decided hits')
        assert 0 < dev_depth < np.inf and 0 < dev_uv < np.inf


# ---------------------------------------------------------------- the door's C ABI and Python shape
def test_header_ctypes_table_and_library_carry_the_door():
    from ptina_amd import _lib
    from ptina_amd.tree import lbvh
    src = open(os.path.join(ROOT, 'include', 'miptina.h')).read()
    enum = dict((k, int(v)) for k, v in re.findall(r'\b(MPT_WALK_[A-Z0-9_]+)\s*=\s*(\d+)', src))
    assert [enum[k] for k in ('MPT_WALK_GATHER', 'MPT_WALK_LDS', 'MPT_WALK_WIDE_EXACT', 'MPT_WALK_WIDE_QUANT', 'MPT_WALK_LDS4', 'MPT_WALK_COUNT')] == [0, 1, 2, 3, 4, 5]
    assert lbvh.WALKS == ('gather', 'lds', 'wide_exact', 'wide_quant', 'lds4') and len(lbvh.WALKS) == enum['MPT_WALK_COUNT']
    declared = set(re.findall(r'\b(mpt_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    assert 'mpt_walk_trace' in declared and 'mpt_walk_trace' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['mpt_walk_trace'][1]) == 13
    assert hasattr(_lib.load_library(), 'mpt_walk_trace')
    assert callable(lbvh.LinearBVH.walk_trace)


def test_bad_arguments_fail_with_a_message():
    from ptina_amd import _lib
    lib = _lib.load_library()
    o = np.zeros((4, 3), np.float32)
    hit = np.zeros(4, np.int32)
    none = None
    assert lib.mpt_walk_trace(None, 0, 4, _lib.fptr(o), _lib.fptr(o), none, none, _lib.iptr(hit), none, none, none, none, 0) != 0
    assert 'null context' in _lib.last_error()
    assert lib.mpt_walk_trace(None, 0, -2, _lib.fptr(o), _lib.fptr(o), none, none, _lib.iptr(hit), none, none, none, none, 0) != 0
    assert 'mpt_walk_trace' in _lib.last_error() and 'n -2' in _lib.last_error()
    assert lib.mpt_walk_trace(None, 0, 4, _lib.fptr(o), _lib.fptr(o), none, none, _lib.iptr(hit), none, none, none, none, -7) != 0
    assert 'chunk -7' in _lib.last_error()


def test_the_door_is_built_with_the_render_kernels_flags_in_both_libraries():
    '''one rule for walk_eval.hip, with FASTFLAGS, that the spill-test build goes through as well (it sets FASTFLAGS and OBJ)'''
    mk = open(os.path.join(ROOT, 'ptina_amd', 'csrc', 'Makefile')).read()
    rule = re.search(r'^\$\(OBJ\)/walk_eval\.o: walk_eval\.hip \$\(DEPS\)\n\t.*\n\t(.*)$', mk, flags=re.M)
    assert rule and '-DMPT_STRICT=0' in rule.group(1) and '$(FASTFLAGS)' in rule.group(1) and '-ffp-contract=fast' in rule.group(1)
    assert '$(OBJ)/walk_eval.o' in re.search(r'^\$\(OUT\):(.*)$', mk, flags=re.M).group(1)
    assert re.search(r'^spilltest:\n\t\$\(MAKE\) OBJ=_obj_spill OUT=\.\./libmiptina_spilltest\.so FASTFLAGS=.*MPT_X_SPILL_CAP=4.* all$', mk, flags=re.M)

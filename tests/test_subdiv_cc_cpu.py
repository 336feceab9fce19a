'''
CPU tests of Catmull-Clark subdivision: the pure function of the host runtime (mpt_subdiv_topology_cc:
no context, no GPU), decoded by the documented layout, against the independent numpy restatement the GPU tests hold the kernels to
(tests/subdiv_cc_ref.py); the restatement itself against values worked out by hand and against the uniform bicubic B-spline, a
yardstick with no topology in it; both schemes' topology functions against the words they gave before they shared their code; and
that code under the host sanitizers, in a stand-alone program.
'''

import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import subdiv_ref
import subdiv_crease_ref
import subdiv_cc_ref as ref
import test_subdiv_cpu as loop_cpu

u32 = np.uint32
LEVELS = (1, 2, 3)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _topology(rec, levels, polys=None, creases=None, corners=None):
    from ptina_amd import _lib
    return _lib.subdiv_topology_cc(rec, levels, polys, creases, corners)


def _rule(r):
    return (r[0], r[1], list(r[2]), r[3])


def _tables_equal(got, want, what):
    assert np.array_equal(got['counts'], want['counts']), (what, got['counts'], want['counts'])
    assert np.array_equal(got['first_corner'], want['first_corner']), what
    assert sorted(got['rules']) == sorted(want['rules'])
    for l in got['rules']:
        assert [_rule(r) for r in got['rules'][l]] == [_rule(r) for r in want['rules'][l]], (what, l)
    assert got['rings'] == want['rings'], what
    assert [(v, k, list(i)) for v, k, i in got['records']] == [(v, k, list(i)) for v, k, i in want['records']], what
    assert np.array_equal(got['quads1'], want['quads1']), what
    assert np.array_equal(got['faces'], want['faces']), what


# ---------------------------------------------------------------- the topology function against the restatement
@pytest.mark.parametrize('name', ref.NAMES + ref.CREASED)
def test_topology_tables_equal_the_restatement(name):
    rec, polys, creases, corners = ref.fixture(name)
    n = int(polys.sum())
    euler = dict(cube=2, pyramid=2, cap5=2, grid=1, cylinder=0, quad=1, triangle=1, pentagon=1)[name.split('_')[0]]
    for levels in LEVELS:
        rc, words, got = _topology(rec, levels, polys, creases, corners)
        assert rc == 0
        _tables_equal(got, ref.fixture_topology(name, levels), '%s at level %d' % (name, levels))
        # counts: polygons, then n quads per polygon, then four per quad; Euler's number at every level
        assert got['counts'][:, 2].tolist() == [polys.size] + [n * 4 ** (l - 1) for l in range(1, levels + 1)]
        for l, (V, E, F) in enumerate(got['counts'].tolist()):
            assert V - E + F == euler, (name, l, V, E, F)
            if l:
                Vb, Eb, Fb = got['counts'][l - 1].tolist()
                assert V == Vb + Eb + Fb
        assert got['faces'].shape == (2 * n * 4 ** (levels - 1), 3)
        if name in ref.NAMES:
            assert got['offsets'][9] == 0 and len(got['records']) == got['counts'][levels, 0]


@pytest.mark.parametrize('name', ref.NAMES)
def test_zero_creases_give_the_uncreased_block(name):
    rec, polys, _, _ = ref.fixture(name)
    n = int(polys.sum())
    for levels in LEVELS:
        rc, plain, _ = _topology(rec, levels, polys)
        assert rc == 0
        for creases, corners in ((np.zeros(n, np.float32), None), (None, np.zeros(n, bool)), (np.zeros(n), np.zeros(n, np.uint8))):
            rc, words, _ = _topology(rec, levels, polys, creases, corners)
            assert rc == 0 and np.array_equal(words, plain)


def test_the_fixtures_cover_what_they_are_for():
    val = lambda name: sorted(len(r[2]) // 2 for r in ref.fixture_topology(name, 1)['rules'][1] if r[0] == ref.VERT_INT and r[1] & ref.CC)   # noqa: E731
    assert val('cube') == [3] * 8 and val('pyramid') == [3] * 4 + [4] and 5 in val('cap5') and val('grid') == [4] * 16 and val('quad') == []
    rules = ref.fixture_topology('grid', 1)['rules'][1]
    assert sum(r[0] == ref.VERT_BND for r in rules) == 20 and sum(r[:2] == (ref.EDGE_BND, 0) for r in rules) == 20
    assert sum(r[:2] == (ref.EDGE_BND, ref.CC) for r in rules) == 25 and sum(r[:2] == (ref.EDGE_INT, ref.CC) for r in rules) == 40
    assert sorted(set(ref.fixture('pyramid')[1].tolist())) == [3, 4] and 5 in ref.fixture('cap5')[1]
    rec, polys, _, _ = ref.fixture('grid')
    tris, _ = subdiv_ref.weld(rec)
    uv_of = {}
    for s, v in enumerate(tris.reshape(-1)):
        uv_of.setdefault(int(v), set()).add(tuple(rec[s, 6:8].tolist()))
    assert any(len(x) > 1 for x in uv_of.values())                       # a uv seam
    # the creased ones: blends of every kind occur
    kinds = set()
    for name in ref.CREASED:
        for l in LEVELS:
            for rules in ref.fixture_topology(name, l)['rules'].values():
                kinds |= set(r[:2] for r in rules)
    assert {(ref.VERT_INT, ref.CC | ref.BLEND_CREASE), (ref.VERT_INT, ref.FIXED), (ref.EDGE_INT, ref.CC | ref.BLEND_EDGE), (ref.VERT_BND, 0)} <= kinds
    cage_rules = ref.fixture_topology('cube_two', 1)['rules'][1]
    assert sum(r[:2] == (ref.EDGE_BND, 0) for r in cage_rules) == 4          # the edge stated as 0.25 and 2 has 2: sharp at level 0


# ---------------------------------------------------------------- refusals
def _quad(order, polys):
    P = np.float32([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0.5)])
    rec = np.zeros((len(order), 8), np.float32)
    rec[:, :3] = P[list(order)]
    return rec, None if polys is None else np.array(polys, np.int32), None


def _creased_quads(value):
    rec, polys = ref.fan_records([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (2, 0, 0), (2, 1, 0)], [(0, 1, 2, 3), (1, 4, 5, 2)])
    creases = np.zeros(8, np.float32)
    creases[6] = value
    return rec, polys, creases


def _of_loop(kind):
    return lambda: (loop_cpu.REFUSALS[kind][2](), None, None)


REFUSALS = {
    'polys_sum': (10, 'the polygons hold 3 triangles, the mesh has 2', lambda: _quad((0, 1, 2, 0, 2, 3), [5])),
    'polys_few': (10, 'polygon 1 has 2 corners, outside', lambda: _quad((0, 1, 2, 0, 2, 3), [4, 2])),
    'polys_many': (10, 'polygon 0 has 65 corners, outside', lambda: _quad((0, 1, 2, 0, 2, 3), [65])),
    'not_a_fan': (10, 'face 1 does not continue the fan of polygon 0', lambda: _quad((0, 1, 2, 2, 3, 0), [4])),
    'polygon_corners': (5, 'polygon 0 has two corners on one vertex', lambda: _quad((0, 1, 2, 0, 2, 1), [4])),
    'crease_negative': (9, 'the crease of edge 2 of polygon 1 is negative', lambda: _creased_quads(-0.5)),
    'crease_nan': (9, 'the crease of edge 2 of polygon 1 is not a number', lambda: _creased_quads(np.nan)),
    'finite': (4, 'corner 1 of face 1 is not finite', _of_loop('finite')),
    'edge_faces': (6, 'third on the edge', _of_loop('edge_faces')),
    'edge_direction': (7, 'same direction', _of_loop('edge_direction')),
    'fan': (8, 'not one fan', _of_loop('fan')),
}


@pytest.mark.parametrize('kind', sorted(REFUSALS))
def test_every_refusal_fires_with_its_words(kind):
    code, words, make = REFUSALS[kind]
    rec, polys, creases = make()
    rc, why, got = _topology(rec, 2, polys, creases)
    assert rc == code and got is None and why.startswith('subdivision: ') and words in why, (rc, why)


def test_levels_and_sizes_are_refused():
    rec, polys, _, _ = ref.fixture('quad')
    assert _topology(rec, 0, polys)[0] == 2 and _topology(rec, 6, polys)[0] == 2 and 'outside [1, 5]' in _topology(rec, 6, polys)[1]
    assert _topology(rec, 5, polys)[0] == 0
    big = np.tile(rec, (9000, 1))                                         # 36000 corners: 2 * 36000 * 4^4 > 2^24
    rc, why, _ = _topology(big, 5, np.tile(polys, 9000))
    assert rc == 3 and 'too many faces' in why
    rc, _, got = _topology(np.zeros((0, 8), np.float32), 2, np.zeros(0, np.int32))
    assert rc == 0 and got['counts'].tolist() == [[0, 0, 0]] * 3 and got['faces'].shape == (0, 3)
    from ptina_amd import _lib
    with pytest.raises(ValueError, match='creases must hold 4 values'):
        _lib.subdiv_topology_cc(rec, 1, polys, np.zeros(6))


# ---------------------------------------------------------------- the words are what they were
def _loop_digest():
    '''sha256 over the blocks of words mpt_subdiv_topology and mpt_subdiv_topology_creased give for test_subdiv_cpu's and
    test_subdiv_crease_cpu's fixtures at levels 1 to 3'''
    from ptina_amd import _lib
    h = hashlib.sha256()
    for name in subdiv_ref.NAMES:
        for levels in LEVELS:
            rc, words, got = _lib.subdiv_topology_creased(subdiv_ref.fixture(name), levels)
            assert rc == 0
            h.update(np.ascontiguousarray(words, np.int32).tobytes())
            rc, _, plain = _lib.subdiv_topology(subdiv_ref.fixture(name), levels)
            assert rc == 0 and np.array_equal(plain['faces'], got['faces'])
            h.update(np.ascontiguousarray(plain['faces'], np.int32).tobytes())
    for name in subdiv_crease_ref.NAMES:
        for levels in LEVELS:
            rc, words, _ = _lib.subdiv_topology_creased(*((subdiv_crease_ref.fixture(name)[0], levels) + subdiv_crease_ref.fixture(name)[1:]))
            assert rc == 0
            h.update(np.ascontiguousarray(words, np.int32).tobytes())
    return h.hexdigest()


def _cc_digest():
    '''sha256 over the whole blocks of words mpt_subdiv_topology_cc gives for every fixture of subdiv_cc_ref at levels 1 to 3 (the
    tables compared above do not pin the order of the rings inside the block; this does)'''
    h = hashlib.sha256()
    for name in ref.NAMES + ref.CREASED:
        rec, polys, creases, corners = ref.fixture(name)
        for levels in LEVELS:
            rc, words, _ = _topology(rec, levels, polys, creases, corners)
            assert rc == 0
            h.update(np.ascontiguousarray(words, np.int32).tobytes())
    return h.hexdigest()


def test_loop_topologies_are_word_for_word_what_they_were():
    '''LOOP_DIGEST was recorded on the commit before Catmull-Clark, CC_DIGEST on the commit before the two schemes shared one level
    builder and one set of crease rules; the tables are also still the Loop restatements' '''
    assert _loop_digest() == LOOP_DIGEST
    assert _cc_digest() == CC_DIGEST
    from ptina_amd import _lib
    for name in subdiv_ref.NAMES:
        rc, _, got = _lib.subdiv_topology(subdiv_ref.fixture(name), 2)
        want = subdiv_ref.fixture_topology(name, 2)
        assert rc == 0 and got['rules'][2] == want['rules'][2] and got['rings'] == want['rings'] and np.array_equal(got['faces'], want['faces'])
    for name in subdiv_crease_ref.NAMES:
        rc, _, got = _lib.subdiv_topology_creased(*((subdiv_crease_ref.fixture(name)[0], 2) + subdiv_crease_ref.fixture(name)[1:]))
        want = subdiv_crease_ref.fixture_topology(name, 2)
        assert rc == 0 and [_rule(r) for r in got['rules'][2]] == [_rule(r) for r in want['rules'][2]] and np.array_equal(got['faces'], want['faces'])
        assert not any(r[1] & ref.CC for l in got['rules'] for r in got['rules'][l])
    # and the new entry point is another function: the same triangles as polygons of their own are another surface
    rec = subdiv_ref.fixture('octahedron')
    rc, words, got = _topology(rec, 2)
    assert rc == 0 and any(r[1] & ref.CC for r in got['rules'][1]) and got['counts'][:, 2].tolist() == [8, 24, 96]
    assert _lib.subdiv_topology(rec, 2)[2]['counts'][:, 2].tolist() == [8, 32, 128]


LOOP_DIGEST = '30519cbaf5cfea60411fa968f07115e83bfdbe0aa17fc93f2cace02f2839af70'
CC_DIGEST = '84ac9de44e6ebf252bd8dbac00285821fa04b762ad3133e3c0336a779278aa6e'


# ---------------------------------------------------------------- the rules under the host sanitizers
def test_rule_check_program_builds_and_passes(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'subdiv_rule_check')
    subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'subdiv_rule_check.cpp'),
                    '-o', exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.splitlines() == ['subdiv_rule_check: 36 topologies, 72 creased, 19 refusals, 0 failures',
                                       'subdiv_rule_check: Catmull-Clark: 48 topologies, 96 creased, 19 refusals']


# ---------------------------------------------------------------- the restatement against what is known by hand
def _ulps(a, b):
    '''the distance in f32 ulps between f64 values rounded to f32 (finite, of one sign or zero)'''
    a, b = np.asarray(a, np.float64).astype(np.float32), np.asarray(b, np.float64).astype(np.float32)
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))   # noqa: E731
    return np.abs(key(a) - key(b))


def test_restatement_on_the_hand_computed_cube():
    '''level 1 of the cube with corners at +-1: face points (+-1, 0, 0) ..., edge points (+-0.75, +-0.75, 0) ..., vertex points
    (+-5/9, +-5/9, +-5/9), to 1 f32 ulp'''
    rec, polys, _, _ = ref.fixture('cube')
    rc, _, tables = _topology(rec, 1, polys)                               # (the library's tables, the restatement's arithmetic)
    assert rc == 0
    topo = ref.fixture_topology('cube', 1)
    P0, P1 = ref.positions(rec, tables)
    assert np.array_equal(P1, ref.fixture_positions('cube', 1)[1])
    assert topo['counts'].tolist() == [[8, 12, 6], [26, 48, 24]] and P1.shape == (26, 3)
    assert np.array_equal(np.abs(P0), np.ones((8, 3)))
    assert (_ulps(P1[:8], np.sign(P0) * (5.0 / 9.0)) <= 1).all()
    for e in range(12):
        a, b = topo['rules'][1][8 + e][2][:2]
        want = np.where(P0[a] == P0[b], 0.75 * P0[a], 0.0)
        assert (_ulps(P1[8 + e], want) <= 1).all() and (want == 0).sum() == 1
    faces = set()
    for f in range(6):
        corners = P0[topo['rules'][1][20 + f][2]]
        want = np.where((corners == corners[0]).all(axis=0), corners[0], 0.0)
        assert (_ulps(P1[20 + f], want) <= 1).all() and (np.abs(want) == 1).sum() == 1
        faces.add(tuple(want.tolist()))
    assert len(faces) == 6
    out = ref.fixture_subdivided('cube', 1)
    assert out.shape == (144, 8) and np.array_equal(out[:, :3], P1[topo['faces'].reshape(-1)].astype(np.float32))


def test_fan_writes_the_mesh_the_scheme_reads_and_the_uvs_go_down_by_hand():
    '''tools.polys.fan: triangle i of polygon (c_0 .. c_n-1) is (c_0, c_i+1, c_i+2), texcoords per vertex or per polygon corner;
    and one quad with the unit square for uvs, one level: the four child quads' uvs by hand, emitted as (0, 1, 2), (0, 2, 3)'''
    from ptina_amd.tools.polys import fan
    p = np.float32([(0, 0, 0), (2, 0, 0), (2, 2, 1), (0, 2, 0), (-1, 1, 0)])
    t = np.float32([(0, 0), (1, 0), (1, 1), (0, 1), (0.5, 0.5)])
    rec, polys = fan([(0, 1, 2, 3), (0, 3, 4)], p, t=t)
    assert rec.dtype == np.float32 and rec.shape == (9, 8) and polys.dtype == np.int32 and polys.tolist() == [4, 3]
    corners = [0, 1, 2, 0, 2, 3, 0, 3, 4]
    assert np.array_equal(rec[:, :3], p[corners]) and np.array_equal(rec[:, 6:8], t[corners]) and np.array_equal(rec[:, 3:6], np.tile(np.float32([0, 0, 1]), (9, 1)))
    seam = fan([(0, 1, 2, 3), (0, 3, 4)], p, t=[t[:4], t[[0, 3, 4]] + np.float32(0.25)])[0]
    assert np.array_equal(seam[:6], rec[:6]) and np.array_equal(seam[6:, 6:8], rec[6:, 6:8] + np.float32(0.25))
    rc, _, got = _topology(rec, 1, polys)
    assert rc == 0 and ref.cage(rec, polys)[0] == [[0, 1, 2, 3], [0, 3, 4]]
    assert got['quads1'].tolist() == [[0, 4 | i << 8] for i in range(4)] + [[2, 3 | i << 8] for i in range(3)]
    with pytest.raises(ValueError, match='polygon 1 has 2 corners'):
        fan([(0, 1, 2), (0, 3)], p)
    with pytest.raises(ValueError, match='names a vertex outside'):
        fan([(0, 1, 5)], p)
    one, polys = fan([(0, 1, 2, 3)], p, t=t)
    uv = ref.face_uvs(one, ref.topology(one, 1, polys))
    quads = [[(0, 0), (0.5, 0), (0.5, 0.5), (0, 0.5)], [(1, 0), (1, 0.5), (0.5, 0.5), (0.5, 0)], [(1, 1), (0.5, 1), (0.5, 0.5), (1, 0.5)],
             [(0, 1), (0, 0.5), (0.5, 0.5), (0.5, 1)]]
    want = []
    for q in quads:
        want += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    assert uv.tolist() == [[list(map(float, c)) for c in tri] for tri in want]
    two = ref.face_uvs(one, ref.topology(one, 2, polys))
    assert two.shape == (32, 3, 2) and two[0].tolist() == [[0, 0], [0.25, 0], [0.25, 0.25]] and two[1].tolist() == [[0, 0], [0.25, 0.25], [0, 0.25]]


def _insert_knots(Z):
    '''one level of knot insertion of the uniform cubic B-spline along axis 0: masks [1, 6, 1] / 8 and [1, 1] / 2 (an end keeps
    its value: what the comparison stays away from)'''
    n = Z.shape[0] - 1
    out = np.empty((2 * n + 1,) + Z.shape[1:], np.float64)
    out[0], out[-1] = Z[0], Z[-1]
    out[2:-1:2] = (Z[:-2] + 6.0 * Z[1:-1] + Z[2:]) / 8.0
    out[1::2] = (Z[:-1] + Z[1:]) / 2.0
    return out


@pytest.mark.parametrize('levels', LEVELS)
def test_restatement_is_the_bicubic_b_spline_where_the_grid_is_regular(levels):
    '''an open 8 x 8-quad grid with exact regular x and y and random z: refined by separable 1-D knot insertion, compared at every
    level-L vertex at least two cage cells from the boundary (the boundary rules reach less than 1 + 1/2 + 1/4 cells inward), matched
    by its (x, y).  Two f64 computations that differ by rounding only: at most 1 f32 ulp apart after the one rounding'''
    g = np.random.default_rng(11)
    Z = g.uniform(-1, 1, (9, 9)).astype(np.float32).astype(np.float64)   # [x, y]: values the mesh's f32 records hold exactly
    verts = [(x, y, Z[x, y]) for y in range(9) for x in range(9)]
    polygons = [(y * 9 + x, y * 9 + x + 1, (y + 1) * 9 + x + 1, (y + 1) * 9 + x) for y in range(8) for x in range(8)]
    rec, polys = ref.fan_records(verts, polygons)
    rc, _, tables = _topology(rec, levels, polys)                          # (the library's tables, the restatement's arithmetic)
    assert rc == 0
    P = ref.positions(rec, tables)[-1]
    assert np.array_equal(P, ref.positions(rec, ref.topology(rec, levels, polys))[-1])
    for _ in range(levels):
        Z = _insert_knots(_insert_knots(Z).transpose(1, 0)).transpose(1, 0)
    h = 2 ** levels
    assert Z.shape == (8 * h + 1, 8 * h + 1) and P.shape[0] == Z.size
    inner = ((P[:, :2] >= 2) & (P[:, :2] <= 6)).all(axis=1)
    assert inner.sum() == (4 * h + 1) ** 2
    ij = P[inner, :2] * h
    assert np.array_equal(ij, np.round(ij))                              # exact dyadic x and y
    want = Z[ij[:, 0].astype(int), ij[:, 1].astype(int)]
    d = _ulps(P[inner, 2], want)
    print('level %d: %d vertices, largest distance %d ulp' % (levels, inner.sum(), d.max()))
    assert d.max() <= 1

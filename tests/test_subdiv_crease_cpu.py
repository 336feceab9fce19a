'''
CPU tests of semi-sharp creases, corners and hard edges of Loop subdivision: the pure function
mpt_subdiv_topology_creased (no context, no GPU), decoded by the documented layout, against the numpy restatement the GPU tests
hold the kernels to (tests/subdiv_crease_ref.py), and the restatement against what can be worked out by hand.
'''

import ctypes as C

import numpy as np
import pytest

import subdiv_ref
import subdiv_crease_ref as ref

LEVELS = (1, 2, 3)
INF = float('inf')


def _topology(rec, levels, creases=None, corners=None):
    from ptina_amd import _lib
    return _lib.subdiv_topology_creased(rec, levels, creases, corners)


def _plain_words(rec, levels):
    '''the block of mpt_subdiv_topology, its counts and its nine offsets'''
    from ptina_amd import _lib
    lib = _lib.load_library()
    rec = np.ascontiguousarray(rec, np.float32)
    counts, off, need = np.zeros((levels + 1, 3), np.int64), np.zeros(9, np.int32), C.c_int64(0)
    cp = counts.ctypes.data_as(C.POINTER(C.c_int64))
    assert lib.mpt_subdiv_topology(_lib.fptr(rec), rec.shape[0] // 3, levels, cp, _lib.iptr(off), None, 0, C.byref(need), None, 0) == 0
    w = np.zeros(int(need.value), np.int32)
    assert lib.mpt_subdiv_topology(_lib.fptr(rec), rec.shape[0] // 3, levels, cp, _lib.iptr(off), _lib.iptr(w), w.size, C.byref(need), None, 0) == 0
    return w, counts, off


def _same_rules(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[:3] == tuple(w[:3]), (i, g, w)
        # the parameter: the same f64, bit for bit
        assert (g[3] is None) == (w[3] is None) and (g[3] is None or np.float64(g[3]).tobytes() == np.float64(w[3]).tobytes()), (i, g, w)


# ---------------------------------------------------------------- the topology function against the restatement
@pytest.mark.parametrize('name', ref.NAMES)
def test_topology_tables_equal_the_restatement(name):
    '''counts, first corners, every level's kinds, variants, ids and parameters, the whole rings, the sectors and the faces'''
    rec, creases, corners = ref.fixture(name)
    for levels in LEVELS:
        rc, words, got = _topology(rec, levels, creases, corners)
        assert rc == 0
        want = ref.fixture_topology(name, levels)
        assert np.array_equal(got['counts'], want['counts'])
        assert np.array_equal(got['first_corner'], want['first_corner'])
        for l in range(1, levels + 1):
            _same_rules(got['rules'][l], want['rules'][l])
        assert got['rings'] == want['rings'], (name, levels)
        assert got['records'] == [tuple(r) for r in want['records']], (name, levels)
        assert np.array_equal(got['faces'], want['faces'])
        assert got['offsets'][9] > 0 and got['offsets'][10] == len(want['records']) and got['offsets'][8] == words.size
        # a record's vertex is the corner's own, and every face lies in the sector of each of its corners
        vert = np.array([r[0] for r in got['records']])
        assert np.array_equal(vert[got['faces']], want['vfaces'])
        for (r0, r1, r2), (v0, v1, v2) in zip(got['faces'].tolist(), want['vfaces'].tolist()):
            for r, a, b in ((r0, v1, v2), (r1, v2, v0), (r2, v0, v1)):
                ids = got['records'][r][2]
                pairs = list(zip(ids, ids[1:])) + ([(ids[-1], ids[0])] if got['records'][r][1] == ref.VERT_INT else [])
                assert (a, b) in pairs


def _grid_ids():
    '''the control vertex id of every vertex of subdiv_ref.grid() as it is indexed there'''
    welded, _ = subdiv_ref.weld(ref.fixture('grid_line')[0])
    return dict(zip(np.array(subdiv_ref.grid()[1]).reshape(-1).tolist(), welded.reshape(-1).tolist()))


def test_the_fixtures_cover_what_they_are_for():
    count = lambda name, levels, l, kind, variant: sum(r[0] == kind and r[1] == variant for r in ref.fixture_topology(name, levels)['rules'][l])   # noqa: E731
    # the cube at 1.5: sharp, then fractional, then smooth; no edge is hard at L = 2, 3
    assert count('cube_1p5', 3, 1, ref.EDGE_BND, ref.PLAIN) == 12 and count('cube_1p5', 3, 1, ref.VERT_INT, ref.FIXED) == 8
    assert count('cube_1p5', 3, 2, ref.EDGE_INT, ref.BLEND_EDGE) == 24 and count('cube_1p5', 3, 2, ref.VERT_INT, ref.BLEND_CORNER) == 8
    assert count('cube_1p5', 3, 2, ref.VERT_INT, ref.BLEND_CREASE) == 12
    assert all(r[1] == ref.PLAIN and r[0] in (ref.VERT_INT, ref.EDGE_INT) for r in ref.fixture_topology('cube_1p5', 3)['rules'][3])
    assert len(ref.fixture_topology('cube_1p5', 1)['records']) > ref.fixture_topology('cube_1p5', 1)['counts'][1, 0]
    for levels in (2, 3):
        t = ref.fixture_topology('cube_1p5', levels)
        assert len(t['records']) == t['counts'][levels, 0] and all(kind == ref.VERT_INT for _, kind, _ in t['records'])
    # the cube at inf: a corner has three sectors, a vertex on an edge two
    t = ref.fixture_topology('cube_inf', 2)
    per = np.bincount([r[0] for r in t['records']])
    assert (per[:8] == 3).all() and sorted(set(per.tolist())) == [1, 2, 3]
    # the dart: both ends of the one sharp edge take the smooth rule, and have one open sector of all their faces at L = 1
    t = ref.fixture_topology('octa_dart', 1)
    assert [r[:2] for r in t['rules'][1][:6]] == [(ref.VERT_INT, ref.PLAIN)] * 6 and count('octa_dart', 1, 1, ref.EDGE_BND, ref.PLAIN) == 1
    assert t['records'][0][1] == ref.VERT_BND and len(t['records'][0][2]) == 5 and t['records'][0][2][0] == t['records'][0][2][-1]
    assert len(t['records']) == t['counts'][1, 0] + 1                     # (the vertex of the sharp edge has two sectors)
    # the fan: k = 3, f = ((0.5 + 1) + 2.5) / 3 at level 1 -- fixed --, then ((0 + 0) + 1.5) -> k = 1: smooth
    t = ref.fixture_topology('fan7_spokes', 3)
    assert t['rules'][1][0][:2] == (ref.VERT_INT, ref.FIXED) and t['rules'][2][0][:2] == (ref.VERT_INT, ref.PLAIN)
    # ... and a fractional corner with an ordered sum where the three are 0.25, 0.5 and 1.5
    verts, faces = subdiv_ref.bipyramid(7)
    t = ref.topology(subdiv_ref.mesh_records(verts, faces), 1, ref.edge_creases(faces, {(0, 3): 0.25, (0, 5): 0.5, (0, 8): 1.5}))
    assert t['rules'][1][0][:2] == (ref.VERT_INT, ref.BLEND_CORNER) and t['rules'][1][0][3] == ((0.25 + 0.5) + 1.5) / 3.0
    # the grid's line: interior vertices of two sharp edges, and boundary vertices the line makes corners
    t, w = ref.fixture_topology('grid_line', 1), _grid_ids()
    assert [t['rules'][1][w[v]][:2] for v in (2, 32)] == [(ref.VERT_INT, ref.FIXED)] * 2
    for v in (8, 14):
        kind, variant, ids, _ = t['rules'][1][w[v]]
        assert (kind, variant) == (ref.VERT_BND, ref.PLAIN) and sorted(ids) == sorted((w[v - 6], w[v + 6]))
    assert t['rules'][1][w[0]][:2] == (ref.VERT_BND, ref.PLAIN) and ref.fixture_topology('grid_corners', 1)['rules'][1][w[0]][:2] == (ref.VERT_INT, ref.FIXED)
    assert ref.fixture_subdivided('grid_line', 3).shape == (9600, 8) and ref.fixture_subdivided('cube_inf', 2).shape == (576, 8)
    # the edge two faces state differently takes the larger: sharp at level 1 (2 >= 1), where 0.25 would blend
    t = ref.fixture_topology('octa_two', 1)
    assert count('octa_two', 1, 1, ref.EDGE_BND, ref.PLAIN) == 4 and count('octa_two', 1, 1, ref.EDGE_INT, ref.BLEND_EDGE) == 0


def test_the_fan_has_a_fractional_corner_with_an_ordered_sum():
    '''spokes at 0.5, 1 and 2.5: at level 2 they are 0, 0 and 1.5 -- one sharp edge, smooth; stated a level up they blend'''
    verts, faces = subdiv_ref.bipyramid(7)
    rec = subdiv_ref.mesh_records(verts, faces)
    creases = ref.edge_creases(faces, {(0, 3): 0.1, (0, 5): 0.7, (0, 8): 0.3})
    rc, _, got = _topology(rec, 1, creases)
    want = ref.topology(rec, 1, creases)
    assert rc == 0 and got['rules'][1][0][:2] == (ref.VERT_INT, ref.BLEND_CORNER)
    f32 = lambda x: float(np.float32(x))                                  # noqa: E731
    ring = want['rules'][1][0][2]
    welded, _ = subdiv_ref.weld(rec)
    w = dict(zip(np.array(faces).reshape(-1).tolist(), welded.reshape(-1).tolist()))
    assert w[0] == 0
    stated = {w[3]: 0.1, w[5]: 0.7, w[8]: 0.3}
    order = [f32(stated[r]) for r in ring if r in stated]
    assert got['rules'][1][0][3] == ((order[0] + order[1]) + order[2]) / 3.0 == want['rules'][1][0][3]


@pytest.mark.parametrize('name', subdiv_ref.NAMES)
def test_zero_creases_give_todays_words(name):
    '''all-zero sharpnesses and no flag, stated or left out: the block of mpt_subdiv_topology, word for word, and its counts'''
    rec = subdiv_ref.fixture(name)
    k = rec.shape[0] // 3
    for levels in LEVELS:
        plain, counts, off = _plain_words(rec, levels)
        for creases, corners in ((None, None), (np.zeros((k, 3), np.float32), np.zeros((k, 3), bool)), (np.full((k, 3), -0.0, np.float32), None)):
            rc, words, got = _topology(rec, levels, creases, corners)
            assert rc == 0 and np.array_equal(words, plain)
            assert np.array_equal(got['counts'], counts) and np.array_equal(got['offsets'][:9], off)
            assert got['offsets'][9] == 0 and got['offsets'][10] == counts[levels, 0]
        want = subdiv_ref.fixture_topology(name, levels)
        assert [(kind, ids) for kind, _, ids, _ in got['rules'][levels]] == want['rules'][levels]
        assert got['records'] == [(v, kind, ids) for v, (kind, ids) in enumerate(want['rings'])]
        mine = ref.topology(rec, levels)
        assert np.array_equal(mine['faces'], want['faces']) and mine['rings'] == want['rings']


# ---------------------------------------------------------------- refusals
def test_refusals_name_the_face_and_the_edge():
    rec, creases, _ = ref.fixture('octa_dart')
    for value, words in ((-0.5, 'is negative'), (-INF, 'is negative'), (float('nan'), 'is not a number')):
        bad = creases.copy()
        bad[5, 2] = value
        rc, why, got = _topology(rec, 2, bad)
        assert rc == 9 and got is None and why == 'subdivision: the crease of edge 2 of face 5 %s' % words, why
        with pytest.raises(ref.Refusal) as e:
            ref.topology(rec, 2, bad)
        assert e.value.kind == 'crease' and 'the crease of edge 2 of face 5 %s' % words in str(e.value)
    # what mpt_subdiv_topology refuses is refused in its words
    from ptina_amd import _lib
    assert _topology(rec, 0, creases)[:2] == _lib.subdiv_topology(rec, 0)[:2] == (2, 'subdivision: levels 0 outside [1, 5]')
    broken = rec.copy()
    broken[4, 1] = np.nan
    assert _topology(broken, 1, creases)[:2] == (4, 'subdivision: the position of corner 1 of face 1 is not finite')
    # the first bad value in face order is the one named
    bad = creases.copy()
    bad[6, 0], bad[3, 1] = -1.0, np.nan
    assert _topology(rec, 1, bad)[1] == 'subdivision: the crease of edge 1 of face 3 is not a number'


# ---------------------------------------------------------------- checks that do not need the restatement's rules
def _positions_by_the_library_tables(name, levels):
    '''the f64 positions of every level by the LIBRARY's decoded tables (the arithmetic is the restatement's)'''
    rec, creases, corners = ref.fixture(name)
    rc, _, got = _topology(rec, levels, creases, corners)
    assert rc == 0
    return ref.positions(rec, got), got


def test_inf_cube_stays_a_cube():
    '''every vertex of every level lies on the cube, and the eight corners do not move'''
    P, got = _positions_by_the_library_tables('cube_inf', 3)
    corners = P[0].copy()
    assert sorted(map(tuple, corners.tolist())) == sorted((x, y, z) for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0))
    for p in P:
        assert np.array_equal(p[:8], corners)
        assert (np.abs(p).max(axis=1) == 1.0).all() and (np.abs(p) <= 1.0).all()
    # every face of the last level lies in one face of the cube
    vert = np.array([r[0] for r in got['records']])
    tri = P[-1][vert[got['faces']]]                                       # [F,3,3]
    assert ((np.abs(tri) == 1.0).all(axis=1)).any(axis=1).all()


def test_flagged_grid_corners_do_not_move():
    P, _ = _positions_by_the_library_tables('grid_corners', 3)
    Q, _ = _positions_by_the_library_tables('grid_line', 3)
    w = _grid_ids()
    for v in (w[0], w[5], w[30], w[35]):
        assert all(np.array_equal(p[v], P[0][v]) for p in P)
        assert not np.array_equal(Q[1][v], Q[0][v])                       # (unflagged, the corner shrinks)
    # the ends of the crease line are corners too: a crease that reaches the boundary
    for v in (w[2], w[32]):
        assert all(np.array_equal(p[v], P[0][v]) for p in P) and all(np.array_equal(q[v], Q[0][v]) for q in Q)


def test_blender_crease():
    from ptina_amd.tools.crease import blender_crease
    got = blender_crease([0.0, 0.5, 0.999, 1.0, 2.0])
    assert got.dtype == np.float32 and got[:2].tolist() == [0.0, 2.5] and got[2] == np.float32(0.999) * np.float32(0.999) * np.float32(10)
    assert got[3:].tolist() == [INF, INF] and blender_crease(1.0) == INF and blender_crease(0.3) == np.float32(0.3) * np.float32(0.3) * np.float32(10)

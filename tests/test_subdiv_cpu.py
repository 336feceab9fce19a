'''
CPU tests of Loop subdivision: the pure functions of the host runtime (mpt_subdiv_topology, mpt_subdiv_plan:
no context, no GPU) against the independent numpy restatement the GPU tests hold the kernels to (tests/subdiv_ref.py), and the
restatement itself against what can be worked out by hand.
'''

import numpy as np
import pytest

import subdiv_ref

u32 = np.uint32
LEVELS = (1, 2, 3)


def _topology(rec, levels):
    from ptina_amd import _lib
    return _lib.subdiv_topology(rec, levels)


# ---------------------------------------------------------------- the topology function against the restatement
@pytest.mark.parametrize('name', subdiv_ref.NAMES)
def test_topology_tables_equal_the_restatement(name):
    '''counts, first corners, rule kinds, ring order and ids of every level, the last level's rings and faces: exactly'''
    for levels in LEVELS:
        rc, why, got = _topology(subdiv_ref.fixture(name), levels)
        assert rc == 0 and why == ''
        want = subdiv_ref.fixture_topology(name, levels)
        assert np.array_equal(got['counts'], want['counts']), (name, levels, got['counts'], want['counts'])
        assert np.array_equal(got['first_corner'], want['first_corner'])
        for l in range(1, levels + 1):
            assert got['rules'][l] == want['rules'][l], (name, levels, l)
        assert got['rings'] == want['rings'], (name, levels)
        assert np.array_equal(got['faces'], want['faces'])
        k = subdiv_ref.fixture(name).shape[0] // 3
        assert got['counts'][:, 2].tolist() == [k * 4 ** l for l in range(levels + 1)]


@pytest.mark.parametrize('name', subdiv_ref.CLOSED)
def test_closed_meshes_keep_eulers_number(name):
    rc, _, got = _topology(subdiv_ref.fixture(name), 3)
    assert rc == 0
    for V, E, F in got['counts'].tolist():
        assert V - E + F == 2, (name, V, E, F)
    assert all(kind == subdiv_ref.VERT_INT for kind, _ in got['rings'])
    for V, E, F in subdiv_ref.fixture_topology(name, 3)['counts'].tolist():
        assert V - E + F == 2


def test_the_fixtures_cover_what_they_are_for():
    '''valence 3, 7 and 12; boundary vertices, two corners of valence 2 and regular interior vertices; a uv seam in every mesh'''
    val = lambda name: sorted(len(r) for k, r in subdiv_ref.fixture_topology(name, 1)['rules'][1] if k == subdiv_ref.VERT_INT)   # noqa: E731
    assert set(val('tetrahedron')) == {3} and val('fan7')[-2:] == [7, 7] and val('fan12')[-2:] == [12, 12]
    rules = subdiv_ref.fixture_topology('grid', 1)['rules'][1]
    bnd = [len(r) for k, r in rules if k == subdiv_ref.VERT_BND]
    assert len(bnd) == 20 and sorted(bnd)[:2] == [2, 2] and val('grid') == [6] * 16
    assert sum(k == subdiv_ref.EDGE_BND for k, _ in rules) == 20
    for name in subdiv_ref.NAMES:
        rec = subdiv_ref.fixture(name)
        faces, _ = subdiv_ref.weld(rec)
        uv_of = {}
        for s, v in enumerate(faces.reshape(-1)):
            uv_of.setdefault(int(v), set()).add(tuple(rec[s, 6:8].tolist()))
        if name != 'triangle':                                          # (a lone triangle shares no vertex: nothing to seam)
            assert any(len(x) > 1 for x in uv_of.values()), name + ' has no uv seam'
        assert rec.shape[0] // 3 == faces.shape[0]
    assert subdiv_ref.fixture('grid').shape[0] == 150 and subdiv_ref.fixture_subdivided('grid', 3).shape == (9600, 8)


def test_negative_zero_welds_with_zero():
    rec = subdiv_ref.fixture('pair').copy()
    zeros = np.flatnonzero((rec[:, :3] == 0).all(axis=1))                # the two corners on vertex 0
    assert zeros.tolist() == [0, 3] and not np.signbit(rec[0, 0])
    rec[3, 0] = np.float32(-0.0)
    assert np.signbit(rec[3, 0])
    rc, _, got = _topology(rec, 2)
    want = subdiv_ref.fixture_topology('pair', 2)
    assert rc == 0 and np.array_equal(got['faces'], want['faces']) and np.array_equal(got['first_corner'], want['first_corner'])
    assert np.array_equal(subdiv_ref.topology(rec, 2)['faces'], want['faces'])


# ---------------------------------------------------------------- refusals
def _tri(*pts):
    return subdiv_ref.mesh_records(np.array(pts, np.float32).reshape(-1, 3), np.arange(len(pts)).reshape(-1, 3), seam=1)


A, B, C, D, E, F = (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (2, 0, 1)
REFUSALS = {
    'finite': (4, 'not finite', lambda: _bad_position()),
    'degenerate': (5, 'two corners on one vertex', lambda: _tri(A, B, C, A, D, A)),
    'edge_faces': (6, 'third on the edge', lambda: _tri(A, B, C, B, A, D, A, B, E)),
    'edge_direction': (7, 'same direction', lambda: _tri(A, B, C, A, B, D)),
    'fan': (8, 'not one fan', lambda: _tri(A, B, C, A, D, E)),
}


def _bad_position():
    rec = subdiv_ref.fixture('pair').copy()
    rec[4, 1] = np.inf
    return rec


@pytest.mark.parametrize('kind', sorted(REFUSALS))
def test_every_refusal_fires_with_its_words(kind):
    code, words, make = REFUSALS[kind]
    rec = make()
    rc, why, got = _topology(rec, 2)
    assert rc == code and got is None and why.startswith('subdivision: ') and words in why, (rc, why)
    with pytest.raises(subdiv_ref.Refusal) as e:
        subdiv_ref.topology(rec, 2)
    assert e.value.kind == kind
    if kind == 'finite':
        assert 'corner 1 of face 1' in why
    if kind == 'degenerate':
        assert 'face 1' in why
    if kind == 'fan':
        assert 'vertex 0' in why


def test_levels_and_sizes_are_refused():
    rec = subdiv_ref.fixture('triangle')
    assert _topology(rec, 0)[0] == 2 and _topology(rec, 6)[0] == 2 and 'outside [1, 5]' in _topology(rec, 6)[1]
    assert _topology(rec, 5)[0] == 0
    big = np.tile(subdiv_ref.fixture('triangle'), (20000, 1))
    rc, why, _ = _topology(big, 5)
    assert rc == 3 and 'too many faces' in why
    rc, _, got = _topology(np.zeros((0, 8), np.float32), 2)             # k = 0 is a mesh and stays one
    assert rc == 0 and got['counts'].tolist() == [[0, 0, 0]] * 3 and got['faces'].shape == (0, 3)


# ---------------------------------------------------------------- the launch plan
def test_plan_equals_a_numpy_plan():
    from ptina_amd import _lib
    g = np.random.default_rng(3)
    sizes = [0, 1, 255, 256, 257, 512, 1000, 9600]
    for _ in range(200):
        n = int(g.integers(0, 9))
        items = g.choice(sizes, n)
        dirty = g.integers(0, 2, n) if g.integers(0, 3) else None
        assert _lib.subdiv_plan(items, dirty) == subdiv_ref.plan(items, dirty)
    assert _lib.subdiv_plan([256, 0, 257]) == ([(0, 0), (2, 1)], 3)
    with pytest.raises(ValueError):
        _lib.subdiv_plan([5, -1])


# ---------------------------------------------------------------- the restatement against what is known by hand
def test_restatement_keeps_a_flat_regular_grid():
    '''Loop's regular interior rule reproduces linear functions: a flat grid stays flat, and an interior vertex whose ring is
    regular (valence 6, neighbours symmetric about it) stays put, at every level'''
    verts, faces = subdiv_ref.grid(bump=0.0)
    rec = subdiv_ref.mesh_records(verts, faces)
    topo = subdiv_ref.topology(rec, 2)
    out = subdiv_ref.subdivide(rec, 2, topo)
    assert np.all(out[:, 2] == 0)
    assert np.all(out[:, 3:5] == 0) and np.all(out[:, 5] == 1)          # the normals of a flat, consistently wound sheet
    P0 = rec[topo['first_corner'], :3].astype(np.float64)
    P1 = subdiv_ref.refine(P0, topo['rules'][1])
    P2 = subdiv_ref.refine(P1, topo['rules'][2])
    inner = [v for v, (k, r) in enumerate(topo['rules'][1][:P0.shape[0]]) if k == subdiv_ref.VERT_INT]
    assert len(inner) == 16
    assert np.array_equal(P1[inner], P0[inner]) and np.array_equal(P2[inner], P0[inner])   # (quarters and halves: exact in f64)
    edge = next(i for i, (k, r) in enumerate(topo['rules'][1]) if k == subdiv_ref.EDGE_INT)
    a, b = topo['rules'][1][edge][1][:2]
    assert np.array_equal(P1[edge], 0.5 * (P0[a] + P0[b]))              # on a flat regular grid an edge vertex is the midpoint


def test_restatement_on_a_hand_computed_triangle():
    '''one triangle, one level: vertices 0 1 2, edges (0,1) (0,2) (1,2) -> 3 4 5, four faces, every rule a boundary rule'''
    rec = np.zeros((3, 8), np.float32)
    rec[:, :3] = [(0, 0, 0), (4, 0, 0), (0, 8, 0)]
    rec[:, 6:8] = [(0, 0), (1, 0), (0, 0.5)]
    topo = subdiv_ref.topology(rec, 1)
    assert topo['counts'].tolist() == [[3, 3, 1], [6, 9, 4]]
    assert topo['faces'].tolist() == [[0, 3, 4], [1, 5, 3], [2, 4, 5], [3, 5, 4]]
    assert topo['rules'][1] == [(1, [1, 2]), (1, [2, 0]), (1, [0, 1]), (3, [0, 1]), (3, [0, 2]), (3, [1, 2])]
    out = subdiv_ref.subdivide(rec, 1, topo)
    # corners shrink: 0.75 v + 0.125 (p + q); edge vertices are midpoints
    P = {0: (0.5, 1, 0), 1: (3, 1, 0), 2: (0.5, 6, 0), 3: (2, 0, 0), 4: (0, 4, 0), 5: (2, 4, 0)}
    assert out[:, :3].tolist() == [list(map(float, P[v])) for v in topo['faces'].reshape(-1)]
    assert np.all(out[:, 3:6] == [0, 0, 1])
    uv = {0: (0, 0), 1: (1, 0), 2: (0, 0.5), 3: (0.5, 0), 4: (0, 0.25), 5: (0.5, 0.25)}    # face-varying: corners keep theirs, midpoints between
    assert out[:, 6:8].tolist() == [list(map(float, uv[v])) for v in topo['faces'].reshape(-1)]
    two = subdiv_ref.subdivide(rec, 2)
    assert two.shape == (48, 8) and two[0, 6:8].tolist() == [0, 0] and two[1, 6:8].tolist() == [0.25, 0]

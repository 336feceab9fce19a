'''
GPU tests (-m gpu) of spaced scatters -- a scatter with a minimum distance (ModelPool.add_scatter(min_distance=, candidates=),
set_scatter, scatter_spacing, scatter_spacing_stats; mpt_scatter_set_spacing ... mpt_scatter_space_points;
ptina_amd/csrc/scatter_space.hip, scene_scatter.cpp).

The elimination is a predicate over exact f64 comparisons, so nothing here has a margin: through the door
(mpt_scatter_space_points: the device's grid and round kernels on explicit points) the kept flags are exactly those of
tests/scatter_space_ref.py and the rounds at most its synchronous count; through add_scatter the kept flags and the chosen
candidates equal the restatement run on the restatement's own candidate positions, and records and matrices equal
tests/scatter_ref.py's bit for bit.  Surfaces, helpers and parameter sets are test_scatter_gpu's.  count, M and r of every
add_scatter test are chosen so that, in the restatement alone and asserted at the start of the test, at least `count` candidates
are kept, at least a quarter are rejected and the synchronous form takes at least 3 rounds.
'''

import types

import numpy as np
import pytest

import deform_ref
import scatter_ref as sc
import scatter_space_ref as ss
import subdiv_ref as sr
import test_displace_gpu as dg
from test_scatter_gpu import (IMAGES, TUFT, VARIANTS, _ctx, _kernels, _plain, _points_differ, _pose, _set_pose, _sstats, _start, _sticky_scene, _surface_mesh,
                              _surface_rec, _want, _world, _worlds_differ, _same)

pytestmark = pytest.mark.gpu
GRID_KERNELS = 5                                                          # positions, box, count, scan, fill
BATCH = 8                                                                 # csrc/mpt_types.h MPT_SPACE_BATCH


# ---------------------------------------------------------------- 1: the door
@pytest.fixture(scope='module')
def door_cases():
    '''(name, points, r, kept, rounds): the restatement, once for the module'''
    return [(name, pts, r, *ss.eliminate(pts, r)) for name, pts, r in ss.door_cases()]


def test_door_flags_equal_the_restatement_and_rounds_stay_below_its_count(fresh, door_cases):
    from ptina_amd import _lib
    _start()
    c = _ctx()
    for name, pts, r, kept, rounds in door_cases:
        got, took = _lib.scatter_space_points(c, pts, r)
        print('%s: %d points, %d kept, %d rounds on the device, %d synchronous' % (name, len(pts), int(got.sum()), took, rounds))
        bad = np.flatnonzero(got.astype(bool) != kept)
        assert bad.size == 0, (name, bad[:8])
        assert 1 <= took <= rounds, (name, took, rounds)
    by_name = {name: (pts, r, kept, rounds) for name, pts, r, kept, rounds in door_cases}
    # the chain lies in one wave, whose lanes look together: the device's rounds are the synchronous 40, past the first batch
    pts, r, kept, rounds = by_name['a chain of 40, 0.6 r apart']
    assert rounds == 40 > BATCH and _lib.scatter_space_points(c, pts, r)[1] == 40
    # a second call on other points leaves nothing of the first behind
    pts, r, kept, _ = by_name['257 uniform points']
    assert np.array_equal(_lib.scatter_space_points(c, pts, r)[0].astype(bool), kept)
    assert _lib.scatter_space_points(c, np.zeros((0, 3)), 1.0)[0].size == 0
    for bad in (-1.0, float('nan')):
        with pytest.raises(RuntimeError, match='mpt_scatter_space_points: bad arguments'):
            _lib.scatter_space_points(c, pts, bad)


def test_door_changes_nothing_else_in_the_context(fresh):
    from ptina_amd import _lib
    pool = _start()
    surf = pool.add_object(_plain(pool, 'octahedron'), sc.BENT)
    sid, objs = pool.add_scatter(surf, _plain(pool, TUFT), 16, seed=3, min_distance=0.5, candidates=128)
    pool.compose()
    before = pool.scatter_spacing(sid), pool.scatter_to_numpy(sid), pool.to_numpy()
    stats = [getattr(pool.scatter_spacing_stats(), k) for k, _ in _lib.ScatterSpacingInfo._fields_]
    _kernels()
    pts = np.random.default_rng(5).random((300, 3))
    kept, _ = ss.eliminate(pts, 0.1)
    assert np.array_equal(_lib.scatter_space_points(_ctx(), pts, 0.1)[0].astype(bool), kept)
    after = pool.scatter_spacing(sid), pool.scatter_to_numpy(sid), pool.to_numpy()
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert _same(np.asarray(x), np.asarray(y))
    assert stats == [getattr(pool.scatter_spacing_stats(), k) for k, _ in _lib.ScatterSpacingInfo._fields_] and _kernels() == 0
    pool.compose()
    assert _sstats(pool) == ((0, 0, 0), (0, 0, 0, 0, 0))


# ---------------------------------------------------------------- 2: through add_scatter
def _spaced_want(rec, world, seed, count, m, r, **kw):
    '''the restatement of a spaced scatter: (kept [m], index [count], synchronous rounds, candidate records [m], matrices [count])'''
    cands, _, q = _want(rec, world, seed, m, **kw)
    P = sc.world_corners(rec, world)
    kept, index, rounds, pos = ss.spaced(P, cands, r, count)
    print('restatement: %d of %d candidates kept at r = %g, %d synchronous rounds, count %d' % (kept.sum(), m, r, rounds, count))
    assert kept.sum() >= count and (~kept).mean() >= 0.25 and rounds >= 3, 'precondition: choose another r'
    align = sc.UP if kw.get('align', 'normal') == 'up' else sc.NORMAL
    return kept, index, rounds, cands, sc.place(P, cands[index], align, kw.get('up', (0, 1, 0)))


def _check_spaced(pool, sid, want, count, m, r, what):
    kept, index, rounds, cands, worlds = want
    got_m, got_kept, got_rounds, flags, got_index = pool.scatter_spacing(sid)
    assert (got_m, got_kept) == (m, int(kept.sum())) and 1 <= got_rounds <= rounds, (what, got_m, got_kept, got_rounds, rounds)
    assert np.array_equal(flags, kept), (what, np.flatnonzero(flags != kept)[:8])
    assert np.array_equal(got_index, index), (what, got_index[:8], index[:8])
    points, got_worlds, _ = pool.scatter_to_numpy(sid)
    _points_differ(points, cands[index], what)
    _worlds_differ(got_worlds, worlds, what)
    close = ss.conflicts(got_worlds[:, :3, 3], r)[np.triu_indices(count, 1)]    # the instances' translations, by the rule's own expression
    assert not close.any(), (what, int(close.sum()))
    return points, got_worlds


CASES = [('octahedron', 0, 16, 128, 0.5), ('octahedron', 0, 64, 320, 0.3), ('octahedron', 0, 256, 1200, 0.15),
         ('fan7', 3, 16, 128, 0.3), ('fan7', 3, 64, 320, 0.2), ('fan7', 3, 256, 1200, 0.1)]


@pytest.mark.parametrize('variant', [0, 2])                               # density off / on
@pytest.mark.parametrize('name,levels,count,m,r', CASES)
def test_spaced_scatter_equals_the_restatement_bit_for_bit(fresh, name, levels, count, m, r, variant):
    kw = VARIANTS[variant]
    rec = _surface_rec(name, levels)
    want = _spaced_want(rec, sc.BENT, sc.SEED, count, m, r, **kw)
    if m == 1200:
        assert m > 4 * 256 and m % 256                                    # several workgroups of candidates and a partial last one
    pool = _start()
    dg._load_images(IMAGES)
    surf = pool.add_object(_surface_mesh(pool, name, levels), sc.BENT, 1)
    tuft = _plain(pool, TUFT)
    sid, objs = pool.add_scatter(surf, tuft, count, seed=sc.SEED, mtlid=2, min_distance=r, candidates=m, **kw)
    plain, _ = pool.add_scatter(surf, tuft, m, seed=sc.SEED, mtlid=2, **kw)      # the same seed, M instances, no distance
    assert objs == range(1, 1 + count)
    pool.compose()
    s = pool.scatter_spacing_stats()
    assert _sstats(pool) == ((2, 2, count + m), (1, 3, 1, 1, 1 + s.host_reads))
    assert (s.scatters, s.candidates, s.kept, s.grid_launches, s.compact_launches) == (1, m, int(want[0].sum()), GRID_KERNELS, 1)
    assert s.round_launches % BATCH == 0 and s.rounds <= s.round_launches < s.rounds + BATCH and s.host_reads == s.round_launches // BATCH + 1
    assert _kernels() == 7 + GRID_KERNELS + s.round_launches + 1
    what = '%s at level %d, %d of %d at r = %g, %s' % (name, levels, count, m, r, kw)
    _check_spaced(pool, sid, want, count, m, r, what)
    _points_differ(pool.scatter_to_numpy(plain)[0], want[3], 'the plain scatter of M: the candidates')
    with pytest.raises(RuntimeError, match='scatter %d is a plain scatter' % plain):
        pool.scatter_spacing(plain)
    pool.compose()                                                        # nothing changed: nothing launched
    assert _sstats(pool) == ((0, 0, 0), (0, 0, 0, 0, 0)) and _kernels() == 0 and pool.scatter_spacing_stats().scatters == 0


# ---------------------------------------------------------------- 3: several scatters in one compose
def test_two_spaced_scatters_and_a_plain_one_take_one_launch_of_each_kind(fresh):
    pool = _start()
    dg._load_images(IMAGES)
    rec0, rec1 = _surface_rec('octahedron', 0), _surface_rec('fan7', 3)
    wa = _spaced_want(rec0, sc.BENT, 5, 64, 320, 0.3, **VARIANTS[0])
    wb = _spaced_want(rec1, _world(6), 6, 16, 300, 0.25, **VARIANTS[2])
    s0 = pool.add_object(_surface_mesh(pool, 'octahedron', 0), sc.BENT, 0)
    s1 = pool.add_object(_surface_mesh(pool, 'fan7', 3), _world(6), 1)
    tuft = _plain(pool, TUFT)
    a, _ = pool.add_scatter(s0, tuft, 64, seed=5, min_distance=0.3, candidates=320, **VARIANTS[0])
    p, _ = pool.add_scatter(s1, tuft, 100, seed=7, **VARIANTS[3])
    b, _ = pool.add_scatter(s1, tuft, 16, seed=6, min_distance=0.25, candidates=300, **VARIANTS[2])
    pool.compose()
    s = pool.scatter_spacing_stats()
    assert _sstats(pool) == ((3, 3, 180), (1, 3, 1, 1, 1 + s.host_reads))
    assert (s.scatters, s.candidates, s.kept, s.grid_launches, s.compact_launches) == (2, 620, int(wa[0].sum() + wb[0].sum()), GRID_KERNELS, 1)
    assert s.round_launches % BATCH == 0 and s.round_launches < max(wa[2], wb[2]) + BATCH and s.host_reads == s.round_launches // BATCH + 1
    assert _kernels() == 7 + GRID_KERNELS + s.round_launches + 1
    _check_spaced(pool, a, wa, 64, 320, 0.3, 'the first spaced scatter')
    _check_spaced(pool, b, wb, 16, 300, 0.25, 'the second spaced scatter')
    alone = _want(rec1, _world(6), 7, 100, **VARIANTS[3])
    points, worlds, _ = pool.scatter_to_numpy(p)
    _points_differ(points, alone[0], 'the plain scatter between them')
    _worlds_differ(worlds, alone[1], 'the plain scatter between them')


# ---------------------------------------------------------------- 4: stickiness
def test_spaced_instances_stick_and_later_composes_eliminate_nothing(fresh):
    import displace_ref as dr
    from ptina_amd.things import BVHTree
    from test_scatter_gpu import STICKY_DISP
    pool = _start()
    dg._load_images(IMAGES)
    count, m, r = 64, 320, 0.25
    rig, mesh, surf, other, pose, _, _ = _sticky_scene(pool, 8)
    rec = dg._expected('cylinder', 2, STICKY_DISP, rig, pose)
    want = _spaced_want(rec, _world(21), 9, count, m, r, scale=(0.03, 0.08))
    sid, objs = pool.add_scatter(surf, _plain(pool, TUFT), count, seed=9, mtlid=2, scale=(0.03, 0.08), min_distance=r, candidates=m)
    pool.compose()
    points, worlds = _check_spaced(pool, sid, want, count, m, r, 'posed cylinder')
    spacing = pool.scatter_spacing(sid)
    tree = BVHTree()
    tree.build()
    _kernels()
    pose2 = _pose(43)
    _set_pose(pool, surf, pose2)
    pool.set_displacement(mesh, -0.2)
    pool.compose()
    s = pool.scatter_spacing_stats()
    assert _sstats(pool) == ((0, 2, 8 + count), (0, 0, 0, 1, 0)) and _kernels() == 1
    assert [getattr(s, k) for k in ('scatters', 'candidates', 'kept', 'rounds', 'grid_launches', 'round_launches', 'compact_launches', 'host_reads')] == [0] * 8
    rec2 = dg._expected('cylinder', 2, (1, dr.NORMAL, dr.A, -0.2, 0.45), rig, pose2)
    points2, worlds2, _ = pool.scatter_to_numpy(sid)
    _points_differ(points2, points, 'the records after the edit')
    _worlds_differ(worlds2, sc.place(sc.world_corners(rec2, _world(21)), points), 'the matrices after the edit')
    assert not np.array_equal(worlds2, worlds)
    for x, y in zip(spacing, pool.scatter_spacing(sid)):
        assert np.array_equal(x, y)
    assert tree.update(max_growth=float('inf')) == 'refit'


# ---------------------------------------------------------------- 5: rescatter and the distance
def test_rescatter_and_set_scatter_eliminate_again(fresh):
    pool = _start()
    dg._load_images(IMAGES)
    rec = _surface_rec('fan7', 3)
    count, m, r = 64, 320, 0.2
    w1 = _spaced_want(rec, sc.BENT, 1, count, m, r)
    w2 = _spaced_want(rec, sc.BENT, 2, count, m, r)
    surf = pool.add_object(_surface_mesh(pool, 'fan7', 3), sc.BENT)
    sid, objs = pool.add_scatter(surf, _plain(pool, TUFT), count, seed=1, min_distance=r, candidates=m)
    pool.compose()
    p1, _ = _check_spaced(pool, sid, w1, count, m, r, 'seed 1')
    pool.rescatter(sid, 2)
    with pytest.raises(RuntimeError, match='scatter %d has not been placed yet' % sid):
        pool.scatter_spacing(sid)
    pool.compose()
    assert pool.scatter_spacing_stats().scatters == 1
    p2, _ = _check_spaced(pool, sid, w2, count, m, r, 'seed 2')
    assert not np.array_equal(p1['face'], p2['face'])
    pool.rescatter(sid, 1)
    pool.compose()
    _check_spaced(pool, sid, w1, count, m, r, 'the old seed')
    # the distance goes: the plain scatter's records; and comes back: the spaced ones
    pool.set_scatter(sid, min_distance=0)
    pool.compose()
    assert pool.scatter_spacing_stats().scatters == 0 and _sstats(pool) == ((1, 1, count), (1, 3, 1, 1, 1))
    _points_differ(pool.scatter_to_numpy(sid)[0], w1[3][:count], 'without a distance')
    with pytest.raises(RuntimeError, match='is a plain scatter'):
        pool.scatter_spacing(sid)
    pool.set_scatter(sid, min_distance=r)
    pool.compose()
    _check_spaced(pool, sid, w1, count, m, r, 'with the distance again')
    # other candidates, and a parameter of the plain rule beside the distance
    w3 = _spaced_want(rec, sc.BENT, 1, count, 400, 0.15, scale=(0.5, 0.75))
    pool.set_scatter(sid, min_distance=0.15, candidates=400, scale=(0.5, 0.75))
    pool.compose()
    _check_spaced(pool, sid, w3, count, 400, 0.15, 'other candidates')
    with pytest.raises(ValueError, match='unknown scatter parameters: colour'):
        pool.set_scatter(sid, colour=1)


# ---------------------------------------------------------------- 6: refusals
def test_too_few_kept_refuses_and_leaves_scene_and_model(fresh):
    import query_ref as qr
    import visibility_ref as vr
    from ptina_amd.things import BVHTree
    pool = _start('fast')
    rec = _surface_rec('octahedron', 0)
    count, m, big = 64, 320, 0.6
    cands, _, _ = _want(rec, sc.BENT, 4, m)
    kept, _ = ss.eliminate(ss.positions(sc.world_corners(rec, sc.BENT), cands), big)
    assert 0 < kept.sum() < count
    surf = pool.add_object(_plain(pool, 'octahedron'), sc.BENT)
    tuft = _plain(pool, TUFT)
    first, _ = pool.add_scatter(surf, tuft, 8, seed=2)
    pool.compose()
    tree = BVHTree()
    tree.build()
    model, mtl = pool.to_numpy()
    o, d = qr.rays(vr.positions(model), 4, 64)
    hits = tree.intersect(o, d)
    sid, objs = pool.add_scatter(surf, tuft, count, seed=4, min_distance=big, candidates=m)
    words = r'scatter %d: %d of its %d candidates are kept at the minimum distance 0\.6, fewer than its count %d' % (sid, kept.sum(), m, count)
    for _ in range(2):                                                    # the scatter stays due: the same refusal again
        with pytest.raises(RuntimeError, match=words):
            pool.compose()
    assert _same(pool.to_numpy()[0], model) and np.array_equal(pool.to_numpy()[1], mtl)
    again = tree.intersect(o, d)
    for k in ('hit', 'index', 'object'):
        assert np.array_equal(np.asarray(again[k]), np.asarray(hits[k])), k
    with pytest.raises(RuntimeError, match='scatter %d has not been placed yet' % sid):
        pool.scatter_to_numpy(sid)
    want = _spaced_want(rec, sc.BENT, 4, count, m, 0.3)
    pool.set_scatter(sid, min_distance=0.3)
    pool.compose()
    _check_spaced(pool, sid, want, count, m, 0.3, 'after the refusal')
    _points_differ(pool.scatter_to_numpy(first)[0], _want(rec, sc.BENT, 2, 8)[0], 'the scatter that was there before')
    assert pool.nfaces == 8 + 4 * (8 + count)
    # the arguments of mpt_scatter_set_spacing
    c = _ctx()
    for bad, words in ((-0.5, 'the minimum distance -0.5 is negative or not finite'), (float('inf'), 'the minimum distance inf is negative or not finite'),
                       (float('nan'), 'the minimum distance -?nan is negative or not finite')):
        with pytest.raises(RuntimeError, match='mpt_scatter_set_spacing: scatter %d: %s' % (sid, words)):
            c.call('mpt_scatter_set_spacing', sid, bad, m)
    for bad in (count - 1, 2 ** 24 + 1):
        with pytest.raises(RuntimeError, match=r'mpt_scatter_set_spacing: scatter %d: %d candidates outside \[%d, 16777216\]' % (sid, bad, count)):
            c.call('mpt_scatter_set_spacing', sid, 0.3, bad)
    with pytest.raises(RuntimeError, match='mpt_scatter_set_spacing: unknown scatter 9'):
        c.call('mpt_scatter_set_spacing', 9, 0.3, m)
    with pytest.raises(ValueError, match='negative or not finite'):
        pool.add_scatter(surf, tuft, 4, min_distance=-1.0)
    with pytest.raises(ValueError, match=r'3 candidates outside \[4, 16777216\]'):
        pool.add_scatter(surf, tuft, 4, min_distance=0.1, candidates=3)
    assert pool.scatter_stats().scatters == 2
    pool.compose()
    assert _sstats(pool) == ((0, 0, 0), (0, 0, 0, 0, 0))                  # the refused calls marked nothing


# ---------------------------------------------------------------- 7: the worker facade
def test_worker_facade_passes_the_keywords_through(fresh):
    import threading
    from ptina_amd.common import reset_all
    from ptina_amd.tools.mtworker import DaemonModule, OnDemandProxy
    reset_all()
    seen = []

    def module():
        seen.append(threading.get_ident())
        from ptina_amd import worker
        ns = types.SimpleNamespace(**{k: getattr(worker, k) for k in dir(worker) if not k.startswith('_')})
        ns.add_mesh = lambda name: worker.ModelPool().add_mesh(*deform_ref.split(sr.fixture(name)))
        ns.add_object = lambda mesh: worker.ModelPool().add_object(mesh, sc.BENT)
        ns.fetch = lambda sid: (worker.ModelPool().scatter_to_numpy(sid), worker.ModelPool().scatter_spacing(sid))
        return ns
    count, m, r = 16, 128, 0.5
    want = _spaced_want(sr.fixture('octahedron'), sc.BENT, 12, count, m, r, scale=(0.1, 0.2))
    w = OnDemandProxy(lambda: DaemonModule(module))
    w.init()
    surf = w.add_object(w.add_mesh('octahedron'))
    sid, objs = w.add_scatter(surface=surf, mesh=w.add_mesh(TUFT), count=count, seed=12, scale=(0.1, 0.2), min_distance=r, candidates=m)
    assert seen and seen[0] != threading.get_ident() and objs == range(1, 1 + count)
    w.compose_model()
    (points, worlds, _), (got_m, got_kept, _, flags, index) = w.fetch(sid)
    assert (got_m, got_kept) == (m, int(want[0].sum())) and np.array_equal(flags, want[0]) and np.array_equal(index, want[1])
    _points_differ(points, want[3][want[1]], 'through the worker')
    _worlds_differ(worlds, want[4], 'through the worker')
    w.synchronize()

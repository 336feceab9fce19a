'''
The binary node records and the triangle records on the GPU (-m gpu), downloaded through BVHTree().records()
(mpt_get_records) and held to tests/record_checks.py word for word: no comparison here carries a tolerance.

1  built records over every builder: B1 - B6, N1 and T1 - T3 against the model; the device SAH pass's fnode equals the host
   pass's word for word up to 1024 triangles
2  n = 0 and n = 1                      3  refitted records: every property against the target, the id rows unchanged, the
   round trip's words those of the build, cost_built / cost_now the integers of B6 over the records before / after
4  gpu_build = 0 against 1              5  through load_meshes, set_world, compose and refit
6  the door changes nothing a render reads or writes                7  the door's refusals
8  the exact sweep of SahBuild::split restated in numpy: the id rows of the host and of the device pass, node for node
'''

import ctypes as C

import numpy as np
import pytest

import record_checks as rc
from test_refit_gpu import _moved_model, _set_builder
from test_tree_invariants_gpu import BUILDERS, _random_model

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
SIZES = [2, 3, 5, 33, 65, 300, 1025, 2049]
ARRAYS = ('snode', 'fnode', 'tgeo', 'tshade', 'tfast')


def _things():
    from ptina_amd.things import init_things
    from ptina_amd.common import ctx
    init_things()
    return ctx()


def _load(v, m):
    from ptina_amd.things import ModelPool
    ModelPool().load(v, m)


def _tree():
    from ptina_amd.things import BVHTree
    return BVHTree()


def _specified(rec):
    '''the records with the two unspecified words of fnode's id row zeroed: what two builders must agree on'''
    out = {k: np.array(rec[k], copy=True) for k in ARRAYS}
    out['fnode'][:, 3, 2:4] = 0
    return out


def _same(a, b, what):
    a, b = _specified(a), _specified(b)
    for k in ARRAYS:
        assert a[k].shape == b[k].shape, f'{what}: {k} has shapes {a[k].shape} and {b[k].shape}'
        bad = np.argwhere(a[k] != b[k])
        assert bad.shape[0] == 0, (f'{what}: {k} differs in {bad.shape[0]} words; first at (record, row, word) {bad[0].tolist()}: '
                                   f'0x{int(a[k][tuple(bad[0])]):08x} != 0x{int(b[k][tuple(bad[0])]):08x}')


def _download_and_check(c, v, m, n, what, sah):
    '''records() and to_numpy() of the tree as it stands, every property against the model (v, m) -> (records, tree, Binary)'''
    rec, tree = _tree().records(), _tree().to_numpy()
    assert [rec[k].shape for k in ARRAYS] == [(max(n - 1, 0), 2, 4), (max(n - 1, 0), 4, 4), (n, 4, 4), (n, 4, 4), (n + 1, 3, 4)], what
    assert all(rec[k].dtype == np.uint32 for k in ARRAYS)
    assert c.get_option('tree_depth') == tree['depth']
    try:
        b = rc.check_all(v, m, rec, tree, n, sah, fast_depth=c.get_option('fast_depth'))
    except AssertionError as e:
        raise AssertionError(f'{what}: {e}') from None
    return rec, tree, b


def _built(c, v, m, n, builder, what):
    tree, sah, wide = builder
    _load(v, m)
    _set_builder(c, tree, sah, wide)
    _tree().build()
    if sah == 1 or (sah is None and tree is None):
        assert c.get_option('sah_fallback') == 0, f'{what}: the device SAH pass fell back to the host pass'
    return _download_and_check(c, v, m, n, what, tree != 0)


# ---------------------------------------------------------------- 1: built records
@pytest.mark.parametrize('n', SIZES)
def test_built_records_over_every_builder(fresh, n):
    '''2 to 5 triangles: roots whose children are leaves; 1025, 2049: the binned levels of the device SAH pass wrote the binary
    records.  The records of a build do not depend on the collapse, and up to 1024 triangles not on who made the SAH pass'''
    v, m = _random_model(n)
    c = _things()
    seen = {}
    for builder in BUILDERS:
        what = f'n {n} tree {builder[0]} sah_build {builder[1]} wide_build {builder[2]}'
        seen[builder], _, _ = _built(c, v, m, n, builder, what)
    _same(seen[(1, 1, 1)], seen[(1, 1, 0)], f'n {n}: device SAH pass, the two collapses')
    _same(seen[(1, 0, 1)], seen[(1, 0, 0)], f'n {n}: host SAH pass, the two collapses')
    _same(seen[(0, None, 1)], seen[(0, None, 0)], f'n {n}: LBVH, the two collapses')
    if n <= 1024:
        _same(seen[(1, 1, 1)], seen[(1, 0, 1)], f'n {n}: the device SAH pass against the host pass')
    for k in ('snode', 'tgeo', 'tshade', 'tfast'):           # (what the SAH pass does not touch)
        assert np.array_equal(seen[(1, 1, 1)][k], seen[(0, None, 1)][k]), f'n {n}: {k} depends on the option tree'


# ---------------------------------------------------------------- 2: no nodes
@pytest.mark.parametrize('n', [0, 1])
def test_no_nodes(fresh, n):
    from ptina_amd import scenes
    c = _things()
    v, m, _, _ = scenes.scene_random_tris(2, seed=2, edge=0.05)
    for at in (0, 1):                                        # built, then refitted to the other triangle
        _load(v[3 * at:3 * at + 3 * n], m[at:at + n])
        if at == 0:
            _tree().build()
        else:
            assert _tree().refit() == 1.0
        count = C.c_int(-1)
        c.call('mpt_get_records', None, None, None, None, None, 0, C.byref(count))
        assert count.value == n
        rec, _, b = _download_and_check(c, v[3 * at:3 * at + 3 * n], m[at:at + n], n, f'n {n}', True)
        assert b.ni == 0 and rec['fnode'].size == 0 and rec['snode'].size == 0
        assert (rec['tfast'][n] == 0xffffffff).all() and c.get_option('fast_depth') == 0
    assert _tree().refit_stats().cost_now == 0.0


# ---------------------------------------------------------------- 3: refitted records
def _refit_and_check(c, built, v, m, n, what, sah):
    '''built: (records, tree, Binary) of the build; loads the target (v, m), refits -> the same three for the refitted tree'''
    _load(v, m)
    _tree().refit()
    rec, tree, b = _download_and_check(c, v, m, n, what, sah)
    assert np.array_equal(b.ids, built[2].ids), f'{what}: an id row of fnode changed'
    assert np.array_equal(rec['snode'][:, :, 3], built[0]['snode'][:, :, 3]), f'{what}: a child of snode changed'
    assert np.array_equal(tree['leaf'], built[1]['leaf']), f'{what}: the leaf order changed'
    info = _tree().refit_stats()
    assert info.host_fetches == 0 and info.refits >= 1
    return rec, tree, b, info


@pytest.mark.parametrize('kind', ['jitter', 'shuffled'])
@pytest.mark.parametrize('n', SIZES)
def test_refitted_records(fresh, n, kind):
    v, m = _random_model(n)
    sv, sm = _moved_model(v, m, kind, n)
    c = _things()
    for builder in (BUILDERS if n <= 300 else [(None, None, None)]):
        what = f'n {n} {kind} tree {builder[0]} sah_build {builder[1]} wide_build {builder[2]}'
        sah = builder[0] != 0
        built = _built(c, sv, sm, n, builder, what + ', built')
        rec, _, _, info = _refit_and_check(c, built, v, m, n, what + ', refitted', sah)
        try:
            rc.check_b6(built[0]['fnode'], n, info.cost_built, 'cost_built')
            rc.check_b6(rec['fnode'], n, info.cost_now, 'cost_now')
        except AssertionError as e:
            raise AssertionError(f'{what}: {e}') from None
        if kind == 'jitter':                                 # back to the start model: the words of the build over it
            back, _, _, info = _refit_and_check(c, built, sv, sm, n, what + ', refitted back', sah)
            _same(back, built[0], what + ': there and back')
            assert np.array_equal(back['fnode'], built[0]['fnode'])      # (the unspecified words too: a refit never writes them)
            rc.check_b6(built[0]['fnode'], n, info.cost_built, 'cost_built')
            assert info.cost_now == info.cost_built and info.growth == 1.0 and info.refits == 2


@pytest.mark.parametrize('kind', ['identical', 'on_a_line', 'huge', 'two_clusters'])
def test_refitted_records_of_degenerate_targets(fresh, kind):
    '''the targets of test_refit_gpu.test_records_of_degenerate_targets, from the unit-size random model they are made of'''
    n = 3000
    from ptina_amd import scenes
    sv, m, _, _ = scenes.scene_random_tris(n, seed=7, edge=0.05)
    v = np.array(sv, F, copy=True).reshape(n, 3, 8)
    if kind == 'identical':
        v[:] = v[0]
    elif kind == 'on_a_line':
        v[:, :, 1:3] = v[0, :, 1:3]
        v[:, :, 0] = v[0, :, 0] + np.arange(n, dtype=F)[:, None] * 1e-3
    elif kind == 'huge':
        v[:, :, :3] *= F(1e18)
    else:
        v[:] = v[0]
        v[n // 3:, :, :3] += F(5.0)
    v = v.reshape(n * 3, 8)
    c = _things()
    for wide in (1, 0):
        what = f'{kind} sah_build 1 wide_build {wide}'
        built = _built(c, sv, m, n, (1, 1, wide), what + ', built')
        rec, _, _, info = _refit_and_check(c, built, v, m, n, what + ', refitted', True)
        rc.check_b6(built[0]['fnode'], n, info.cost_built, 'cost_built')
        rc.check_b6(rec['fnode'], n, info.cost_now, 'cost_now')
        if kind == 'huge':
            assert np.isnan(rec['tgeo'][:, 0, 3].view(F)).all(), 'D = inf - inf was the point of the model'


# ---------------------------------------------------------------- 4: the host build against the device build
@pytest.mark.parametrize('n,builder', [(2, (0, None, 1)), (3, (0, None, 1)), (33, (0, None, 1)), (300, (0, None, 1)), (1025, (0, None, 1)),
                                       (300, (1, 0, 1))])
def test_host_build_gives_the_device_builds_words(fresh, n, builder):
    v, m = _random_model(n)
    c = _things()
    seen = []
    for gpu_build in (1, 0):
        c.set_option('gpu_build', gpu_build)
        what = f'n {n} gpu_build {gpu_build} tree {builder[0]} sah_build {builder[1]}'
        rec, tree, _ = _built(c, v, m, n, builder, what)
        seen.append((rec, tree))
    _same(seen[0][0], seen[1][0], f'n {n} tree {builder[0]}: gpu_build 1 against 0')
    assert np.array_equal(seen[0][1]['leaf'], seen[1][1]['leaf'])


# ---------------------------------------------------------------- 5: through the composition
def _placed(center, yaw_deg):
    th = np.radians(yaw_deg)
    return np.array([[np.cos(th), 0, np.sin(th), center[0]], [0, 1, 0, center[1]], [-np.sin(th), 0, np.cos(th), center[2]], [0, 0, 0, 1.0]])


def test_records_through_the_composition(fresh):
    from ptina_amd import scenes
    from ptina_amd.things import ModelPool
    c = _things()
    pool = ModelPool()
    parts = []
    for seed in (1, 2):
        v = np.asarray(scenes.scene_random_tris(80, seed=seed, edge=0.25)[0], np.float64).reshape(80, 3, 8)
        parts.append((v[:, :, 0:3] - [0.0, 2.0, 0.0], v[:, :, 3:6], v[:, :, 6:8]))
    objs = pool.load_meshes([(*parts[0], _placed((0.0, 2.0, 0.0), 0.0), 0), (*parts[1], _placed((0.2, 2.1, 0.0), 30.0), 1),
                             (*parts[0], _placed((-0.3, 1.9, 0.3), 120.0), 2), (*parts[1], _placed((0.0, 2.0, -0.4), 200.0), 0)])
    _tree().build()
    pool.set_world(objs[2], _placed((0.6, 2.3, 0.8), 75.0))
    pool.compose()
    with pytest.raises(RuntimeError, match='BVH not built'):
        _tree().records()
    count = C.c_int(-1)
    with pytest.raises(RuntimeError, match='BVH not built'):
        c.call('mpt_get_records', None, None, None, None, None, 0, C.byref(count))
    _tree().refit()
    assert _tree().refit_stats().host_fetches == 0
    rec, tree = _tree().records(), _tree().to_numpy()
    info = _tree().refit_stats()
    assert info.host_fetches == 0 and info.refits == 1
    v, m = pool.to_numpy()                                   # (fetches the model: after the counts above)
    assert m.shape[0] == 320 and set(np.unique(m).tolist()) == {0, 1, 2}
    b = rc.check_all(v, m, rec, tree, 320, True, fast_depth=c.get_option('fast_depth'))
    rc.check_b6(rec['fnode'], 320, info.cost_now, 'cost_now')
    assert info.cost_now != info.cost_built                  # (an object moved)
    _tree().build()                                          # the composed model, built: every property again, another topology or not
    _download_and_check(c, v, m, 320, 'composed and built', True)
    assert b.ni == 319


# ---------------------------------------------------------------- 6: the door is inert
@pytest.mark.parametrize('mode', ['strict', 'fast'])
def test_the_door_changes_nothing_a_render_reads_or_writes(fresh, mode):
    from helpers import setup_engine
    from ptina_amd import scenes
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import FilmTable
    from ptina_amd.sampling.sobol import SobolSampler
    scene = scenes.scene_s34()

    def run(door, read_between):
        reset_all()
        eng = setup_engine(scene, 24, 24, mode=mode)
        ctx().set_option('count', 1)
        eng.render(4)
        if read_between:
            FilmTable().get_raw()                            # (the first launch has run: the door meets a settled context)
        rec = _tree().records() if door else None            # (else: it meets the four frames still deferred)
        eng.render(4)
        raw = FilmTable().get_raw().copy()
        return raw, SobolSampler().state(), ctx().counters(), ctx().get_option('last_kernel'), rec

    for read_between in (True, False):
        raw0, sobol0, cnt0, k0, _ = run(False, read_between)
        raw1, sobol1, cnt1, k1, rec = run(True, read_between)
        what = f'{mode}, records() {"after a read-back" if read_between else "on deferred frames"}'
        diff = np.flatnonzero((raw0.view(U) != raw1.view(U)).reshape(-1, 4).any(axis=1))
        assert diff.size == 0, f'{what}: {diff.size} film elements differ; first {int(diff[0])}: {raw0.reshape(-1, 4)[diff[0]]} against {raw1.reshape(-1, 4)[diff[0]]}'
        assert raw1.reshape(-1, 4)[:, 3].min() == 8
        assert sobol0[0] == sobol1[0] and np.array_equal(sobol0[1], sobol1[1]) and np.array_equal(sobol0[2].view(U), sobol1[2].view(U)), what
        assert cnt0 == cnt1 and cnt0['samples'] > 0, (what, cnt0, cnt1)
        assert k0 == k1, what
        rc.check_all(scene[0], scene[1], rec, _tree().to_numpy(), 34, True, fast_depth=ctx().get_option('fast_depth'))


# ---------------------------------------------------------------- 7: refusals
def test_the_doors_refusals(fresh):
    from ptina_amd._lib import fptr
    n = 33
    v, m = _random_model(n)
    c = _things()
    _load(v, m)
    count = C.c_int(-1)
    with pytest.raises(RuntimeError, match='BVH not built'):
        c.call('mpt_get_records', None, None, None, None, None, 0, C.byref(count))
    _tree().build()
    c.call('mpt_get_records', None, None, None, None, None, 0, C.byref(count))         # all NULL: the count alone, whatever the room
    assert count.value == n
    rows = dict(snode=(n - 1) * 2, fnode=(n - 1) * 4, tgeo=n * 4, tshade=n * 4, tfast=(n + 1) * 3)
    out = {k: np.full((rows[k], 4), 0x5a5a5a5a, U).view(F) for k in ARRAYS}
    for k in ARRAYS:                                         # each array alone, then all of them: too little room
        count.value = -1
        args = [fptr(out[q]) if q == k else None for q in ARRAYS]
        with pytest.raises(RuntimeError, match=rf'room for {n - 1} faces, the records hold {n}'):
            c.call('mpt_get_records', *args, n - 1, C.byref(count))
        assert count.value == n
    with pytest.raises(RuntimeError, match=r'room for 0 faces'):
        c.call('mpt_get_records', *(fptr(out[q]) for q in ARRAYS), 0, C.byref(count))
    assert all((out[k].view(U) == 0x5a5a5a5a).all() for k in ARRAYS), 'a refused call wrote into its outputs'
    want = _tree().records()
    c.call('mpt_get_records', None, fptr(out['fnode']), None, None, fptr(out['tfast']), n + 7, None)      # some arrays, ample room, no count
    assert np.array_equal(out['fnode'].view(U).reshape(-1, 4, 4), want['fnode']) and np.array_equal(out['tfast'].view(U).reshape(-1, 3, 4), want['tfast'])
    assert all((out[k].view(U) == 0x5a5a5a5a).all() for k in ('snode', 'tgeo', 'tshade'))
    _load(v, m)                                              # the model loaded again: the tree is stale until built or refitted
    with pytest.raises(RuntimeError, match='BVH not built'):
        _tree().records()


# ---------------------------------------------------------------- 8: the exact sweep, stated independently
def _sweep_ids(llo, lhi):
    '''SahBuild::split / build_range (tree_build.cpp) for ranges within sah_exact_max, over per-slot boxes [n][3] -> ids [n-1][2].
    Centres 0.5f * (lo + hi); per axis whose centres differ, the range sorted by (centre, slot) and every split k costed in f32 as
    area(left) * k + area(right) * (cnt - k); strict <, so the lowest axis and then the lowest k win; no axis left: halved as it lies'''
    n = llo.shape[0]
    ctr = (F(0.5) * (llo + lhi)).astype(F)
    ids = np.zeros((n - 1, 2), np.int64)
    todo = [(np.arange(n), 0)]
    while todo:
        idx, me = todo.pop()
        cnt = idx.size
        best, order, m = F(np.inf), idx, cnt // 2
        cl, ch = ctr[idx].min(axis=0), ctr[idx].max(axis=0)
        for a in range(3):
            if not ch[a] > cl[a]:
                continue
            by = idx[np.lexsort((idx, ctr[idx, a]))]
            lo, hi = llo[by], lhi[by]
            k = np.arange(1, cnt)
            left = rc.area(np.minimum.accumulate(lo, axis=0)[k - 1], np.maximum.accumulate(hi, axis=0)[k - 1])
            right = rc.area(np.minimum.accumulate(lo[::-1], axis=0)[::-1][k], np.maximum.accumulate(hi[::-1], axis=0)[::-1][k])
            x = left * k.astype(F)
            y = right * (cnt - k).astype(F)
            cost = x + y
            assert cost.dtype == np.float32 and not np.isnan(cost).any()
            if cost.min() < best:
                best, order, m = cost.min(), by, int(k[np.argmin(cost)])
        for side, (part, number) in enumerate(((order[:m], me + 1), (order[m:], me + m))):
            if part.size == 1:
                ids[me, side] = ~part[0]
            else:
                ids[me, side] = number
                todo.append((part, number))
    return ids


SWEEP = [2, 3, 7, 33, 129, 'equal_centres']


@pytest.mark.parametrize('case', SWEEP)
def test_the_exact_sweep_rule_gives_both_passes_id_rows(fresh, case):
    '''nodes compared: n - 1 for each of the two passes -- 1, 2, 6, 32 and 128, and 32 for the model whose centres are all equal
    (33 triangles of different sizes about one point: no axis can be chosen, every range is halved as it lies)'''
    if case == 'equal_centres':
        n = 33
        v, m = _random_model(n)
        v = np.array(v, F, copy=True).reshape(n, 3, 8)
        tri = np.array([[-1, -1, -1], [1, 1, 1], [1, -1, 0]], F)
        v[:, :, 0:3] = F(0.5) + tri[None] * (np.arange(1, n + 1, dtype=F) / F(128))[:, None, None]       # boxes 0.5 +- k / 128, exact: centres 0.5
        v = v.reshape(3 * n, 8)
    else:
        n = case
        v, m = _random_model(n)
    c = _things()
    assert n <= c.get_option('sah_exact_max')
    for sah in (0, 1):
        what = f'{case}: sah_build {sah}'
        rec, tree, b = _built(c, v, m, n, (1, sah, 1), what)
        llo, lhi = rc.leaf_boxes(rc.positions(v), tree['leaf'])
        if case == 'equal_centres':
            ctr = F(0.5) * (llo + lhi)
            assert (ctr == F(0.5)).all()
        want = _sweep_ids(llo, lhi)
        bad = np.argwhere(b.ids != want)
        assert bad.shape[0] == 0, (f'{what}: {bad.shape[0]} of {2 * (n - 1)} ids differ from the rule; first at node {bad[0][0]} child {bad[0][1]}: '
                                   f'{int(b.ids[tuple(bad[0])])} != {int(want[tuple(bad[0])])}')
        print(f'{what}: {n - 1} nodes compared')

'''
The traversal of the production PathEngine kernels held to an exhaustive float64 search on arbitrary rays, ray for ray (-m gpu).
BVHTree.walk_trace (mpt_walk_trace, csrc/walk_eval.hip) sends a batch of rays through the in-wave state
machine of csrc/render_lane.h -- lane_start_ray, stage_node / stage_node4, stage_leaf, classify, the render kernels' own code --
over each of its five walk types, set up as the render kernel of that walk sets it up.  tests/query_ref.py says which rays it can
decide without a tree; on those hit and index are exact for every walk: no share of outliers, no other kernel as the witness.

The sets (tests/test_walks_cpu.py: their caps, and the oracle's own walk on every one of them) and what only they reach:
  A  origins in and around the box, all eight direction octants: the entry-plane choice for rays going up an axis (LdsWalk::PLANE_OFF
     with offx / offy / offz, ox ^ 8; ox ^ 16 of node4; the dnx / dny / dnz selects of the 8-bit step) -- a plane picked by the wrong sign
     makes tn > tf for a box the ray enters, and the hit behind it is lost; T_SCALED with origins inside the model (the fmed3 clamp,
     tbest scaled then unscaled: a wrong clamp passes or fails the box at distance 1 / ts; a missing unscale shows in depth)
  B  bounce rays that start ON a face and avoid it: navoid in its three encodings (~slot, (slot << 4) | 1, 0), filtered in stage_node
     for the binary walks and in stage_leaf for the 4-wide ones, the leaf a ray starts in included -- without the filter the ray hits its
     own face at t ~ 0 (most of set B is then wrong: test_walks_cpu shows it); with the wrong encoding it filters nothing, or another face
  C  rays with one or two direction components exactly +-0: 1 / d = +-inf and o / d = inf or NaN in exit_min and the slab FMAs -- a NaN
     that wins a min / max drops or admits a box; the -0.0 half picks the "down" planes by the sign bit of -inf
  shadow rays (dis given): the `stop` exit of stage_leaf, dd <= tbest against dd < tbest with the bound moved up one float for the
     LDS-resident walks, the stack left non-empty for the next ray (the batches that follow run on the same LDS columns) -- a shadow ray
     that keeps walking answers the same, one that stops on a hit beyond dis, or misses one within it, does not
  the 16-bit key / id sort (IDS16) meets other orders and ties than a camera ray's in all of the above: a mis-sorted pair only costs
     steps unless an id is lost, which loses a hit
No deliberately wrong kernel is built or run: what a test would catch is argued above from the code.

depth, u and v are what SHADE would be handed, the walk's own f32 numbers.  On decided hits they are bit-identical across the five
walks (the same tri_test_fast on the same record and ray; t_scale is a power of two).  Against f64: depth within query_ref.DEPTH_GAP
(a larger error could have changed the winner); u and v within UV_RATIO x the deviation of the oracle's own f32 intersect on the
same rays (twice the largest ratio DESIGN 3.15 records, 5.6; the ratios are printed and DESIGN 3.16 records them).
'''

import os
import subprocess
import sys

import numpy as np
import pytest

import query_ref as qr
import visibility_ref as vr
from test_visibility_ref_cpu import case
from test_visibility_gpu import TREES, _setup, _deep
from test_query_gpu import _objects, _placed, bits, check
from test_walks_cpu import sets, far, assert_caps, oracle_deviation

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALKS = ('gather', 'lds', 'wide_exact', 'wide_quant', 'lds4')
GATHER = ('gather', 'wide_exact', 'wide_quant')
INF = np.float32(1e6)
UV_RATIO = 2 * 5.6


def tree():
    from ptina_amd.things import BVHTree
    return BVHTree()


def exact(ref, got, what):
    '''hit and index exactly the yardstick's on every decided ray; a miss reads -1 / 1e6 / 0 / 0; depth within DEPTH_GAP'''
    check(ref, got, what)
    ok = ref['decided'] & ref['hit']
    rel = np.abs(got['depth'].astype(np.float64) - np.where(ok, ref['t'], 0.0)) / np.where(ok, ref['t'], 1.0)
    bad = np.flatnonzero(ok & ~(rel <= qr.DEPTH_GAP))
    assert bad.size == 0, f'{what}: {bad.size} depths off by more than {qr.DEPTH_GAP} relative; first ray {int(bad[0])}: {got["depth"][bad[0]]!r} against {ref["t"][bad[0]]!r}'
    return int(ref['decided'].sum())


def same_on_hits(ref, a, b, what):
    '''depth, u, v of two walks bit for bit on the decided hits (and hit, index on every decided ray)'''
    ok = ref['decided'] & ref['hit']
    for key in ('depth', 'u', 'v'):
        diff = np.flatnonzero(ok & (bits(a[key]) != bits(b[key])))
        assert diff.size == 0, f'{what}: {key} differs in {diff.size} decided hits; first ray {int(diff[0])}: {a[key][diff[0]]!r} against {b[key][diff[0]]!r}'


def through_walks(name, walks, which_sets, what, oracle_mod=None):
    '''every set of a case through every walk, on the tree as it stands -> decided rays checked per walk'''
    s = assert_caps(name)
    checked = 0
    for which in which_sets:
        if which not in s:
            continue
        o, d, avoid, ref = s[which]
        first = None
        for walk in walks:
            got = tree().walk_trace(walk, o, d, avoid=avoid)
            assert got['hit'].dtype == bool and got['depth'].dtype == np.float32 and got['index'].dtype == np.int32 and got['hit'].shape == (o.shape[0],)
            n = exact(ref, got, f'{what} set {which} walk {walk}')
            if first is None:
                first = got
                checked += n
                if oracle_mod is not None:
                    _, dev_uv = qr.deviation(ref, got)
                    _, orc_uv = oracle_deviation(oracle_mod, name, which)
                    print(f'{what} set {which}: u, v within {dev_uv:.3g} of the f64 values, the oracle within {orc_uv:.3g}: ratio {dev_uv / orc_uv:.2f} of {UV_RATIO} allowed')
                    assert dev_uv <= UV_RATIO * orc_uv, f'{what} set {which}: u, v off by {dev_uv:.3g}, {dev_uv / orc_uv:.1f} x the oracle\'s {orc_uv:.3g}'
            else:
                same_on_hits(ref, first, got, f'{what} set {which}: walk {walks[0]} against {walk}')
    print(f'{what}: {checked} decided rays through each of {len(walks)} walks')
    return checked


# ---------------------------------------------------------------- 1. closest hit, every walk x sets A, B, C
@pytest.mark.parametrize('name', ['n2', 'n3', 'n33', 'n300', 'n1025', 'moved', 'x1024', 'flat'])
def test_closest_hit_through_all_five_walks(fresh, oracle_mod, name):
    '''n2 / n3: 4-wide nodes with unused slots; n1025: the first binned SAH level; moved: 8-bit planes far from the origin;
    x1024: T_SCALED; flat: a lo == hi slab'''
    _setup(case(name), 'fast')
    assert through_walks(name, WALKS, 'ABC', name, oracle_mod) > 1000


def test_a_scene_beyond_lds_through_the_gather_walks_and_refused_by_the_lds_walks(fresh, oracle_mod):
    _setup(case('n5000'), 'fast')
    through_walks('n5000', GATHER, 'ABC', 'n5000', oracle_mod)
    o, d, _, _ = sets('n5000')['A']
    for walk in ('lds', 'lds4'):
        with pytest.raises(RuntimeError, match='do not fit'):
            tree().walk_trace(walk, o, d)
        with pytest.raises(RuntimeError, match='do not fit'):
            tree().walk_trace(walk, o[:0], d[:0])


def test_the_64_level_binary_walk_and_both_4_wide_gather_walks_on_a_deep_tree(fresh, oracle_mod):
    _deep('fast')                                            # (asserts fast_depth + 2 > 32)
    through_walks('deep', GATHER, 'ABC', 'deep', oracle_mod)


def test_a_strict_context_is_refused(fresh):
    _setup(case('n300'), 'strict')
    o, d, _, _ = sets('n300')['A']
    for walk in WALKS:
        with pytest.raises(RuntimeError, match='strict mode'):
            tree().walk_trace(walk, o, d)
    with pytest.raises(RuntimeError, match='walk 5'):
        tree().walk_trace(5, o, d)


# ---------------------------------------------------------------- 2. every tree builder
@pytest.mark.parametrize('builder', list(TREES))
@pytest.mark.parametrize('name', ['n300', 'n1025'])
def test_every_tree_builder(fresh, name, builder):
    _setup(case(name), 'fast', TREES[builder])
    through_walks(name, WALKS, 'AB', f'{name} {builder}')


# ---------------------------------------------------------------- 3. shadow rays
@pytest.mark.parametrize('name', ['n300', 'n1025', 'n5000'])
def test_shadow_rays(fresh, name):
    _setup(case(name), 'fast')
    s = assert_caps(name)
    for which in 'AB':
        o, d, avoid, ref = s[which]
        hits, misses = ref['decided'] & ref['hit'], ref['decided'] & ~ref['hit']
        tn = np.where(hits, ref['t'], 1.0)
        for walk in (WALKS if name != 'n5000' else GATHER):
            what = f'shadow {name} set {which} walk {walk}'
            short = tree().walk_trace(walk, o, d, avoid=avoid, dis=(0.5 * tn).astype(np.float32))
            long_ = tree().walk_trace(walk, o, d, avoid=avoid, dis=(2.0 * tn).astype(np.float32))
            any_ = tree().walk_trace(walk, o, d, avoid=avoid, dis=INF)
            assert short.dtype == bool and short.shape == (o.shape[0],)
            for got, want, how in ((short, False, 'dis = tn / 2'), (long_, True, 'dis = 2 tn'), (any_, True, 'dis = 1e6')):
                bad = np.flatnonzero(hits & (got != want))
                assert bad.size == 0, f'{what}, {how}: {bad.size} decided hits are not {want}; first ray {int(bad[0])}, t {ref["t"][bad[0]]}'
            bad = np.flatnonzero(misses & (any_ | long_ | short))
            assert bad.size == 0, f'{what}: {bad.size} decided misses are occluded; first ray {int(bad[0])}'
            # a closest-hit batch behind the shadow batches, on the stacks they left: the answers of a fresh context's (test 1)
            exact(ref, tree().walk_trace(walk, o, d, avoid=avoid), what + ', the closest hits after it')


# ---------------------------------------------------------------- 4. a far origin
@pytest.mark.parametrize('name', ['n300', 'x1024'])
def test_rays_from_far_outside(fresh, name):
    '''t_scale follows the batch's origins (fill_t_scale): from 64 radii the scaled distances still end below 1'''
    _setup(case(name), 'fast')
    for radii in (4, 64):
        o, d, ref = far(name, radii)
        dec, hits, misses = float(ref['decided'].mean()), float((ref['decided'] & ref['hit']).mean()), float((ref['decided'] & ~ref['hit']).mean())
        print(f'{name} from {radii} radii: decided {dec:.3f}, hits {hits:.3f}, misses {misses:.3f}')
        assert dec >= 0.90 and hits >= 0.20 and misses >= 0.20
        a = tree().walk_trace('lds4', o, d)
        b = tree().walk_trace('wide_quant', o, d)
        exact(ref, a, f'{name} from {radii} radii, lds4')
        exact(ref, b, f'{name} from {radii} radii, wide_quant')
        same_on_hits(ref, a, b, f'{name} from {radii} radii')
    # ... and the batch of test 1 behind it is not affected by the scale the far batch asked for
    o, d, _, ref = sets(name)['A']
    exact(ref, tree().walk_trace('lds4', o, d), f'{name} set A after the far batches')


# ---------------------------------------------------------------- 5. after refit()
def test_after_a_refit_the_walks_see_the_moved_object(fresh):
    _setup(case('n300'), 'fast')
    pool, objs, _ = _objects()
    tree().build()
    pos = vr.positions(pool.to_numpy()[0])
    pool.set_world(objs[2], _placed((0.6, 2.3, 0.8), 75.0))
    pool.compose()
    o, d = qr.rays(pos, 320)
    for walk in WALKS:
        with pytest.raises(RuntimeError, match='BVH not built'):
            tree().walk_trace(walk, o, d)
    tree().refit()
    now = vr.positions(pool.to_numpy()[0])
    assert not np.array_equal(now[160:240], pos[160:240])
    o, d = qr.rays(now, 321)
    ref = qr.classify(now, o, d)
    qr.caps('refitted', ref)
    ob, db, av = qr.bounce_rays(now, o, d, ref, 322)
    refb = qr.classify(now, ob, db, avoid=av)
    qr.caps_of_set('refitted', 'B', refb)
    old = qr.classify(pos, o, d)
    for walk in WALKS:
        got = tree().walk_trace(walk, o, d)
        exact(ref, got, f'refitted, set A, walk {walk}')
        exact(refb, tree().walk_trace(walk, ob, db, avoid=av), f'refitted, set B, walk {walk}')
        assert qr.errors(old, got, 'the model before the move'), f'walk {walk}: the rays do not tell the moved model from the one before'


# ---------------------------------------------------------------- 6. the spill path
_SPILL_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from ptina_amd.common import reset_all
from ptina_amd.things import BVHTree
from test_visibility_ref_cpu import case
from test_visibility_gpu import _setup, _deep
from test_walks_cpu import sets
out = {}
for name in ('n1025', 'deep'):
    reset_all()
    if name == 'deep':
        _deep('fast')
    else:
        _setup(case(name), 'fast')
    for which in 'AB':
        o, d, avoid, _ = sets(name)[which]
        for walk in ('wide_exact', 'wide_quant'):
            got = BVHTree().walk_trace(walk, o, d, avoid=avoid)
            for key, a in got.items():
                out[f'{name}.{which}.{walk}.{key}'] = a
reset_all()
np.savez(sys.argv[2], **out)
for path in sorted({line.split()[-1] for line in open('/proc/self/maps') if 'libmiptina' in line}):
    print('LOADED', path)
print('DONE')
'''


def test_spilled_stacks_against_truth_and_the_normal_library(fresh, tmp_path):
    '''libmiptina_spilltest.so keeps 4 stack levels per lane in LDS: push / pop beyond CAP and the divergent branch of stage_node4
    near CAP run for every ray, on the door's own strip.  Same tree, same order: the truth, and the normal library's bits'''
    lib = os.path.join(ROOT, 'ptina_amd', 'libmiptina_spilltest.so')
    assert os.path.exists(lib), 'build it with make -C ptina_amd/csrc spilltest (__graft_entry__.build() does)'
    script, out = tmp_path / 'spill.py', tmp_path / 'spill.npz'
    script.write_text(_SPILL_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], env=dict(os.environ, MIPTINA_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'DONE' in r.stdout, r.stdout + r.stderr
    loaded = [line.split(' ', 1)[1] for line in r.stdout.splitlines() if line.startswith('LOADED ')]
    assert [os.path.realpath(x) for x in loaded] == [os.path.realpath(lib)], f'the child process mapped {loaded}, not only {lib}'
    spilled = np.load(out)
    for name in ('n1025', 'deep'):
        from ptina_amd.common import reset_all
        reset_all()
        if name == 'deep':
            _deep('fast')
        else:
            _setup(case(name), 'fast')
        for which in 'AB':
            o, d, avoid, ref = sets(name)[which]
            for walk in ('wide_exact', 'wide_quant'):
                got = {key: spilled[f'{name}.{which}.{walk}.{key}'] for key in ('hit', 'depth', 'index', 'u', 'v')}
                exact(ref, got, f'spilltest library, {name} set {which} walk {walk}')
                normal = tree().walk_trace(walk, o, d, avoid=avoid)
                exact(ref, normal, f'normal library, {name} set {which} walk {walk}')
                for key in got:
                    diff = np.flatnonzero(bits(got[key]) != bits(normal[key]))
                    assert diff.size == 0, f'{name} set {which} walk {walk}: {key} of the spilltest library differs in {diff.size} rays; first {int(diff[0])}'


# ---------------------------------------------------------------- 7. launch edges
def _raw(walk, n, o, d, only=None, chunk=0, dis=None):
    '''mpt_walk_trace itself; only: the one output that is asked for (the others NULL)'''
    from ptina_amd.common import ctx
    from ptina_amd._lib import fptr, iptr
    kinds = dict(hit=np.int32, depth=np.float32, index=np.int32, u=np.float32, v=np.float32)
    out = {k: np.full(n, 77, t) for k, t in kinds.items() if only in (None, k)}
    ptr = lambda k: None if k not in out else (iptr(out[k]) if kinds[k] == np.int32 else fptr(out[k]))   # noqa: E731
    ctx().call('mpt_walk_trace', WALKS.index(walk), n, fptr(o), fptr(d), None, None if dis is None else fptr(dis), ptr('hit'), ptr('depth'), ptr('index'), ptr('u'), ptr('v'), chunk)
    return out


def same(a, b, what):
    for key in ('hit', 'depth', 'index', 'u', 'v'):
        diff = np.flatnonzero(bits(a[key]) != bits(b[key]))
        assert diff.size == 0, f'{what}: {key} differs in {diff.size} rays; first {int(diff[0])}: {a[key][diff[0]]!r} against {b[key][diff[0]]!r}'


@pytest.mark.parametrize('walk', WALKS)
def test_launch_edges(fresh, walk):
    _setup(case('n300'), 'fast')
    o, d, _, ref = sets('n300')['A']
    full = tree().walk_trace(walk, o, d)
    exact(ref, full, f'edges {walk}')
    for n in (1, 255, 256, 257, 1023, 1025):
        part = tree().walk_trace(walk, o[:n], d[:n])
        assert part['hit'].shape == (n,)
        same(part, {k: a[:n] for k, a in full.items()}, f'{walk}: the first {n} rays alone')
    empty = tree().walk_trace(walk, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert all(a.shape == (0,) for a in empty.values()) and empty['hit'].dtype == bool
    assert tree().walk_trace(walk, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), dis=1.0).shape == (0,)
    occ = tree().walk_trace(walk, o, d, dis=INF)
    for chunk in (1024, 100):
        same(tree().walk_trace(walk, o, d, chunk=chunk), full, f'{walk}: chunks of {chunk}')
        assert np.array_equal(tree().walk_trace(walk, o, d, dis=INF, chunk=chunk), occ)
    raw = _raw(walk, qr.RAYS, o, d)
    for key in raw:
        one = _raw(walk, qr.RAYS, o, d, only=key, chunk=1024)
        assert list(one) == [key] and np.array_equal(bits(one[key]), bits(raw[key])), f'{walk}: {key} asked for alone'
        assert np.array_equal(raw[key] != 0, full[key]) if key == 'hit' else np.array_equal(bits(raw[key]), bits(full[key])), f'{walk}: {key} through the C call'
    # a shadow batch writes the verdicts and nothing else
    shadow = _raw(walk, qr.RAYS, o, d, dis=np.full(qr.RAYS, INF, np.float32))
    assert np.array_equal(shadow['hit'] != 0, occ) and all(np.all(shadow[k] == 77) for k in ('depth', 'index', 'u', 'v'))


@pytest.mark.parametrize('walk', WALKS)
def test_bad_rays_are_misses_and_leave_the_others_alone(fresh, walk):
    _setup(case('n300'), 'fast')
    o, d, _, ref = sets('n300')['A']
    clean = tree().walk_trace(walk, o, d)
    clean_occ = tree().walk_trace(walk, o, d, dis=INF)
    rng = np.random.default_rng(5)
    at = rng.permutation(qr.RAYS)[:96]
    ob, db = o.copy(), d.copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for k, r in enumerate(at):
        axis = k % 3
        kind = (k // 3) % 6
        if kind == 0:
            db[r] = 0.0
        elif kind == 1:
            db[r] = (-0.0, 0.0, -0.0)
        elif kind == 2:
            ob[r, axis] = nan
        elif kind == 3:
            ob[r, axis] = inf if k % 2 else -inf
        elif kind == 4:
            db[r, axis] = nan
        else:
            db[r, axis] = inf
    got = tree().walk_trace(walk, ob, db)
    occ = tree().walk_trace(walk, ob, db, dis=INF)
    assert not got['hit'][at].any() and np.all(got['index'][at] == -1) and np.all(got['depth'][at] == INF)
    assert np.all(got['u'][at] == 0) and np.all(got['v'][at] == 0) and not occ[at].any()
    keep = np.ones(qr.RAYS, bool)
    keep[at] = False
    same({k: a[keep] for k, a in got.items()}, {k: a[keep] for k, a in clean.items()}, f'{walk}: the rays beside the bad ones')
    assert np.array_equal(occ[keep], clean_occ[keep])
    assert clean['hit'][at].any()                            # (some of the replaced rays were hits)


# ---------------------------------------------------------------- 8. no side effects
def test_the_door_changes_nothing_a_render_reads_or_writes(fresh):
    from helpers import setup_engine
    from ptina_amd import scenes
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import FilmTable
    from ptina_amd.sampling.sobol import SobolSampler
    scene = scenes.scene_s34()
    pos = vr.positions(scene[0])
    o, d = qr.rays(pos, 34, 512)
    ref = qr.classify(pos, o, d)
    assert (ref['decided'] & ref['hit']).any()

    def run(door, read_between):
        reset_all()
        eng = setup_engine(scene, 24, 24, mode='fast')
        ctx().set_option('count', 1)
        eng.render(4)
        if read_between:
            FilmTable().get_raw()                            # (the first launch has run: the door meets a settled context)
        answers = {}
        if door:                                             # (else: it meets the four frames still deferred, and flushes them)
            for walk in WALKS:
                answers[walk] = tree().walk_trace(walk, o, d)
                tree().walk_trace(walk, o, d, dis=INF)
        eng.render(4)
        raw = FilmTable().get_raw().copy()
        return raw, SobolSampler().state(), ctx().counters(), ctx().get_option('last_kernel'), answers

    for read_between in (True, False):
        raw0, sobol0, cnt0, k0, _ = run(False, read_between)
        raw1, sobol1, cnt1, k1, answers = run(True, read_between)
        what = f'door {"after a read-back" if read_between else "on deferred frames"}'
        diff = np.flatnonzero((bits(raw0) != bits(raw1)).reshape(-1, 4).any(axis=1))
        assert diff.size == 0, f'{what}: {diff.size} film elements differ; first {int(diff[0])}: {raw0.reshape(-1, 4)[diff[0]]} against {raw1.reshape(-1, 4)[diff[0]]}'
        assert raw1.reshape(-1, 4)[:, 3].min() == 8
        assert sobol0[0] == sobol1[0] and np.array_equal(sobol0[1], sobol1[1]) and np.array_equal(bits(sobol0[2]), bits(sobol1[2])), what
        assert cnt0 == cnt1 and cnt0['samples'] > 0, (what, cnt0, cnt1)
        assert k0 == k1 == 5, what
        for walk in WALKS:
            exact(ref, answers[walk], f'{what}, walk {walk}')


# ---------------------------------------------------------------- 9. the same sets through the public queries, both builds
@pytest.mark.parametrize('mode', ['strict', 'fast'])
@pytest.mark.parametrize('name', ['n3', 'n300', 'n1025', 'n5000', 'moved', 'x1024', 'flat', 'deep'])
def test_bounce_and_axis_rays_through_the_public_queries(fresh, oracle_mod, name, mode):
    '''BVHTree.intersect / occluded (bvh_walk over fnode; the strict build: the reference's walk) on sets B and C, which the query
    tests never send.  depth / u / v as test_query_gpu.tolerance takes them: 4 x the oracle's own deviation on the same rays'''
    s = assert_caps(name)
    if name == 'deep':
        _deep(mode)
    else:
        _setup(case(name), mode)
    for which in 'BC':
        if which not in s:
            continue
        o, d, avoid, ref = s[which]
        dev_depth, dev_uv = oracle_deviation(oracle_mod, name, which)
        got = tree().intersect(o, d, avoid=avoid)
        print(f'{name} {mode} set {which}: deviation depth, uv {qr.deviation(ref, got)} of {(4 * dev_depth, 4 * dev_uv)} allowed')
        check(ref, got, f'intersect {mode} {name} set {which}', tol_depth=4 * dev_depth, tol_uv=4 * dev_uv)
        occ = tree().occluded(o, d, avoid=avoid)
        bad = np.flatnonzero(ref['decided'] & (occ != ref['hit']))
        assert bad.size == 0, f'occluded {mode} {name} set {which}: {bad.size} decided rays wrong; first {int(bad[0])}'

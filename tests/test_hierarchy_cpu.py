'''
CPU tests of parent bindings: the pure functions of the host runtime (mpt_hierarchy_rule, mpt_parent_check:
no context, no GPU) against the restatement the GPU tests hold the kernel to (tests/hierarchy_ref.py) -- bit for bit wherever no
LINEAR rotation track's theta branch feeds the chain, within the first-order bound pushed through every product where one does --, a
chain of depth 1 against mpt_motion_rule and a hand product, every refusal by number, tools.skin.attach, and the rule alone under the
host sanitizers (tools/hierarchy_rule_check.cpp).
'''

import os
import re

import numpy as np
import pytest

import anim_ref as ar
import anim_blend_ref as br
import hierarchy_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('mpt_object_set_parent', 'mpt_object_get_parent', 'mpt_hierarchy_stats', 'mpt_hierarchy_kernel_time', 'mpt_parent_check', 'mpt_hierarchy_rule')


@pytest.fixture(scope='module')
def cases():
    return hr.chain_cases()


def _rule(chain, t):
    from ptina_amd import _lib
    return _lib.hierarchy_rule(hr.packed(chain), t)


def test_header_ctypes_table_and_library_carry_the_new_calls():
    from ptina_amd import _lib, worker
    from ptina_amd.things import ModelPool
    from ptina_amd.tools import skin
    lib = _lib.load_library()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'miptina.h')).read(), flags=re.S)
    for s in NEW:
        assert re.search(r'\bint %s\s*\(' % s, header), s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
    assert 'mpt_hierarchy_info;' in header
    assert [f for f, _ in _lib.HierarchyInfo._fields_] == ['bound_children', 'deepest', 'evaluated', 'levels', 'launches']
    assert [f for f, _ in _lib.AnimBlendInfo._fields_] == ['object_clips', 'blended_objects', 'moved_objects', 'evaluated_blended', 'evaluated_moved']
    assert callable(worker.set_object_parent) and callable(skin.attach)
    for f in ('set_parent', 'parent_of', 'hierarchy_stats'):
        assert callable(getattr(ModelPool, f))
    assert (_lib.HIER_MAX_DEPTH, _lib.HIER_ONE_GROUP) == (hr.MAX_DEPTH, hr.ONE_GROUP)
    types = open(os.path.join(ROOT, 'ptina_amd', 'csrc', 'mpt_types.h')).read()
    assert re.search(r'#define MPT_HIER_MAX_DEPTH %d\b' % hr.MAX_DEPTH, types) and re.search(r'#define MPT_HIER_ONE_GROUP %d\b' % hr.ONE_GROUP, types)


def test_hierarchy_rule_equals_the_restatement(cases):
    n = theta_n = 0
    worst = 0.0
    for name, chain, exact in cases:
        for t in hr.TIMES:
            got = _rule(chain, t)
            theta, ratio = hr.check_chain(got, chain, t, ar.ULP_TRIG_HOST, '%s t %g' % (name, t))
            assert theta == 0 or not exact, (name, 'a case that claims to be exact takes the theta branch')
            assert np.isfinite(got).all()
            n += theta == 0
            theta_n += theta > 0
            worst = max(worst, ratio)
    print('%d chains bit for bit, %d on the theta branch with largest |rule - restatement| / bound %.4f' % (n, theta_n, worst))
    assert n >= 40 and theta_n >= 10


def test_cases_cover_the_corners_they_name(cases):
    depths = {len(c[1]) - 1 for c in cases}
    assert {0, 1, 2, 3, hr.MAX_DEPTH} <= depths
    links = [ln for c in cases for ln in c[1]]
    assert any(ln.get('pal') is not None and ln.get('motion') is not None for ln in links)
    assert any(ln.get('pal') is not None and ln.get('motion') is None for ln in links)
    assert any(ln.get('motion') is None and list(np.asarray(ln['local'])[3]) != [0, 0, 0, 1] for ln in links)         # not affine
    assert {tr.interpolation for ln in links if ln.get('motion') for tr in ln['motion'][0]} == {0, 1, 2}
    assert any(c[1][0].get('motion') for c in cases) and any(c[1][-1].get('motion') for c in cases)
    assert any(0 < k < len(c[1]) - 1 and ln.get('motion') for c in cases for k, ln in enumerate(c[1]))
    assert sum(not c[2] for c in cases) >= 6
    # the theta cases carry a bound that is not zero and stays under the cap
    for name, chain, exact in cases:
        if not exact:
            thetas = [hr.chain_world(chain, t)[1] for t in hr.TIMES]
            assert max(thetas) > 0, name
            for t, th in zip(hr.TIMES, thetas):
                if th:
                    b = hr.chain_bound(chain, t, ar.ULP_TRIG_DEVICE, ar.ULP_TRIG_HOST)
                    assert 0 < b.max() <= hr.CAP * np.abs(hr.chain_world(chain, t)[0]).max(), name


def test_a_chain_of_depth_1_is_the_motion_rule_and_one_hand_product_bit_for_bit():
    from ptina_amd import _lib
    g = np.random.default_rng(5)
    n = 0
    for name, tracks, rest, base, binds, exact in br.motion_cases():
        clip = br.pack_clip(tracks)
        for b in binds[:4]:
            for t in hr.TIMES:
                M = _lib.motion_rule(clip, b, rest, base, t)                       # (host against host: the same library on the theta branch too)
                P, L, pal = hr.general(g), hr.affine(g), hr.affine(g)[:3]
                moved = dict(motion=(tracks, b, rest, base))
                assert hr.same_bits(_rule([moved], t), M), (name, 'a root alone')
                # moved child of a static root; static child of a moved root; on a joint: by the one expression, by hand
                assert hr.same_bits(_rule([dict(local=P), moved], t), np.array(hr.mat4_mul(list(P.reshape(16)), list(M.reshape(16)))).reshape(4, 4)), name
                assert hr.same_bits(_rule([moved, dict(local=L)], t), np.array(hr.mat4_mul(list(M.reshape(16)), list(L.reshape(16)))).reshape(4, 4)), name
                X = hr.mat4_mul(list(pal.reshape(12)) + [0.0, 0.0, 0.0, 1.0], list(L.reshape(16)))
                assert hr.same_bits(_rule([moved, dict(local=L, pal=pal)], t), np.array(hr.mat4_mul(list(M.reshape(16)), X)).reshape(4, 4)), name
                n += 1
    assert n >= 40
    # the product is not numpy's matmul order by accident: it is the written sum, and agrees with matmul to rounding
    A, B = hr.general(g), hr.general(g)
    W = np.array(hr.mat4_mul(list(A.reshape(16)), list(B.reshape(16)))).reshape(4, 4)
    assert np.abs(W - A @ B).max() < 1e-15
    assert hr.same_bits(_rule([dict(local=A), dict(local=B)], 0.0), W)


def test_an_identity_palette_entry_changes_nothing_and_a_joint_acts_as_a_skinned_vertex():
    g = np.random.default_rng(6)
    P, L = hr.affine(g), hr.affine(g)
    eye = np.eye(4)[:3]
    assert hr.same_bits(_rule([dict(local=P), dict(local=L, pal=eye)], 0.0), _rule([dict(local=P), dict(local=L)], 0.0))
    # a point of the child moves as deform's skinning moves a vertex with weight 1 on the joint: world(parent) . M . (local . x)
    M = hr.affine(g)
    W = _rule([dict(local=P), dict(local=L, pal=M[:3])], 0.0)
    x = np.array([0.3, -0.7, 0.2, 1.0])
    assert np.abs(W @ x - P @ (M @ (L @ x))).max() < 1e-14


def test_attach_folds_the_bind_matrix_in():
    from ptina_amd.tools import skin
    g = np.random.default_rng(7)
    bind, local, glob = hr.affine(g), hr.affine(g), hr.affine(g)
    ib = np.linalg.inv(bind)
    A = skin.attach(ib, local)
    assert A.dtype == np.float64 and A.shape == (4, 4)
    # skinning matrix . attach = global . local: the child sits in the joint's frame
    assert np.abs((glob @ ib) @ A - glob @ local).max() < 1e-13
    assert np.array_equal(skin.attach(ib[:3], local), A)
    with pytest.raises(ValueError):
        skin.attach(np.eye(3), local)


def test_set_parent_refuses_by_number():
    from ptina_amd import _lib
    P = _lib.parent_check
    R = _lib.PARENT_REFUSALS
    parents, inst, nj = [-1, 0, 1, -1, -1, 3], [0, 0, 0, 0, 1, 0], [0, 4, 0, 0, 0, 0]
    v = lambda *a: P(parents, inst, nj, *a)[0]                                 # noqa: E731
    assert R[v(6, 0)] == R[v(-1, 0)] == R[v(0, 6)] == R[v(0, -2)] == 'unknown' and v(6, None) == 1
    assert R[v(0, 0)] == R[v(0, 1)] == R[v(0, 2)] == R[v(1, 2)] == 'cycle'
    assert R[v(4, 0)] == R[v(0, 4)] == 'instance'
    assert R[v(3, 0, 0)] == R[v(3, 2, 1)] == 'no skin'
    assert R[v(3, 1, 4)] == R[v(3, 1, 400)] == R[v(3, 1, -2)] == 'joint'
    assert v(3, 1, 0) == v(3, 1, 3) == v(3, 1) == v(3, 2) == v(2, 3) == v(2, 5) == 0
    assert v(2, None) == v(0, None) == v(4, None) == 0                         # unparenting is never a cycle
    for a in ((6, 0), (0, 2), (4, 0), (3, 0, 0), (3, 1, 4)):
        assert P(parents, inst, nj, *a)[1], a                                  # every refusal has its words
    assert parents == [-1, 0, 1, -1, -1, 3]
    # depth: a chain of 65 objects is 64 deep and holds; one more link does not, at the top, at the bottom or in the middle
    m = hr.MAX_DEPTH
    chain = [-1] + list(range(m)) + [-1, -1]                                    # objects 0 .. m in one chain; m + 1 and m + 2 free
    z = [0] * (m + 3)
    assert P(chain, z, z, m + 1, m - 1)[0] == 0 and R[P(chain, z, z, m + 1, m)[0]] == 'depth'
    assert R[P(chain, z, z, 0, m + 1)[0]] == 'depth'                            # the whole chain under another root
    two = [-1] + list(range(31)) + [-1] + list(range(32, 63))                   # two chains 31 deep
    z = [0] * 64
    assert P(two, z, z, 32, 31)[0] == 0 and P(two, z, z, 32, 30)[0] == 0        # 31 + 1 + 31 = 63
    two = [-1] + list(range(32)) + [-1] + list(range(33, 65))                   # two chains 32 deep: 32 + 1 + 32 = 65
    z = [0] * 66
    assert R[P(two, z, z, 33, 32)[0]] == 'depth' and P(two, z, z, 33, 31)[0] == 0


def test_hierarchy_rule_refuses_by_number():
    from ptina_amd import _lib
    tk = br.track
    clip = br.pack_clip([tk(0, 'T', [0, 1], np.zeros((2, 3)))])
    ok = (0.0, 1.0, True)
    eye = np.eye(4)

    def verdict(chain):
        with pytest.raises(ValueError) as e:
            _lib.hierarchy_rule(chain, 0.0)
        return int(str(e.value).rsplit(' ', 1)[1])
    assert verdict([]) == 602 and verdict([dict(local=eye)] * (hr.MAX_DEPTH + 2)) == 602
    assert np.array_equal(_lib.hierarchy_rule([dict(local=eye)] * (hr.MAX_DEPTH + 1), 0.0), eye)
    bad = eye.copy()
    bad[1, 2] = np.nan
    assert verdict([dict(local=eye), dict(local=bad)]) == 603
    pal = np.eye(4)[:3].copy()
    pal[0, 0] = np.inf
    assert verdict([dict(local=eye), dict(local=eye, pal=pal)]) == 604
    two = br.pack_clip([tk(1, 'T', [0, 1], np.zeros((2, 3)))])                  # an object clip names target 0 alone
    assert verdict([dict(local=eye), dict(motion=(two, ok, None, None))]) == 103
    w = br.pack_clip([tk(None, 'W', [0, 1], np.zeros((2, 1)))])
    assert verdict([dict(motion=(w, ok, None, None))]) == 104
    assert verdict([dict(local=eye), dict(motion=(clip, ok, [0, 0, np.nan, 0, 0, 0, 1, 1, 1, 1], None))]) == 501
    assert verdict([dict(local=eye), dict(motion=(clip, ok, [0, 0, 0, 0, 0, 0, 0, 1, 1, 1], None))]) == 502
    assert verdict([dict(local=eye), dict(motion=(clip, (0.0, np.inf, True), None, None))]) == 504
    assert verdict([dict(local=eye), dict(motion=(clip, ok, None, bad))]) == 603   # (a base is a local matrix)


def test_rule_check_program_builds_and_passes(tmp_path):
    '''tools/hierarchy_rule_check.cpp, a stand-alone program over anim_rule.h, built with the host's address and undefined-behaviour
    sanitizers and run'''
    import shutil
    import subprocess
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'hierarchy_rule_check')
    subprocess.run([cxx, '-std=c++17', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tools', 'hierarchy_rule_check.cpp'), '-o', exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and ' 0 failures' in run.stdout, run.stderr[-2000:]

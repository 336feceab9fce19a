'''
CPU tests of clip blending and object motion: the pure functions of the host runtime (mpt_anim_blend_rule,
mpt_motion_rule: no context, no GPU) against the restatement the GPU tests hold the kernels to (tests/anim_blend_ref.py) -- bit for bit
wherever the slerp's theta branch is not taken, within the first-order bound with the host library's measured error where it is --
the identities at weight 0 and 1 against mpt_anim_rule, every refusal that needs no device, and the rule alone under the host
sanitizers (tools/anim_blend_rule_check.cpp).
'''

import os
import re

import numpy as np
import pytest

import anim_ref as ar
import anim_blend_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('mpt_object_set_animation_blend', 'mpt_scene_add_object_clip', 'mpt_object_set_motion', 'mpt_get_object_world', 'mpt_anim_blend_stats',
       'mpt_motion_kernel_time', 'mpt_anim_blend_rule', 'mpt_motion_rule')


@pytest.fixture(scope='module')
def bcases():
    return br.blend_cases()


@pytest.fixture(scope='module')
def mcases():
    return br.motion_cases()


def _skel(skel):
    return skel if skel is not None else (np.zeros(0, np.int32), np.zeros((0, 10)), np.zeros((0, 3, 4)))


def _blend(skel, T, a, ba, b, bb, fade, t):
    from ptina_amd import _lib
    return _lib.anim_blend_rule(*_skel(skel), T, br.pack_clip(a), ba, br.pack_clip(b), bb, fade, t)


def _motion(tracks, binding, rest, base, t):
    from ptina_amd import _lib
    return _lib.motion_rule(br.pack_clip(tracks), binding, rest, base, t)


def test_header_ctypes_table_and_library_carry_the_new_calls():
    from ptina_amd import _lib, worker
    from ptina_amd.things import ModelPool
    lib = _lib.load_library()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'miptina.h')).read(), flags=re.S)
    for s in NEW:
        assert re.search(r'\bint %s\s*\(' % s, header), s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
    assert 'mpt_anim_blend_info;' in header
    assert [f for f, _ in _lib.AnimInfo._fields_] == ['skeletons', 'clips', 'tracks', 'bound_objects', 'evaluated_objects']     # (mpt_anim_info keeps its layout)
    for f in ('set_object_animation_blend', 'add_object_clip', 'set_object_motion'):
        assert callable(getattr(worker, f))
    for f in ('set_animation_blend', 'add_object_clip', 'set_motion', 'world_to_numpy', 'anim_blend_stats'):
        assert callable(getattr(ModelPool, f))


def test_weight_follows_the_fade():
    w = br.weight
    assert w(1.0, 0.25, 0.75, 2.0, 1.0) == 0.25 and w(1.0, 0.25, 0.75, 1.0, 0.5) == 0.25 and w(1.0, 0.25, 0.75, 0.5, 0.5) == 0.75
    assert w(1.0, 0.0, 1.0, -3.0, 1.0) == 1.0 and w(1.0, 0.0, 1.0, 0.5, 2.0) == 0.25
    assert w(1.0, 0.125, 0.875, 1.0, 0.0) == 0.875 and w(1.0, 0.125, 0.875, 1.5, 0.0) == 0.125 and w(1.71, 0.125, 0.875, 1.5, 0.0) == 0.875
    assert w(1.0, 0.9, 0.2, 0.75, 1.0) == 0.9 + 0.25 * (0.2 - 0.9)
    fades = br.fades()
    got = {w(1.0, *f) for f in fades}
    assert {0.0, 1.0, 0.5, br.W_LO, br.W_HI} <= got and any(f[0] > f[1] for f in fades)


def test_no_case_is_left_undecided_by_the_nlerp_branch(bcases):
    '''every d of the blend's nlerp that is computed from a rotation carrying a theta-branch bound exceeds its own bound, so that
    both sides take the same branch: with the restatement alone, before anything is compared against it'''
    br.undecided[0] = br._decided[0] = 0
    for name, skel, T, a, b, objs, exact in bcases:
        for ba, bb, fade in objs:
            for t in br.TIMES:
                if br.blend_pose(skel, T, a, ba, b, bb, fade, t)[2]:
                    br.blend_bound(skel, T, a, ba, b, bb, fade, t, ar.ULP_TRIG_DEVICE, ar.ULP_TRIG_HOST)
    print('nlerp branches on rotations that carry a bound: %d decided, %d undecided' % (br._decided[0], br.undecided[0]))
    assert br.undecided[0] == 0
    assert br._decided[0] >= 20, 'no case carries a theta-branch error into the blend'


def test_blend_rule_equals_the_restatement(bcases):
    n = theta_n = 0
    worst = 0.0
    br.undecided[0] = 0
    for name, skel, T, a, b, objs, exact in bcases:
        for ba, bb, fade in objs:
            for t in br.TIMES:
                got = _blend(skel, T, a, ba, b, bb, fade, t)
                theta, ratio = br.check_blend(got, skel, T, a, ba, b, bb, fade, t, ar.ULP_TRIG_HOST, '%s %s %s %s t %g' % (name, ba, bb, fade, t))
                assert theta == 0 or not exact, (name, 'a case that claims to be exact takes the theta branch')
                assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
                n += theta == 0
                theta_n += theta > 0
                worst = max(worst, ratio)
    print('%d poses bit for bit, %d on the theta branch with largest |rule - restatement| / bound %.4f' % (n, theta_n, worst))
    assert n >= 100 and theta_n >= 20 and br.undecided[0] == 0


def test_weight_0_is_clip_a_alone_and_weight_1_clip_b_alone_bit_for_bit(bcases):
    from ptina_amd import _lib
    n = 0
    for name, skel, T, a, b, objs, exact in bcases:
        for ba, bb, fade in objs[:4]:
            for t in br.TIMES:
                for w, tracks, bind in ((0.0, a, ba), (1.0, b, bb)):
                    got = _blend(skel, T, a, ba, b, bb, (w, w, 0.0, 0.0), t)
                    want = _lib.anim_rule(*_skel(skel), T, *br.pack_clip(tracks), *bind, t)
                    assert br.same_bits(got[0], want[0]) and br.same_bits(got[1], want[1]), (name, w, t)
                # ... and behind a finished fade from 0.3 the pose is B's
                got = _blend(skel, T, a, ba, b, bb, (0.3, 1.0, t - 1.0, 0.5), t)
                want = _lib.anim_rule(*_skel(skel), T, *br.pack_clip(b), *bb, t)
                assert br.same_bits(got[0], want[0]) and br.same_bits(got[1], want[1]), (name, 'fade', t)
                n += 1
    assert n >= 50


def test_motion_rule_equals_the_restatement(mcases):
    n = theta_n = 0
    for name, tracks, rest, base, binds, exact in mcases:
        for b in binds:
            for t in br.TIMES:
                got = _motion(tracks, b, rest, base, t)
                theta, ratio = br.check_world(got, tracks, b, rest, base, t, ar.ULP_TRIG_HOST, '%s %s t %g' % (name, b, t))
                assert theta == 0 or not exact, name
                assert np.isfinite(got).all()
                n += theta == 0
                theta_n += theta > 0
    assert n >= 80 and theta_n >= 10


def test_cases_cover_the_corners_they_name(bcases, mcases):
    assert sorted({len(c[1][0]) for c in bcases if c[1] is not None}) == [1, 3, 4, 64, 256]
    assert {c[2] for c in bcases} >= {0, 1, 3, 64} and any(c[1] is None and c[2] for c in bcases)
    for side in (3, 4):
        assert {(tr.path, tr.interpolation) for c in bcases for tr in c[side]} >= {(p, i) for p in range(3) for i in range(3)}
    assert any(not c[3] for c in bcases) and any(not c[4] for c in bcases)
    by = {c[0]: c for c in bcases}
    assert len(by['chain of 256'][3]) == len(by['chain of 256'][4]) == 768
    ja, jb = ({tr.target for tr in by['three joints, disjoint'][k]} for k in (3, 4))
    assert ja - jb and jb - ja
    a, b = by['rotation pairs'][3], by['rotation pairs'][4]
    d = [float(np.dot(x.values[0].astype(np.float64), y.values[0].astype(np.float64))) for x, y in zip(a, b)]
    assert d[0] < 0 and d[1] == 0.0 and np.array_equal(a[2].values, b[2].values)
    assert abs(np.linalg.norm(a[3].values[0]) - 2.0) < 1e-6 and abs(np.linalg.norm(b[3].values[0]) - 0.5) < 1e-6
    # both clips looping with different spans and speeds, one negative
    assert any(ba[2] and bb[2] and bb[1] < 0 for c in bcases if c[3] and c[4] for ba, bb, f in c[5])
    spans = [{br.span(c[k]) for c in bcases if c[k] and c[0] != 'rotation pairs'} for k in (3, 4)]
    assert spans == [{(0.0, 2.0)}, {(0.0, 3.0)}]
    # motion: T, R, S alone, all three, none; every interpolation; both branches of the slerp; an identity, an affine and a general base
    paths = [tuple(sorted(tr.path for tr in c[1])) for c in mcases]
    assert {(0,), (1,), (2,), (0, 1, 2), ()} <= set(paths)
    assert {tr.interpolation for c in mcases for tr in c[1]} == {0, 1, 2}
    assert any(c[3] is None for c in mcases) and any(c[3] is not None and list(np.asarray(c[3])[3]) != [0, 0, 0, 1] for c in mcases)
    taus = [ar.local_time(1.0, *b, 0.0, 2.0) for b in mcases[0][4]]
    assert 0.0 in taus and min(taus) < 0.0 and max(taus) > 2.0 and (-1.0, 1.0, True) in mcases[0][4]      # before, on and behind the keys; the wrap at t1


def test_rules_refuse_by_number():
    from ptina_amd import _lib
    tk = br.track
    one = ([-1], [br.REST0], np.zeros((1, 3, 4)))
    clip = br.pack_clip([tk(0, 'T', [0, 1], np.zeros((2, 3)))])
    none = br.pack_clip([])
    ok = (0.0, 1.0, True)

    def verdict(fn, *a):
        with pytest.raises(ValueError) as e:
            fn(*a)
        return int(str(e.value).rsplit(' ', 1)[1])
    B = _lib.anim_blend_rule
    assert verdict(B, *one, 0, clip, ok, none, ok, (-0.1, 1.0, 0.0, 0.0), 0.0) == 403
    assert verdict(B, *one, 0, clip, ok, none, ok, (0.0, 1.5, 0.0, 0.0), 0.0) == 403
    assert verdict(B, *one, 0, clip, ok, none, ok, (0.0, np.nan, 0.0, 0.0), 0.0) == 403
    assert verdict(B, *one, 0, clip, ok, none, ok, (0.0, 1.0, 0.0, -1.0), 0.0) == 402
    assert verdict(B, *one, 0, clip, ok, none, ok, (0.0, 1.0, np.inf, 1.0), 0.0) == 401
    assert verdict(B, *one, 0, clip, ok, none, (np.nan, 1.0, True), (0.0, 1.0, 0.0, 1.0), 0.0) == 401
    bad = br.pack_clip([tk(1, 'T', [0, 1], np.zeros((2, 3)))])                      # a joint beyond the skeleton
    assert verdict(B, *one, 0, bad, ok, none, ok, (0.0, 1.0, 0.0, 1.0), 0.0) == 103
    assert verdict(B, *one, 0, clip, ok, bad, ok, (0.0, 1.0, 0.0, 1.0), 0.0) == 303
    assert verdict(B, [0], [br.REST0], np.zeros((1, 3, 4)), 0, clip, ok, none, ok, (0.0, 1.0, 0.0, 1.0), 0.0) == 203
    M = _lib.motion_rule
    assert verdict(M, bad, ok, None, None, 0.0) == 103                               # an object clip names target 0 alone
    w = br.pack_clip([tk(None, 'W', [0, 1], np.zeros((2, 1)))])
    assert verdict(M, w, ok, None, None, 0.0) == 104                                 # ... and has no W track
    assert verdict(M, clip, ok, [0, 0, np.nan, 0, 0, 0, 1, 1, 1, 1], None, 0.0) == 501
    assert verdict(M, clip, ok, [0, 0, 0, 0, 0, 0, 0, 1, 1, 1], None, 0.0) == 502
    base = np.eye(4)
    base[2, 1] = np.inf
    assert verdict(M, clip, ok, None, base, 0.0) == 503
    assert verdict(M, clip, (0.0, np.inf, True), None, None, 0.0) == 504
    assert br.same_bits(M(none, ok, None, None, 3.0), np.eye(4))


def test_rule_check_program_builds_and_passes(tmp_path):
    '''tools/anim_blend_rule_check.cpp, a stand-alone program over anim_rule.h, built with the host's address and undefined-behaviour
    sanitizers and run'''
    import shutil
    import subprocess
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'anim_blend_rule_check')
    subprocess.run([cxx, '-std=c++17', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tools', 'anim_blend_rule_check.cpp'), '-o', exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and ' 0 failures' in run.stdout, run.stderr[-2000:]

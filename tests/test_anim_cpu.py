'''
CPU tests of keyframe animation: the pure functions of the host runtime (mpt_anim_rule, mpt_clip_check: no
context, no GPU) against the restatement the GPU tests hold the kernel to (tests/anim_ref.py) -- bit for bit wherever the slerp's
theta branch is not taken, within anim_ref.error_bound with the host library's measured error where it is -- and the rule against
tools.skin.joint_matrices and exams/deform_amd.py's palette.
'''

import os
import re

import numpy as np
import pytest

import anim_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('mpt_mesh_set_skeleton', 'mpt_mesh_add_clip', 'mpt_object_set_animation', 'mpt_scene_set_time', 'mpt_get_pose', 'mpt_anim_stats',
       'mpt_anim_kernel_time', 'mpt_anim_rule', 'mpt_clip_check')


@pytest.fixture(scope='module')
def cases():
    return ar.cases()


def _rule(skel, T, tracks, binding, t):
    from ptina_amd import _lib
    parents, rest, ib = skel if skel is not None else (np.zeros(0, np.int32), np.zeros((0, 10)), np.zeros((0, 3, 4)))
    return _lib.anim_rule(parents, rest, ib, T, *ar.pack_clip(tracks), *binding, t)


def test_header_ctypes_table_and_library_carry_the_new_calls():
    from ptina_amd import _lib
    lib = _lib.load_library()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'miptina.h')).read(), flags=re.S)
    for s in NEW:
        assert re.search(r'\bint %s\s*\(' % s, header), s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
    from ptina_amd import worker
    for f in ('set_mesh_skeleton', 'add_mesh_clip', 'set_object_animation', 'set_scene_time'):
        assert callable(getattr(worker, f))


def test_rule_equals_the_restatement_bit_for_bit_off_the_theta_branch(cases):
    n = 0
    for name, skel, T, tracks, binds, exact in cases:
        for b in binds:
            for t in ar.TIMES:
                w, pal, theta = ar.pose(skel, T, tracks, b, t)
                assert (theta == 0) == exact or not exact, (name, b, t, 'a case that claims to be exact takes the theta branch')
                if theta:
                    continue
                gw, gp = _rule(skel, T, tracks, b, t)
                assert ar.same_bits(gw, w) and ar.same_bits(gp, pal), (name, b, t)
                assert np.isfinite(pal).all() and np.isfinite(w).all()
                n += 1
    assert n > 100


def test_rule_stays_within_the_bound_on_the_theta_branch(cases):
    n, worst = 0, 0.0
    for name, skel, T, tracks, binds, exact in cases:
        if exact:
            continue
        for b in binds:
            for t in ar.TIMES:
                theta, ratio = ar.check_pose(_rule(skel, T, tracks, b, t), skel, T, tracks, b, t, ar.ULP_TRIG_HOST, '%s %s t %g' % (name, b, t))
                n += theta > 0
                worst = max(worst, ratio)
    print('theta branch: %d poses, largest |rule - restatement| / bound %.4f' % (n, worst))
    assert n >= 20, 'the theta cases do not take the theta branch'


def test_cases_cover_the_corners_they_name(cases):
    '''the local times the bindings promise, the slerp's corners, every interpolation on every path'''
    by = {c[0]: c for c in cases}
    seen = {(tr.path, tr.interpolation) for c in cases for tr in c[3]}
    assert seen == {(p, i) for p in range(4) for i in range(3)}
    assert {tr.times.size for c in cases for tr in c[3]} >= {1, 2, 33}
    assert sorted({len(c[1][0]) for c in cases if c[1] is not None}) == [1, 3, 5, 64, 256]
    name, skel, T, tracks, binds, _ = by['five joints, two roots']
    t0, t1 = ar.span(tracks)
    assert (t0, t1) == (0.0, 2.0) and list(skel[0]) == [-1, -1, 0, 1, 2]
    tau = [ar.local_time(1.0, *b, t0, t1) for b in binds]
    k = float(tracks[0].times[tracks[0].times.size // 2])
    assert tau[:3] == [1.0, 0.0, 0.0] and tau[3] == tau[4] == k and tau[5:8] == [-2.0, 5.0, 0.0] and tau[8] == 1.25 and tau[9] == 1.0 and tau[10] == 2.75
    assert ar.key([float(x) for x in tracks[0].times], k) == (tracks[0].times.size // 2, None) or ar.key([float(x) for x in tracks[0].times], k)[1][1] == 0.0
    # the slerp's corners
    def dots(c):
        return [float(np.dot(tr.values[0].astype(np.float64), tr.values[1].astype(np.float64))) for tr in c[3]]
    d = dots(by['slerp corners, nlerp'])
    assert d[0] < -ar.THETA_D and d[1] == 1.0 and ar.THETA_D < d[2] < ar.THETA_D + 1e-6
    d = dots(by['slerp corners, theta'])
    assert -ar.THETA_D < d[0] < 0 and ar.THETA_D - 1e-6 < d[1] <= ar.THETA_D and d[2] == 0.0


def test_host_trig_stays_within_its_measured_error(cases):
    '''the host library's acos and sin over the arguments the theta cases hand them, against np.longdouble: half of ULP_TRIG_HOST
    covers the largest error seen (the constant is twice that, rounded up)'''
    import math

    def walk():
        for name, skel, T, tracks, binds, exact in cases:
            if not exact:
                for b in binds:
                    for t in ar.TIMES:
                        ar.pose(skel, T, tracks, b, t)
    args = ar.record_trig(walk)
    assert args['acos'].size >= 20 and args['sin'].size == 3 * args['acos'].size
    assert args['acos'].max() <= ar.THETA_D and args['acos'].min() >= 0.0
    ea = ar.trig_ulps(args['acos'], [math.acos(x) for x in args['acos']], 'acos').max()
    es = ar.trig_ulps(args['sin'], [math.sin(x) for x in args['sin']], 'sin').max()
    print('host libm over %d + %d arguments: acos within %.4f ulp, sin within %.4f ulp' % (args['acos'].size, args['sin'].size, ea, es))
    assert 2 * max(ea, es) <= ar.ULP_TRIG_HOST


def test_clip_check_accepts_and_refuses():
    from ptina_amd import _lib
    tk = ar.track
    q = [[0, 0, 0, 1], [0, 1, 0, 0]]
    good = [tk(0, 'T', [0, 1], [[0, 0, 0], [1, 2, 3]]), tk(1, 'R', [0, 1], q), tk(1, 'S', [0.5], [[1, 1, 1]], 'STEP'),
            tk(None, 'W', [0, 1, 2], np.zeros((3, 3, 2)), 'CUBICSPLINE')]

    def check(tracks, nj=2, T=2, edit=None):
        spec, times, values = ar.pack_clip(tracks)
        if edit:
            edit(spec, times, values)
        return _lib.clip_check(nj, T, spec, times, values)
    assert check(good) == (0, '') and check([]) == (0, '') and check(good[3:], nj=0) == (0, '')
    rc, why = check(good, edit=lambda s, t, v: t.__setitem__(1, np.nan))
    assert rc == 6 and 'times[1] of tracks[0] is not finite' in why
    rc, why = check(good, edit=lambda s, t, v: t.__setitem__(3, 0.0))
    assert rc == 7 and 'times[1] of tracks[1]' in why and 'increase strictly' in why
    rc, why = check(good, edit=lambda s, t, v: t.__setitem__(6, 0.0))            # equal neighbours are not increasing
    assert rc == 7 and 'tracks[3]' in why
    rc, why = check(good, nj=1)
    assert rc == 3 and 'tracks[1] names joint 1, beyond njoints 1' in why
    rc, why = check(good[:1], edit=lambda s, t, v: s.__setitem__((0, 0), -1))
    assert rc == 3 and 'names joint -1' in why
    rc, why = check(good, T=0)
    assert rc == 4 and 'tracks[3] animates the morph weights of a mesh without morph targets' in why
    rc, why = check(good[3:], edit=lambda s, t, v: s.__setitem__((0, 0), 0))
    assert rc == 3 and 'target must be -1' in why
    rc, why = check(good + [tk(1, 'R', [0], [[0, 0, 0, 1]])])
    assert rc == 8 and 'tracks[1] and tracks[4] animate the same target and path' in why
    rc, why = check(good[:2], edit=lambda s, t, v: v.__setitem__(slice(10, 14), 0.0))
    assert rc == 9 and 'rotation values of key 1 of tracks[1] are zero' in why
    cub = [tk(0, 'R', [0, 1], np.float32([[[0] * 4, [0, 0, 0, 1], [0] * 4], [[0] * 4, [0] * 4, [1, 1, 1, 1]]]), 'CUBICSPLINE')]
    rc, why = check(cub)                                                         # zero tangents are fine, a zero value is not
    assert rc == 9 and 'key 1 of tracks[0]' in why
    rc, why = check(good, edit=lambda s, t, v: v.__setitem__(2, np.inf))
    assert rc == 10 and 'values[2] of tracks[0] is not finite' in why
    rc, why = check(good, edit=lambda s, t, v: s.__setitem__((2, 3), 0))
    assert rc == 5 and 'tracks[2] has 0 keys' in why
    for col, word in ((1, 'path 7'), (2, 'interpolation 7')):
        rc, why = check(good, edit=lambda s, t, v, col=col: s.__setitem__((0, col), 7))
        assert rc == 2 and word in why
    spec, times, values = ar.pack_clip(good)
    assert _lib.clip_check(2, 2, spec, times[:-1], values)[0] == 1 and _lib.clip_check(2, 2, spec, times, np.append(values, 0))[0] == 1
    with pytest.raises(ValueError, match='verdict 203'):                         # mpt_anim_rule runs the same checks: parents out of order
        _lib.anim_rule([0, -1], np.tile([0, 0, 0, 0, 0, 0, 1, 1, 1, 1.0], (2, 1)), np.zeros((2, 3, 4)), 0, *ar.pack_clip([]), 0, 1, True, 0)
    with pytest.raises(ValueError, match='verdict 107'):
        _lib.anim_rule([-1], [[0, 0, 0, 0, 0, 0, 1, 1, 1, 1.0]], np.zeros((1, 3, 4)), 0, *ar.pack_clip([tk(0, 'T', [1, 0], np.zeros((2, 3)))]), 0, 1, True, 0)


def test_rest_pose_clip_gives_joint_matrices():
    from ptina_amd.tools.skin import joint_matrices
    from ptina_amd.tools.anim import local_matrices, rest_pose
    g = np.random.default_rng(8)
    parents, rest, ib = ar.skeleton(g, 12, 'tree')
    w, pal = _rule((parents, rest, ib), 0, [], (0.3, 1.0, True), 0.7)
    ib4 = np.concatenate([ib, np.tile([[[0, 0, 0, 1.0]]], (12, 1, 1))], axis=1)
    want = joint_matrices(parents, local_matrices(rest[:, :3], rest[:, 3:7], rest[:, 7:]), ib4)
    assert w.shape == (0,) and np.allclose(pal, want[:, :3], rtol=1e-13, atol=1e-14)
    # identity rest and inverse bind: the identity palette's bits
    t, r, s = rest_pose(12)
    eye = np.tile(np.eye(4)[:3], (12, 1, 1))
    w, pal = _rule((parents, np.concatenate([t, r, s], axis=1), eye), 0, [], (0.0, 1.0, True), 5.0)
    assert ar.same_bits(pal, eye)


def test_linear_rotation_about_z_reproduces_the_bending_tube():
    '''exams/deform_amd.py's palette(bend): a chain of 8 joints up a tube, each turned by bend / 8 about z against its parent --
    here as one clip of LINEAR rotation tracks from no bend at time 0 to the full bend at time 1, read at time 1 (the key itself)
    and half way (the slerp of a rotation about one axis: half the angle)'''
    from ptina_amd.tools.skin import joint_matrices
    from ptina_amd.tools.anim import quaternion
    J, H, bend = 8, 2.4, 1.2
    seg = H / J

    def shift(x, y, z):
        m = np.eye(4)
        m[:3, 3] = [x, y, z]
        return m

    def palette(bend):
        c, s = np.cos(bend / J), np.sin(bend / J)
        turn = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
        local = np.stack([shift(0, 0 if j == 0 else seg, 0) @ turn for j in range(J)])
        return joint_matrices(np.arange(J) - 1, local, np.stack([shift(0, -j * seg, 0) for j in range(J)]))
    parents = np.arange(J) - 1
    rest = np.tile([0, 0, 0, 0, 0, 0, 1, 1, 1, 1.0], (J, 1))
    rest[1:, 1] = seg
    ib = np.stack([shift(0, -j * seg, 0)[:3] for j in range(J)])
    tracks = [ar.track(j, 'R', [0, 1], [[0, 0, 0, 1], quaternion([0, 0, 1], bend / J)]) for j in range(J)]
    for t, b in ((1.0, bend), (0.5, 0.5 * bend), (0.0, 0.0), (7.0, bend)):
        w, pal = _rule((parents, rest, ib), 0, tracks, (0.0, 1.0, False), t)
        assert np.allclose(pal, palette(b)[:, :3], rtol=0, atol=2e-7), (t, np.abs(pal - palette(b)[:, :3]).max())   # the keys are f32


def test_rule_check_program_builds_and_passes(tmp_path):
    '''tools/anim_rule_check.cpp, a stand-alone program over anim_rule.h, built with the host's address and undefined-behaviour
    sanitizers and run'''
    import shutil
    import subprocess
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'anim_rule_check')
    subprocess.run([cxx, '-std=c++17', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tools', 'anim_rule_check.cpp'), '-o', exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and ' 0 failures' in run.stdout, run.stderr[-2000:]

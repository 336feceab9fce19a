'''what the tests of clip blending and object motion share (tests/test_anim_blend_cpu.py, tests/test_anim_blend_gpu.py): a restatement
of the additions to ptina_amd/csrc/anim_rule.h -- the weight of a second binding at scene time t, the blend
of two clips' T, R, S and morph weights, and the world matrix of an object moved by an object clip -- scalar by scalar in f64 in the
written order, on top of tests/anim_ref.py's restatement of the sampler, the local matrix and the products (imported, not edited).

As anim_ref, the same code runs over float and over Err.  Off the slerp's theta branch (a LINEAR rotation track of either clip, or of
the object clip, between two keys further apart than d = 0.9995) everything is held BIT FOR BIT; on it, to the first-order bound: for
poses carried through the blend entry by entry and down the chain in norms (anim_ref._product_bound), for a world matrix entrywise
through the local matrix and the one product.  No new tolerance: the library errors are anim_ref's measured ULP_TRIG_HOST / _DEVICE.

The blend's nlerp branches on d < 0 of two sampled rotations, which may now carry a theta-branch error: a case decides something only if
|d| exceeds d's own bound, so that both sides branch alike.  Every such d is checked and the undecided ones are counted in
`undecided`; the case generators are held to a count of 0 (test_anim_blend_cpu.py).'''

import numpy as np

import anim_ref
from anim_ref import (sample, local, mul, local_time, span, Err, _sqrt, _product_bound, same_bits,          # noqa: F401
                      ULP_TRIG_HOST, ULP_TRIG_DEVICE, CAP, Track, track, pack_clip)

TIMES = (1.0, 1.71)            # the scene times the cases are evaluated at
EYE = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
REST0 = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0]
undecided = [0]                # nlerp branches whose d does not exceed its own bound (see above), since the module was loaded
_decided = [0]                 # ... and those that carried a bound and did


# ---------------------------------------------------------------- A. blending
def weight(t, w0, w1, fade_start, fade_duration):
    '''the weight of the second binding at scene time t'''
    if fade_duration > 0.0:
        x = (t - fade_start) / fade_duration
        s = 0.0 if x < 0.0 else 1.0 if x > 1.0 else x
    else:
        s = 1.0 if t >= fade_start else 0.0
    if s == 0.0:
        return w0
    if s == 1.0:
        return w1
    return w0 + s * (w1 - w0)


def _carries(q):
    return any(isinstance(c, Err) and c.e > 0.0 for c in q)


def blend_rotation(a, b, w):
    '''the normalised lerp over the shorter arc'''
    d = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]
    if _carries(a) or _carries(b):
        if abs(d.v) > d.e:
            _decided[0] += 1
        else:
            undecided[0] += 1
    if d < 0.0:
        b = [-c for c in b]
    q = [a[c] + w * (b[c] - a[c]) for c in range(4)]
    ln = _sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [c / ln for c in q]


def blend_values(a, b, w):
    return [a[c] + w * (b[c] - a[c]) for c in range(len(a))]


def _sampled(rest, ntargets, tracks, binding, t, N):
    '''(weights, the joints' T R S as 10 numbers each) of one clip at scene time t: a track at the binding's local time, else the rest
    value, 0 for the weights'''
    offset, speed, loop = binding
    tau = local_time(float(t), float(offset), float(speed), bool(loop), *span(tracks))
    trs = [[N(float(x)) for x in r] for r in rest]
    w = [N(0.0)] * ntargets
    for tr in tracks:
        v = sample(tr, ntargets, tau, N)
        if tr.path == 3:
            w = v
        else:
            at = (0, 3, 7)[tr.path]
            trs[tr.target][at:at + len(v)] = v
    return w, trs


def _skel(skel):
    parents, rest, ib = skel if skel is not None else (np.zeros(0, np.int64), np.zeros((0, 10)), np.zeros((0, 3, 4)))
    nj = len(parents)
    return parents, np.asarray(rest, np.float64).reshape(nj, 10), np.asarray(ib, np.float64).reshape(nj, 12)


def _blended(skel, ntargets, tracks_a, bind_a, tracks_b, bind_b, fade, t, N):
    '''(weights, the joints' local matrices, parents, inverse binds) of the blend at scene time t; fade = (w0, w1, start, duration)'''
    parents, rest, ib = _skel(skel)
    wa, A = _sampled(rest, ntargets, tracks_a, bind_a, t, N)
    wb, B = _sampled(rest, ntargets, tracks_b, bind_b, t, N)
    w = weight(float(t), *[float(x) for x in fade])
    if w == 0.0:
        wt, trs = wa, A
    elif w == 1.0:
        wt, trs = wb, B
    else:
        wt = blend_values(wa, wb, w)
        trs = [blend_values(a[0:3], b[0:3], w) + blend_rotation(a[3:7], b[3:7], w) + blend_values(a[7:10], b[7:10], w) for a, b in zip(A, B)]
    return wt, [local(x) for x in trs], parents, ib


def blend_pose(skel, ntargets, tracks_a, bind_a, tracks_b, bind_b, fade, t):
    '''(weights [ntargets], palette [nj,3,4], theta) f64 of an object with two bindings at scene time t; theta: how often either clip's
    sampling took the slerp's theta branch (0: reproducible bit for bit)'''
    anim_ref._state['theta'] = 0
    w, loc, parents, ib = _blended(skel, ntargets, tracks_a, bind_a, tracks_b, bind_b, fade, t, float)
    glob, pal = [], []
    for j, G in enumerate(loc):
        if parents[j] >= 0:
            G = mul(glob[int(parents[j])], G)
        glob.append(G)
        pal.append(mul(G, [float(x) for x in ib[j]]))
    return np.array(w, np.float64).reshape(ntargets), np.array(pal, np.float64).reshape(len(pal), 3, 4), anim_ref._state['theta']


def blend_bound(skel, ntargets, tracks_a, bind_a, tracks_b, bind_b, fade, t, ulp_a, ulp_b):
    '''(weights' bounds, palette's bounds [nj,3,4]) between two evaluations whose acos and sin miss by ulp_a and ulp_b units in the last
    place: entry by entry through sampling, blend and local matrices, in norms down the chain, as anim_ref.error_bound'''
    anim_ref._state['ulps'] = float(ulp_a + ulp_b)
    w, loc, parents, ib = _blended(skel, ntargets, tracks_a, bind_a, tracks_b, bind_b, fade, t, Err)
    nj = len(loc)
    out = np.zeros((nj, 3, 4))
    glob = []
    for j in range(nj):
        G = np.array([x.v for x in loc[j]]).reshape(3, 4)
        e = np.array([x.e for x in loc[j]]).reshape(3, 4)
        eG = (float(np.linalg.norm(e[:, :3])), float(np.linalg.norm(e[:, 3])))
        if parents[j] >= 0:
            P, eP = glob[int(parents[j])]
            eG = _product_bound(P, eP, G, eG)
            G = np.array(mul(list(P.reshape(-1)), list(G.reshape(-1)))).reshape(3, 4)
        glob.append((G, eG))
        out[j, :, :3], out[j, :, 3] = _product_bound(G, eG, ib[j].reshape(3, 4), (0.0, 0.0))
    return np.array([x.e for x in w], np.float64).reshape(ntargets), out


def _held(got, want, bound, what, theta):
    '''|got - want| <= bound entry by entry, the bound capped at CAP x the largest entry (asserted); returns the largest ratio'''
    scale = float(np.abs(want).max())
    assert bound.max() <= CAP * scale, (what, 'the bound exceeds the cap: the derivation is wrong', float(bound.max()), scale)
    diff = np.abs(got - want)
    ratio = float((diff[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print('%s: theta branch x%d, bound <= %.3g (%.3g of the largest entry), largest |got - restatement| / bound %.4f'
          % (what, theta, bound.max(), bound.max() / scale, ratio))
    assert np.all(diff <= bound), (what, ratio, float(diff.max()))
    return ratio


def check_blend(got, skel, ntargets, tracks_a, bind_a, tracks_b, bind_b, fade, t, ulp_got, what=''):
    '''holds got = (weights, palette) to the restatement: bit for bit off the theta branch, within blend_bound (capped) on it.  Returns
    (theta, the largest |got - restatement| / bound, or 0.0)'''
    w, pal, theta = blend_pose(skel, ntargets, tracks_a, bind_a, tracks_b, bind_b, fade, t)
    if theta == 0:
        assert same_bits(got[0], w) and same_bits(got[1], pal), (what, 'not the restatement\'s bits', np.abs(got[1] - pal).max() if pal.size else 0,
                                                                 np.abs(got[0] - w).max() if w.size else 0)
        return 0, 0.0
    ew, ep = blend_bound(skel, ntargets, tracks_a, bind_a, tracks_b, bind_b, fade, t, ulp_got, ULP_TRIG_HOST)
    assert same_bits(got[0], w), (what, 'weights do not pass the slerp')
    return theta, _held(got[1], pal, ep, what, theta)


# ---------------------------------------------------------------- B. the motion of an object
def _world(tracks, binding, rest, base, t, N):
    '''the 16 numbers of base . [local(trs); 0 0 0 1], trs the rest overwritten by the object clip's tracks at the local time'''
    _, trs = _sampled([rest], 0, tracks, binding, t, N)
    L = local(trs[0])
    B = [float(x) for x in np.asarray(base, np.float64).reshape(16)]
    W = []
    for r in range(4):
        W += [(B[4 * r] * L[c] + B[4 * r + 1] * L[4 + c]) + B[4 * r + 2] * L[8 + c] for c in range(3)]
        W.append(((B[4 * r] * L[3] + B[4 * r + 1] * L[7]) + B[4 * r + 2] * L[11]) + B[4 * r + 3])
    return W


def motion_world(tracks, binding, rest, base, t):
    '''(world [4,4] f64, theta) of an object bound to an object clip at scene time t'''
    anim_ref._state['theta'] = 0
    W = _world(tracks, binding, REST0 if rest is None else rest, EYE if base is None else base, t, float)
    return np.array(W, np.float64).reshape(4, 4), anim_ref._state['theta']


def motion_bound(tracks, binding, rest, base, t, ulp_a, ulp_b):
    anim_ref._state['ulps'] = float(ulp_a + ulp_b)
    W = _world(tracks, binding, REST0 if rest is None else rest, EYE if base is None else base, t, Err)
    return np.array([x.e for x in W], np.float64).reshape(4, 4)


def check_world(got, tracks, binding, rest, base, t, ulp_got, what=''):
    '''holds got [4,4] to the restatement, as check_blend holds a pose; returns (theta, ratio)'''
    W, theta = motion_world(tracks, binding, rest, base, t)
    if theta == 0:
        assert same_bits(got, W), (what, 'not the restatement\'s bits', np.abs(np.asarray(got) - W).max())
        return 0, 0.0
    return theta, _held(np.asarray(got, np.float64).reshape(4, 4), W, motion_bound(tracks, binding, rest, base, t, ulp_got, ULP_TRIG_HOST), what, theta)


# ---------------------------------------------------------------- the cases both test files walk (fixed seeds)
W_LO, W_HI = 2.0 ** -53, 1.0 - 2.0 ** -53


def fades():
    '''(w0, w1, fade_start, fade_duration) for scene time 1.0: the constant weights 0, 1, 0.5, 2^-53 and 1 - 2^-53; t before, inside,
    exactly on both ends of and behind a fade; a duration of 0 with t on both sides of the start (at 1.0 on the start itself: s = 1; at
    1.5 before it at scene time 1.0 and behind it at 1.71); w0 > w1'''
    return [(0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0), (0.5, 0.5, 0.0, 1.0), (W_LO, W_LO, 0.0, 0.0), (W_HI, W_HI, 5.0, 0.0),
            (0.25, 0.75, 2.0, 1.0), (0.0, 1.0, 0.5, 2.0), (0.25, 0.75, 1.0, 0.5), (0.25, 0.75, 0.5, 0.5), (0.0, 1.0, -3.0, 1.0),
            (0.125, 0.875, 1.0, 0.0), (0.125, 0.875, 1.5, 0.0), (0.9, 0.2, 0.75, 1.0)]


def _objects(g, tracks_a, tracks_b, n=None):
    '''(binding of A, binding of B, fade) per object: anim_ref's bindings for A, others for B -- both looping with different spans and
    speeds, one negative, among them -- and the fades in turn'''
    ba = anim_ref.bindings(tracks_a)
    bb = [(0.25, 1.5, True), (0.5, -1.5, True), (0.0, 1.0, False), (-1.0, 0.5, True), (3.0, 1.0, False)]
    f = fades()
    m = len(f) if n is None else n
    return [(ba[(3 * i) % len(ba)], bb[i % len(bb)], f[i % len(f)]) for i in range(m)]


def blend_cases():
    '''[(name, skel or None, ntargets, tracks of A, tracks of B, [(binding A, binding B, fade)], exact)]; every clip of A spans [0, 2],
    those of B [0, 3]; exact -- no object of the case takes the slerp's theta branch at TIMES'''
    g = np.random.default_rng(4117)
    rt, rc, sk = anim_ref.random_track, anim_ref.random_clip, anim_ref.skeleton
    out = []
    # one joint: LINEAR on both sides, far rotations (theta on both sides, carried through the nlerp)
    a = [rt(g, 0, 0, 1, 2), rt(g, 0, 1, 1, 33, rot='far'), rt(g, 0, 2, 2, 2)]
    b = [rt(g, 0, 0, 2, 33, t_last=3.0), rt(g, 0, 1, 1, 2, rot='far', t_last=3.0), rt(g, 0, 2, 1, 33, t_last=3.0)]
    out.append(('one joint, theta', sk(g, 1), 0, a, b, _objects(g, a, b), False))
    # three joints, three targets: STEP, LINEAR (nlerp), CUBICSPLINE on both sides; disjoint joints (A: 0 and 1, B: 1 and 2 on other paths)
    a = [rt(g, 0, 0, 0, 33), rt(g, 0, 1, 2, 33), rt(g, 1, 2, 1, 2), rt(g, 1, 1, 1, 33, rot='near'), rt(g, -1, 3, 1, 33, ntargets=3)]
    b = [rt(g, 2, 0, 2, 33, t_last=3.0), rt(g, 2, 1, 0, 2, t_last=3.0), rt(g, 1, 0, 1, 33, t_last=3.0), rt(g, 2, 2, 0, 33, t_last=3.0),
         rt(g, -1, 3, 2, 2, ntargets=3, t_last=3.0)]
    out.append(('three joints, disjoint', sk(g, 3, 'star'), 3, a, b, _objects(g, a, b), True))
    # ... a clip without tracks on either side: the rest pose and weights 0 stand in
    out.append(('three joints, B empty', sk(g, 3, 'chain'), 3, a, [], _objects(g, a, [], 5), True))
    out.append(('three joints, A empty', sk(g, 3, 'chain'), 3, [], b, _objects(g, [], b, 5), True))
    # 64 joints, one target
    a = rc(g, 64, 0, rot='near') + [rt(g, -1, 3, 2, 33, ntargets=1)]
    b = rc(g, 64, 0, rot='flip', t_last=3.0) + [rt(g, -1, 3, 1, 2, ntargets=1, t_last=3.0)]
    out.append(('star of 64', sk(g, 64, 'star'), 1, a, b, _objects(g, a, b, 5), True))
    a, b = rc(g, 64, 0, rot='far', density=0.5), rc(g, 64, 0, rot='far', density=0.5, t_last=3.0)
    out.append(('tree of 64, theta', sk(g, 64, 'tree'), 0, a, b, _objects(g, a, b, 4)[1:], False))
    # a chain 256 deep, T R and S on every joint on both sides: 768 tracks a clip, three passes of 256 lanes, all of the aliased region
    a, b = rc(g, 256, 0, rot='flip', density=1.0, nkeys=(2, 33)), rc(g, 256, 0, rot='near', density=1.0, nkeys=(2, 33), t_last=3.0)
    assert len(a) == len(b) == 768
    out.append(('chain of 256', sk(g, 256, 'chain'), 0, a, b, [_objects(g, a, b)[i] for i in (2, 6, 12)], True))
    # morph targets and no skin: 64 targets, 3 targets
    a, b = [rt(g, -1, 3, 2, 33, ntargets=64)], [rt(g, -1, 3, 1, 33, ntargets=64, t_last=3.0)]
    out.append(('morph only, 64 targets', None, 64, a, b, _objects(g, a, b, 7)[2:], True))
    a, b = [rt(g, -1, 3, 0, 2, ntargets=3)], []
    out.append(('morph only, 3 targets', None, 3, a, b, _objects(g, a, b, 7)[2:], True))
    # rotation pairs, a joint each, STEP tracks of one key so that a and b are the keys themselves: d < 0 (b the negated neighbour of a),
    # d exactly 0, identical rotations, keys that are not normalised (lengths 2 and 0.5)
    q = anim_ref.rotation_keys(g, 2, 'near').astype(np.float64)
    K = lambda j, v: Track(j, 1, 0, np.float32([0.0]), np.float32([v]))                 # noqa: E731
    a = [K(0, q[0]), K(1, [0, 0, 0, 1]), K(2, q[1]), K(3, 2.0 * q[0])]
    b = [K(0, -q[1]), K(1, [1, 0, 0, 0]), K(2, q[1]), K(3, 0.5 * q[1])]
    out.append(('rotation pairs', sk(g, 4, 'star'), 0, a, b, _objects(g, a, b), True))
    return out


def motion_cases():
    '''[(name, tracks of the object clip, rest or None, base or None, [bindings], exact)]; every clip spans [0, 2]'''
    g = np.random.default_rng(977)
    rt = anim_ref.random_track
    out = []
    q = g.normal(size=4)
    rest = [0.3, -0.2, 0.1, *(q / np.linalg.norm(q)), 1.1, 0.9, 1.05]
    base = np.eye(4)
    base[:3] = np.array(local([0.5, -0.25, 2.0, 0.6, 0.0, 0.0, 0.8, 1.0, 2.0, 0.5])).reshape(3, 4)
    skew = g.uniform(-1.0, 1.0, (4, 4))                           # not affine: a bottom row of its own
    all_b = lambda tr: anim_ref.bindings(tr)                      # noqa: E731  (times before, on and behind the keys, the wrap at t1)
    tr = [rt(g, 0, 0, 1, 33)]
    out.append(('T alone, LINEAR', tr, None, None, all_b(tr), True))
    tr = [rt(g, 0, 1, 1, 33, rot='far')]
    out.append(('R alone, theta', tr, rest, base, all_b(tr), False))
    tr = [rt(g, 0, 1, 1, 33, rot='flip')]
    out.append(('R alone, nlerp', tr, rest, skew, all_b(tr), True))
    tr = [rt(g, 0, 2, 2, 33)]
    out.append(('S alone, CUBICSPLINE', tr, rest, base, all_b(tr), True))
    tr = [rt(g, 0, 0, 2, 33), rt(g, 0, 1, 2, 2), rt(g, 0, 2, 0, 33)]
    out.append(('T R S, CUBICSPLINE and STEP', tr, None, skew, all_b(tr), True))
    tr = [rt(g, 0, 0, 0, 2), rt(g, 0, 1, 1, 2, rot='far'), rt(g, 0, 2, 1, 2)]
    out.append(('T R S, theta', tr, rest, None, all_b(tr), False))
    out.append(('no tracks: base . rest', [], rest, skew, anim_ref.bindings([], 2), True))
    out.append(('no tracks, defaults: the identity', [], None, None, anim_ref.bindings([], 1), True))
    return out

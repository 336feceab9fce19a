'''
The exhaustive float64 visibility search (tests/visibility_ref.py) on the CPU: against the oracle's own walk on every scene
the GPU kernels are held to (tests/test_visibility_gpu.py imports the scenes and the checks from here), against a
per-sample float64 Moller-Trumbore over all triangles, on hand-made cases, and shown to fail when a triangle or a material
is wrong.  The oracle cases assert ZERO wrong pixels: the comparison is exact (see the module docstring of visibility_ref).
'''

import numpy as np
import pytest

import visibility_ref as vr
from ptina_amd import scenes
from ptina_amd.tools.matrix import translate, scale

WORLD = ([1.0, 0.5, 0.25, 1.0], -1)
ABSORBING = scenes.material(basecolor=(0, 0, 0), transmission=1.0)
OFFSET = np.array([300.0, -200.0, 500.0], np.float32)

# name: (n, edge, nx, ny, variant).  The classified shares below are properties of the reference alone and are asserted
# before any film is looked at (shares()); a row that misses them gets another edge or film, never another cap.
CASES = {
    'n2': (2, 0.5, 64, 64, None),
    'n3': (3, 0.5, 64, 64, None),
    'n33': (33, 0.3, 96, 80, None),
    'n300': (300, 0.2, 96, 80, None),
    'n1025': (1025, 0.12, 160, 128, None),
    'n5000': (5000, 0.06, 256, 256, None),
    'n20000': (20000, 0.03, 384, 384, None),
    'moved': (300, 0.2, 96, 80, 'moved'),           # 8-bit planes far from the origin
    'x1024': (300, 0.2, 96, 80, 'x1024'),           # LdsWalk4::T_SCALED
    'flat': (200, 0.3, 96, 80, 'flat'),             # every box flat along z: the e == 0 branch of the quantised step, a lo == hi slab
    'deep': (352, 0.5, 64, 64, 'deep'),             # a reference tree of 37 levels: the 64-level stacks of the one-lane-per-item kernels (deep_model)
}
# No scaled-down scene: at x 1/1024 the oracle itself loses every full-hit pixel to the reference's absolute epsilons
# (test_scene_scale_dependence_is_the_references pins that); an exhaustive search is not the reference there.
PREVIEW_CASES = ('n300', 'n1025', 'n5000')


def deep_model(edge):
    '''352 triangles, all facing +z, whose reference LBVH is 37 levels of inner nodes deep: 16 copies of one triangle at
    (1, 1, 1); for k = 0 .. 11 and each axis one triangle whose centre has that coordinate at 1 - 2^-(k + 1) -- its Morton code
    leaves the copies' at one bit, so every bit splits one leaf off on the left and the chain descends on the right -- and 300
    fillers of edge 1e-3 near the origin, which change nothing of the chain: the reference's walk gives up after n node
    visits (lbvh.py:324), and with the 53 triangles alone the oracle itself loses full-hit pixels.  Triangle t is
    c + (-e, -e, 0), c + (e, -e, 0), c + (0, e, 0); every centre is moved by (-0.5, 1, -0.5) into BENCH_CAMERA's view'''
    cen = [(1.0, 1.0, 1.0)] * 16
    for k in range(12):
        for a in range(3):
            c = [1.0, 1.0, 1.0]
            c[a] = 1.0 - 2.0 ** -(k + 1)
            cen.append(tuple(c))
    cen = np.concatenate([np.array(cen), np.random.default_rng(53).random((300, 3)) * 0.05]) + [-0.5, 1.0, -0.5]
    e = np.concatenate([np.full(52, float(edge)), np.full(300, 1e-3)])[:, None, None]
    P = cen[:, None, :] + e * np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
    N = np.broadcast_to([0.0, 0.0, 1.0], P.shape)
    return scenes._pack(P, N), np.zeros(P.shape[0], np.int32)


class Case:
    '''one scene: model, camera, film size, and the reference's verdicts (computed once per process, shared by every test)'''

    def __init__(self, name, preview=False):
        n, edge, nx, ny, variant = CASES[name]
        v, m = deep_model(edge) if variant == 'deep' else scenes.scene_random_tris(n, seed=n, edge=edge)[:2]
        v = np.array(v, np.float32, copy=True)
        cam = np.array(scenes.BENCH_CAMERA, np.float64)
        if variant == 'moved':
            v[:, 0:3] += OFFSET
            cam = cam @ translate(-OFFSET.astype(np.float64))
        elif variant == 'x1024':
            v[:, 0:3] *= np.float32(1024.0)
            cam = cam @ scale(1.0 / 1024.0)
        elif variant == 'flat':
            v[:, 2] = np.float32(0.0)
        self.name, self.n, self.nx, self.ny, self.camera = name, m.shape[0], nx, ny, cam
        self.pos = vr.positions(v)
        if preview:
            m = np.random.default_rng(n).integers(0, 63, m.shape[0]).astype(np.int32)
            mats = [scenes.material(basecolor=((k + 1) / 64,) * 3) for k in range(63)]
        else:
            mats = [ABSORBING] * 3
        self.mtlids = m
        self.scene = (v, m, mats, [])
        self.preview = preview

    def classify(self):
        return vr.classify(self.camera, self.pos, self.nx, self.ny)

    def shares(self):
        '''the cap that keeps the test honest -> (full_hit, full_miss)'''
        hit, miss = self.classify()
        fh, fm = float(hit.mean()), float(miss.mean())
        print(f'{self.name}: full hit {fh:.3f}, full miss {fm:.3f}, left out {1 - fh - fm:.3f} of {self.nx}x{self.ny}')
        assert not (hit & miss).any()
        if self.n <= 3:
            assert fh + fm >= 0.9, (self.name, fh, fm)
        else:
            assert fh + fm >= 0.40 and fh >= 0.02, (self.name, fh, fm)
        return hit, miss

    def materials(self):
        '''-> (material or -1, contested), with the cap on both asserted'''
        mat, contested = vr.nearest_material(self.camera, self.pos, self.mtlids, self.nx, self.ny)
        known = float((mat >= 0).mean())
        print(f'{self.name}: nearest material known in {known:.3f} of the pixels, {int(contested.sum())} contested')
        assert known >= 0.04 and int(contested.sum()) >= 100, (self.name, known, int(contested.sum()))
        return mat, contested


_cases = {}


def case(name, preview=False):
    if (name, preview) not in _cases:
        _cases[(name, preview)] = Case(name, preview)
    return _cases[(name, preview)]


def mask_errors(c, raw, frames, what):
    '''raw [nx * ny][4] film of `frames` frames of the absorbing scene -> the messages of every classified pixel that is not
    bit for bit (0, 0, 0, F) / (F, F/2, F/4, F); each names the kernel, the pixel, the film value and the covering triangle'''
    hit, miss = c.shares()
    raw = np.asarray(raw, np.float32).reshape(c.nx, c.ny, 4)
    F = np.float32(frames)
    assert np.all(raw[..., 3] == F), f'{what}: {int((raw[..., 3] != F).sum())} pixels without {frames} samples'
    dark = np.array([0, 0, 0, F], np.float32).view(np.uint32)
    lit = np.array([F, F / 2, F / 4, F], np.float32).view(np.uint32)
    bits = np.ascontiguousarray(raw).view(np.uint32)
    cover = vr.covering(c.camera, c.pos, c.nx, c.ny)
    out = []
    for i, j in np.argwhere(hit & (bits != dark).any(axis=-1)):
        out.append(f'{what}: pixel ({i}, {j}) is {raw[i, j].tolist()}, but triangle {int(cover[i, j])} covers it fully: every ray hits')
    for i, j in np.argwhere(miss & (bits != lit).any(axis=-1)):
        out.append(f'{what}: pixel ({i}, {j}) is {raw[i, j].tolist()}, but no triangle is within {vr.MARGIN} px of it: every ray misses')
    return out


def assert_mask(c, raw, frames, what):
    bad = mask_errors(c, raw, frames, what)
    assert not bad, f'{len(bad)} wrong pixels; ' + '; '.join(bad[:4])


def preview_errors(c, raw1, frames, what):
    '''raw pass-1 film of `frames` preview frames of the 63-material scene -> messages of the pixels whose albedo sum is not
    exactly F (k + 1) / 64 where the nearest material k is known, or exactly 0 where every ray misses'''
    _, miss = c.shares()
    mat, contested = c.materials()
    raw1 = np.asarray(raw1, np.float32).reshape(c.nx, c.ny, 4)
    F = np.float32(frames)
    assert np.all(raw1[..., 3] == F), what
    want = np.where(mat >= 0, (mat + 1).astype(np.float32) / np.float32(64) * F, np.float32(0))
    check = (mat >= 0) | miss
    wrong = check & (raw1[..., :3] != want[..., None]).any(axis=-1)
    cover = vr.covering(c.camera, c.pos, c.nx, c.ny)
    return [f'{what}: pixel ({i}, {j}) is {raw1[i, j].tolist()}, want {float(want[i, j])} (material {int(mat[i, j])}, '
            f'covering triangle {int(cover[i, j])}, {"contested" if contested[i, j] else "uncontested"})' for i, j in np.argwhere(wrong)]


def _oracle(oracle_mod, c, scene=None):
    from helpers import setup_oracle
    return setup_oracle(oracle_mod, scene or c.scene, c.nx, c.ny, camera=c.camera, lights=[], world=WORLD)


# ---------------------------------------------------------------- against the oracle
@pytest.mark.parametrize('name', list(CASES))
def test_the_oracles_walk_agrees_in_every_classified_pixel(oracle_mod, name):
    c = case(name)
    c.shares()
    o = _oracle(oracle_mod, c)
    o.render(4)
    assert_mask(c, o.get_film_raw(), 4, f'oracle {name}')


def test_the_deep_case_needs_more_than_32_stack_levels(oracle_mod):
    '''what makes the GPU's `deep` cases mean something: the reference's own walk of that tree holds more than 32 entries'''
    o = _oracle(oracle_mod, case('deep'))
    o.render(4)
    assert o.counters()['max_stack'] > 32, o.counters()


@pytest.mark.parametrize('name', ['n300', 'n1025'])
def test_the_oracles_preview_names_the_nearest_material(oracle_mod, name):
    c = case(name, preview=True)
    c.materials()
    o = _oracle(oracle_mod, c)
    for _ in range(3):
        o.render_preview()
    bad = preview_errors(c, o.get_film_raw(1), 3, f'oracle preview {name}')
    assert not bad, f'{len(bad)} wrong pixels; ' + '; '.join(bad[:4])


# ---------------------------------------------------------------- against per-sample brute force
def _rays(c, px, py):
    '''camera rays through the film points (px, py) in pixel units, from the f64 inverse of the camera matrix'''
    inv = np.linalg.inv(c.camera)
    x, y = px / c.nx * 2 - 1, py / c.ny * 2 - 1
    a = np.stack([x, y, -np.ones_like(x), np.ones_like(x)], axis=1) @ inv.T
    b = np.stack([x, y, np.ones_like(x), np.ones_like(x)], axis=1) @ inv.T
    o, o1 = a[:, :3] / a[:, 3:], b[:, :3] / b[:, 3:]
    return o, o1 - o


def _nearest(pos, o, d):
    '''float64 Moller-Trumbore of one ray over all triangles -> (index of the nearest hit or -1, its t)'''
    e1, e2 = pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    p = np.cross(d, e2)
    det = (e1 * p).sum(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = o - pos[:, 0]
        u = (s * p).sum(axis=1) / det
        q = np.cross(s, e1)
        v = (q * d).sum(axis=1) / det
        t = (q * e2).sum(axis=1) / det
    ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    if not ok.any():
        return -1, np.inf
    k = int(np.argmin(np.where(ok, t, np.inf)))
    return k, float(t[k])


@pytest.mark.parametrize('name', ['n3', 'n300', 'n1025', 'moved', 'flat'])
def test_random_rays_of_classified_pixels_agree_with_moller_trumbore(name):
    preview = name in ('n300', 'n1025')
    c = case(name, preview=preview)
    hit, miss = c.shares()
    mat = c.materials()[0] if preview else None
    rng = np.random.default_rng(5)
    ij = np.argwhere(hit | miss)
    ij = ij[rng.integers(0, ij.shape[0], 2000)]
    uv = rng.random((2000, 2))
    o, d = _rays(c, ij[:, 0] + uv[:, 0], ij[:, 1] + uv[:, 1])
    seen_hit = seen_mat = 0
    for r in range(2000):
        i, j = ij[r]
        k, _ = _nearest(c.pos, o[r], d[r])
        assert (k >= 0) == bool(hit[i, j]), f'{name}: the ray at ({i} + {uv[r, 0]:.3f}, {j} + {uv[r, 1]:.3f}) hits triangle {k}, the pixel is classified {"hit" if hit[i, j] else "miss"}'
        seen_hit += k >= 0
        if mat is not None and mat[i, j] >= 0:
            assert c.mtlids[k] == mat[i, j], f'{name}: nearest triangle {k} of pixel ({i}, {j}) has material {c.mtlids[k]}, the reference says {mat[i, j]}'
            seen_mat += 1
    assert seen_hit > 0 and (mat is None or seen_mat > 0)


# ---------------------------------------------------------------- hand-made cases
# an orthographic-like check needs no perspective: with this matrix clip = (x, y, z, 1), so pixel units are (x + 1) / 2 * n
_PLAIN = np.eye(4)


def test_one_triangle_by_hand():
    '''vertices at pixel coordinates (1, 1), (7, 1), (1, 7) of an 8 x 8 film: the hypotenuse is x + y = 8.  A pixel (i, j) is
    fully inside iff its far corner (i + 1, j + 1) is: i + j + 2 <= 8 - margin * sqrt 2, and i, j >= 1 + margin -> i, j >= 2;
    the legs and the box [1, 7]^2 separate no pixel of the film (i + 1 <= 1 - margin and i >= 7 + margin have no solution in
    0 .. 7); the hypotenuse does iff the near corner (i, j) lies beyond it: i + j >= 8 + margin * sqrt 2 -> i + j >= 9'''
    px = np.array([[[1, 1], [7, 1], [1, 7]]], np.float64)
    pos = np.concatenate([px / 8 * 2 - 1, np.full((1, 3, 1), 0.5)], axis=2)
    hit, miss = vr.classify(_PLAIN, pos, 8, 8)
    i, j = np.meshgrid(np.arange(8), np.arange(8), indexing='ij')
    assert np.array_equal(hit, (i >= 2) & (j >= 2) & (i + j <= 5))
    assert np.array_equal(miss, i + j >= 9)
    assert int(hit.sum()) == 3 and int(miss.sum()) == 21
    assert np.all(vr.covering(_PLAIN, pos, 8, 8)[hit] == 0)
    # the same triangle wound the other way, and moved by a fraction of the margin: the same verdicts
    hit2, miss2 = vr.classify(_PLAIN, pos[:, ::-1] + [0.01 / 4, 0, 0], 8, 8)
    assert np.array_equal(hit, hit2) and np.array_equal(miss, miss2)
    # margin 0 takes touching pixels in and gives none up: pixel (1, 1) has two corners on the legs (exact distances 0)
    hit0, miss0 = vr.classify(_PLAIN, pos, 8, 8, margin=0.0)
    assert hit0[1, 1] and np.all(hit0[hit]) and np.all(miss0[miss]) and not (hit0 & miss0).any()


def test_a_triangle_seen_edge_on_leaves_out_its_bounding_box():
    pos = np.array([[[-0.5, -0.5, 0.2], [0.5, 0.5, 0.4], [0.0, 0.0, 0.9]]])       # collinear in x, y: zero projected area
    hit, miss = vr.classify(_PLAIN, pos, 8, 8)
    i, j = np.meshgrid(np.arange(8), np.arange(8), indexing='ij')
    assert not hit.any()
    assert np.array_equal(~miss, (i >= 1) & (i <= 6) & (j >= 1) & (j <= 6))        # box [2, 6]^2 in pixels, widened by the margin


def test_a_vertex_behind_the_near_plane_raises():
    v, _, _, _ = scenes.scene_random_tris(5, seed=5, edge=0.1)
    pos = vr.positions(v)
    vr.classify(scenes.BENCH_CAMERA, pos, 8, 8)
    pos[3, 1, 2] = 5.4                                                             # the eye is at z = 5.37
    with pytest.raises(ValueError, match='behind the near plane'):
        vr.classify(scenes.BENCH_CAMERA, pos, 8, 8)
    pos[3, 1, 2] = 5.35                                                            # before the eye, behind the near plane (z = 5.3224)
    with pytest.raises(ValueError, match='first: 3'):
        vr.classify(scenes.BENCH_CAMERA, pos, 8, 8)


# ---------------------------------------------------------------- the check can fail
def test_a_dropped_triangle_is_named(oracle_mod):
    c = case('n300')
    hit, _ = c.shares()
    cover = vr.covering(c.camera, c.pos, c.nx, c.ny)
    # a triangle that alone makes some pixel a full hit: no other triangle comes near that pixel
    victim = None
    for t in np.unique(cover[hit]):
        rest = np.delete(c.pos, t, axis=0)
        _, miss_without = vr.classify(c.camera, rest, c.nx, c.ny)
        if (miss_without & (cover == t)).any():
            victim = int(t)
            break
    assert victim is not None
    v, m, mats, im = c.scene
    keep = np.ones(c.n, bool)
    keep[victim] = False
    o = _oracle(oracle_mod, c, (v.reshape(c.n, 3, 8)[keep].reshape(-1, 8), m[keep], mats, im))
    o.render(4)
    bad = mask_errors(c, o.get_film_raw(), 4, 'oracle without one triangle')
    assert len(bad) > 0 and all(f'triangle {victim} covers it' in b for b in bad), bad[:4]


def test_swapped_materials_fail_on_a_contested_pixel(oracle_mod):
    c = case('n300', preview=True)
    mat, contested = c.materials()
    cover = vr.covering(c.camera, c.pos, c.nx, c.ny)
    i, j = np.argwhere(contested)[0]
    a = int(cover[i, j])
    b = int(np.flatnonzero(c.mtlids != c.mtlids[a])[0])
    v, m, mats, im = c.scene
    m = m.copy()
    m[a], m[b] = m[b], m[a]
    o = _oracle(oracle_mod, c, (v, m, mats, im))
    for _ in range(3):
        o.render_preview()
    bad = preview_errors(c, o.get_film_raw(1), 3, 'oracle with two materials swapped')
    assert any(', contested)' in x for x in bad), bad[:4]

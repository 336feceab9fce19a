'''
CPU tests of texture displacement's pure pieces: mpt_displace_corners against the restatement's table,
tests/displace_ref.py itself against cases worked out by hand, the wrap of the sample, and the displacement launch's plan.  No GPU.
'''

import math

import numpy as np
import pytest

import displace_ref as dr
import subdiv_ref as sr

u32 = np.uint32


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u32), b.view(u32))


# ---------------------------------------------------------------- A: the first-corner table
@pytest.mark.parametrize('levels', [1, 2, 3])
def test_first_corner_table_equals_the_restatement(levels):
    from ptina_amd import _lib
    for name in sr.NAMES:
        topo = sr.fixture_topology(name, levels)
        nverts = len(topo['rings'])
        rc, got = _lib.displace_corners(topo['faces'], nverts)
        want = dr.first_corners(topo['faces'], nverts)
        assert rc == 0 and np.array_equal(got, want), (name, levels)
        flat = topo['faces'].reshape(-1)
        assert np.array_equal(flat[want], np.arange(nverts))              # the corner names its vertex ...
        assert all(not (flat[:s] == v).any() for v, s in enumerate(want.tolist()))   # ... and none before it does


def test_first_corner_table_refusals():
    from ptina_amd import _lib
    faces = sr.fixture_topology('tetrahedron', 1)['faces']
    nverts = int(faces.max()) + 1
    assert _lib.displace_corners(faces, nverts)[0] == 0
    bad = faces.copy()
    bad[3, 1] = nverts
    assert _lib.displace_corners(bad, nverts)[0] == 2                     # an id out of range
    bad[3, 1] = -1
    assert _lib.displace_corners(bad, nverts)[0] == 2
    assert _lib.displace_corners(faces, nverts + 1)[0] == 3               # a vertex no face touches
    with pytest.raises(ValueError):
        dr.first_corners(bad, nverts)
    with pytest.raises(ValueError):
        dr.first_corners(faces, nverts + 1)
    assert _lib.displace_corners(np.zeros((0, 3), np.int32), 0)[0] == 0


# ---------------------------------------------------------------- B: the restatement against cases worked out by hand
def _flat_grid():
    return sr.mesh_records(*sr.grid(4, 4, bump=0.0))


@pytest.mark.parametrize('levels', [1, 2])
def test_flat_grid_under_a_constant_image_moves_along_z(levels):
    '''uvs of the grid are dyadic (multiples of 1/16 and their midpoints) and nx - 1 = 4, ny - 1 = 2 are powers of two, so every
    weight of the sample is exact and a constant image gives its constant exactly; the undisplaced normal is (0, 0, 1) exactly'''
    rec = _flat_grid()
    image = np.empty((5, 3, 4), np.float32)
    image[...] = [0.75, 0.25, 0.5, 1.0]
    flat = sr.subdivide(rec, levels)
    assert (flat[:, 2] == 0).all() and _same(flat[:, 3:6], np.tile(np.float32([0, 0, 1]), (flat.shape[0], 1)))
    for channel, h in ((dr.R, 0.75), (dr.G, 0.25), (dr.A, 1.0), (dr.MEAN, ((0.75 + 0.25) + 0.5) / 3.0)):
        got = dr.displace(rec, levels, image, dr.NORMAL, channel, 1.7, 0.4)
        move = np.float32(1.7 * (h - 0.4))
        assert _same(got[:, [0, 1]], flat[:, [0, 1]]) and (got[:, 2] == move).all(), channel
        assert _same(got[:, 3:8], flat[:, 3:8])                           # normals stay (0, 0, 1), texcoords are untouched


def test_one_by_one_image_is_constant_whatever_the_uv():
    image = np.float32([[[0.3, 0.6, 0.9, 0.1]]])
    g = np.random.default_rng(1)
    u, v = g.uniform(-50, 50, 200), g.uniform(-50, 50, 200)
    got = dr.sample(image, u, v)
    assert (got == image[0, 0].astype(np.float64)).all()


def test_two_by_two_ramp_gives_the_linear_height():
    '''texel (x, y) holds x + 10 y in r (and 2 r, 4 r, 8 r): at dyadic uvs the sample is u + 10 v exactly'''
    image = np.zeros((2, 2, 4), np.float32)
    for x in range(2):
        for y in range(2):
            image[x, y] = np.float32(x + 10 * y) * np.float32([1, 2, 4, 8])
    u, v = np.array([0.0, 0.25, 0.5, 0.75, 0.125]), np.array([0.0, 0.5, 0.25, 0.75, 0.875])
    got = dr.sample(image, u, v)
    assert got[:, 0].tolist() == [0.0, 5.25, 3.0, 8.25, 8.875]            # 0.25 + 10 * 0.5, ...
    assert (got[:, 1] == 2 * got[:, 0]).all() and (got[:, 3] == 8 * got[:, 0]).all()
    assert dr.height(got, dr.MEAN).tolist() == [((h + 2 * h) + 4 * h) / 3.0 for h in got[:, 0].tolist()]
    # u = 1 is texel 1 with weight 0 on texel 2, which wraps to texel 0
    assert dr.sample(image, np.array([1.0]), np.array([1.0]))[0, 0] == 11.0


def test_vector_mode_with_rgb_at_midlevel_is_the_identity():
    image = np.empty((4, 3, 4), np.float32)
    image[...] = [0.375, 0.375, 0.375, 0.9]
    for name in ('icosahedron', 'grid'):
        got = dr.displace(sr.fixture(name), 2, image, dr.VECTOR, dr.R, 3.0, 0.375, topo=sr.fixture_topology(name, 2))
        want = sr.fixture_subdivided(name, 2)
        assert ((got.view(u32) == want.view(u32)) | (got == want)).all()  # (p + 3 * 0 is p, but for -0)


# ---------------------------------------------------------------- C: wrap
def test_scaled_uvs_sample_the_texels_of_their_python_modulo_images():
    '''a 4 x 3 image, not square: an x / y swap or an x * nx + y index cannot pass.  The restatement's sample against one written
    with Python integers and the flat index base + x * ny + y'''
    image = dr.random_image(3, 4, 3)
    flatimg = image.reshape(-1, 4).astype(np.float64)
    nx, ny = 4, 3
    rec = dr.scaled_uv(sr.fixture('grid'))
    uv = dr.vertex_uv(rec, sr.fixture_topology('grid', 2), 2)
    got = dr.sample(image, uv[:, 0], uv[:, 1])
    below = above = 0
    for i, (u, v) in enumerate(uv.tolist()):
        px, py = u * 3.0, v * 2.0
        ix, iy = math.floor(px), math.floor(py)
        x0, x1 = px - ix, py - iy
        y0, y1 = 1.0 - x0, 1.0 - x1

        def at(x, y):
            return flatimg[(x % nx) * ny + (y % ny)]
        want = (((at(ix + 1, iy + 1) * x0) * x1 + (at(ix + 1, iy) * x0) * y1) + (at(ix, iy) * y0) * y1) + (at(ix, iy + 1) * y0) * x1
        assert (got[i] == want).all(), (i, u, v)
        below += ix < 0 or iy < 0
        above += ix + 1 >= nx or iy + 1 >= ny
    assert below > 10 and above > 10, 'the scaled uvs do not leave the image on both sides'


# ---------------------------------------------------------------- D: the plan of the displacement launch
def test_displacement_launch_plan():
    '''the launch runs over the displaced copies among the dirty ones, V_L items each, 256 per block: copies without a displacement
    have no items'''
    from ptina_amd import _lib
    nv = [len(sr.fixture_topology(n, L)['rings']) for n, L in (('grid', 3), ('tetrahedron', 1), ('cylinder', 2), ('fan12', 3), ('pair', 1))]
    assert nv[0] == 1681 and nv[1] < sr.CHUNK
    for displaced, dirty in (([1, 1, 0, 1, 0], None), ([1, 0, 1, 1, 1], [0, 1, 1, 1, 0]), ([0, 0, 0, 0, 0], None), ([1, 1, 1, 1, 1], [1, 1, 1, 1, 1])):
        items = [n if d else 0 for n, d in zip(nv, displaced)]
        assert _lib.subdiv_plan(items, dirty) == sr.plan(items, dirty)
    runs, blocks = _lib.subdiv_plan([nv[0], 0, nv[1]])
    assert runs == [(0, 0), (2, 7)] and blocks == 8                       # 1681 = 6 * 256 + 145

'''
GPU (-m gpu): the HIP device functions that READ SCENE STATE held directly to vectors computed by the reference's own
function bodies (tests/golden/reference_scene_units.npz, made by tests/golden/make_reference_scene_units_golden.py) --
lights_hit, lights_sample / light_sample_one, image_sample, world_at, material_get (strict and production, the latter
through material_from), camera_generate and the normal flip of get_geometries (production: get_geometries_rec).

mpt_unit_eval's scene kinds (include/miptina.h) run them as the render kernels inline them, in the build the context's
mode selects, on the context's own scene.  The fixture's scene state is uploaded through the public classes (LightPool.add,
ImagePool.load, MaterialPool.load, WorldLight.set, Camera.set_perspective), so their packing is under test too.  All three
light states run: five lights, one light (the only way into the production build's scalar-load path of lights_sample) and none.

Bounds, masks and the checks are in tests/scene_units.py, shared with the CPU file that holds the C oracle to the same
vectors: the strict build gets the f32 oracle's bounds, the production build relative 1e-5 plus the reference's own
f32-vs-f64 spread, with the exceptions stated there.  Discrete outputs must be the reference's exactly.  Every check
prints and reports its worst error against its bound.

The production LDS kernels read material records from their LDS copy and unpack them through material_from as well; the
copy itself stays covered by test_lds_and_gather_kernels_agree_bit_for_bit (tests/test_parity_gpu.py).
'''

import numpy as np
import pytest

import scene_units as SU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return SU.load()


class HipEval:
    def __init__(self, c):
        self.c = c

    def __getattr__(self, name):
        return lambda rows: self.c.unit_eval(name, rows)


def upload(gold, state='five', world='env', camera=0):
    from ptina_amd.things import ImagePool, MaterialPool, LightPool, WorldLight, Camera
    ImagePool().load(SU.images_of(gold))
    MaterialPool().load(SU.materials_of(gold))
    LightPool().clear()
    for l in SU.lights_of(gold, state):
        LightPool().add(*l)
    WorldLight().set(*SU.worlds_of(gold)[world])
    Camera().set_perspective(gold['state/camera_pers'][camera])


@pytest.fixture(params=['strict', 'fast'])
def dev(request, fresh):
    from ptina_amd import _lib
    from ptina_amd.things import init_things
    from ptina_amd.common import ctx
    init_things()
    ctx().set_option('mode', _lib.MODE_STRICT if request.param == 'strict' else _lib.MODE_FAST)
    return request.param, HipEval(ctx())


@pytest.mark.parametrize('state', ['five', 'one', 'none'])
def test_lights_hit(gold, dev, state):
    mode, ev = dev
    upload(gold, state=state)
    SU.check_light_hit(ev, gold, mode, state)


@pytest.mark.parametrize('state', ['five', 'one', 'none'])
def test_lights_sample(gold, dev, state):
    mode, ev = dev
    upload(gold, state=state)
    SU.check_light_sample(ev, gold, mode, state)


def test_image_sample(gold, dev):
    mode, ev = dev
    upload(gold)
    SU.check_image_sample(ev, gold, mode)


@pytest.mark.parametrize('state', ['plain', 'env'])
def test_world_at(gold, dev, state):
    mode, ev = dev
    upload(gold, world=state)
    SU.check_world_at(ev, gold, mode, state)


def test_material_get(gold, dev):
    mode, ev = dev
    upload(gold)
    SU.check_material_get(ev, gold, mode)


@pytest.mark.parametrize('camera', [0, 1])
def test_camera_generate(gold, dev, camera):
    mode, ev = dev
    upload(gold, camera=camera)
    from ptina_amd.things import Camera
    assert np.allclose(Camera().V2W, gold['state/camera_v2w'][camera], rtol=1e-6, atol=1e-9)      # the inverse the reference's setter stored
    SU.check_camera_generate(ev, gold, mode, camera)


def test_face_side(gold, dev):
    mode, ev = dev
    SU.check_face_side(ev, gold, mode)           # no scene loaded: the shading records come with the rows, the material is the default one

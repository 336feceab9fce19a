'''
GPU tests of the SHADE stage specialised by scene features (ptina_amd/csrc/shade_feat.h; render_kernel_lds4<COUNT, FEAT>).

A scene without textured materials, clearcoat, transmission, an environment map or more than one light runs the plain
instantiation of the LDS-resident kernel; any other scene runs the generic one (option shade_spec = 0 forces it).  The plain
instantiation holds the same operations minus regions no lane of such a scene enters (today the texture, environment-map and
light-list regions; the two lobes stay compiled in, shade_feat.h says why), so its film is the generic one's BIT FOR BIT; a scene with any feature must report the generic instantiation and keep the parity with the oracle the existing tests define
(helpers.FAST).  Options: shade_spec (0 / 1), scene_feat (read-only: the scene's mask), shade_inst (read-only: the mask the last
launch was compiled for: 0 plain, 31 generic), last_kernel (5: the LDS-resident 4-wide kernel).
'''

import numpy as np
import pytest

from ptina_amd import scenes

pytestmark = pytest.mark.gpu

TEXTURED, CLEARCOAT, TRANSMISSION, WORLD_TEXTURE, MANY_LIGHTS = 1, 2, 4, 8, 16
PLAIN, GENERIC = 0, 31


def raw_film(eng, spp, spec):
    '''the raw film (uint32 view) of `spp` frames from the start of the Sobol sequence with option shade_spec = spec, and the
    instantiation / kernel the launch reported'''
    from ptina_amd.common import ctx
    from ptina_amd.things import FilmTable
    from ptina_amd.sampling.sobol import SobolSampler
    c = ctx()
    c.set_option('shade_spec', spec)
    assert c.get_option('shade_spec') == spec
    SobolSampler().reset()
    FilmTable().clear()
    eng.render(spp)
    film = FilmTable().get_raw().view(np.uint32).copy()
    return film, c.get_option('shade_inst'), c.get_option('last_kernel')


def assert_same_bits(a, b, what):
    bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
    assert bad.size == 0, '%s: %d of %d film elements differ, first %d: %s vs %s' % (
        what, bad.size, a.shape[0], bad[0], a[bad[0]].view(np.float32), b[bad[0]].view(np.float32))


def plain_vs_generic(scene, nx, ny, spp, what, lights=None, world=None, batch=None):
    from helpers import setup_engine
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import LightPool
    reset_all()
    eng = setup_engine(scene, nx, ny, mode='fast', lights=lights, world=world)
    c = ctx()
    if batch:
        c.set_option('batch', batch)
    assert LightPool().count == 1, what + ': the light list of a plain scene holds one light'
    assert c.get_option('shade_spec') == 1, 'shade_spec defaults to 1'
    assert c.get_option('scene_feat') == PLAIN, what
    spec, inst1, k1 = raw_film(eng, spp, 1)
    gen, inst0, k0 = raw_film(eng, spp, 0)
    assert k1 == 5 and k0 == 5, what + ': not the LDS-resident 4-wide kernel'
    assert inst1 == PLAIN, what + ' must report the plain instantiation'
    assert inst0 == GENERIC, what + ': shade_spec = 0 must force the generic instantiation'
    assert spec[:, 3].view(np.float32).min() == spp
    print('%s: %d film elements, mean %.6f' % (what, spec.shape[0], float(spec[:, :3].view(np.float32).mean())))
    assert_same_bits(spec, gen, what)
    # and again with the plain one: the selection is per launch, not sticky
    again, inst, _ = raw_film(eng, spp, 1)
    assert inst == PLAIN
    assert_same_bits(again, spec, what + ' (second plain run)')
    reset_all()


@pytest.mark.parametrize('name,n,spp', [('s978', 128, 16), ('s34', 128, 16), ('s978', 512, 32)])
def test_plain_scenes_render_the_generic_film_bit_for_bit(fresh, name, n, spp):
    '''s978 (the headline scene; also at the benchmark's film and sample count) and s34: their materials set basecolor,
    roughness, metallic and specular only, the default light list holds one light, the world light is a constant'''
    plain_vs_generic(scenes.get_scene(name), n, n, spp, '%s %dx%d %d spp' % (name, n, n, spp))


@pytest.mark.parametrize('seed', [1, 2, 3, 5, 8, 13])
def test_random_plain_scenes_render_the_generic_film_bit_for_bit(fresh, seed):
    '''the seeded random scenes of the stress tests (helpers.stress_scene: the cornell walls, 1 .. 900 random triangles with smooth
    normals, 2 .. 5 random opaque Disney materials using every parameter but clearcoat and transmission, a random constant world
    light) with the first of their lights only, at their own small film, sample count and batch size'''
    from helpers import stress_scene
    scene, lights, world, nx, ny, spp, batches = stress_scene(seed)
    plain_vs_generic(scene, nx, ny, spp, 'random plain scene %d (%d triangles, %dx%d, %d spp)' % (seed, scene[1].shape[0], nx, ny, spp),
                     lights=lights[:1], world=world, batch=int(batches[0]))


def _two_box_scene(material, lift=0.01):
    '''the 34-triangle scene with both boxes of `material`, raised off the floor (test_parity_gpu.py: standing on it their bottom
    faces coincide with the floor quad and the reference's own choice between the two hangs on a last bit)'''
    parts = [scenes.cornell_walls(), scenes.box((-0.7, 1.2 + lift, -0.6), (0.6, 1.2, 0.6), 18.0, 3),
             scenes.box((0.75, 0.6 + lift, 0.55), (0.6, 0.6, 0.6), -17.0, 4)]
    v, m = scenes._compose(parts)
    return v, m, list(scenes.WALL_MATERIALS) + [scenes.material(**material), scenes.material(**material)], []


def _feature_cases():
    from ptina_amd.tools.matrix import translate
    checker = np.ones((8, 8, 3), np.float32)
    checker[::2, 1::2] = 0.2
    checker[1::2, ::2] = 0.2
    v, m, mats, _ = scenes.scene_s978()
    tex_mats = [list(x) for x in mats]
    tex_mats[3][0] = ([1.0, 0.9, 0.8], 0)                                   # basecolor textured by image 0
    rot = np.eye(4)
    rot[:3, :3] = [[1, 0, 0], [0, 0, 1], [0, -1, 0]]                        # area light facing down
    two_lights = [(translate([0, 3.9, 0]) @ rot, np.array([18.0, 16.0, 12.0]), 0.6, 'AREA'),
                  (translate([-1.2, 3.0, 1.0]), np.array([6.0, 6.0, 9.0]), 0.2, 'POINT')]
    s978 = scenes.scene_s978()
    return {
        'textured': (TEXTURED, (v, m, tex_mats, [checker]), None, None),
        'clearcoat': (CLEARCOAT, _two_box_scene(dict(basecolor=(0.7, 0.1, 0.1), roughness=0.5, clearcoat=1.0, clearcoatGloss=0.9)), None, None),
        'glass': (TRANSMISSION, _two_box_scene(dict(basecolor=(0.9, 0.95, 1.0), roughness=0.08, transmission=0.9, ior=1.5, specular=0.5)), None, None),
        'environment': (WORLD_TEXTURE, (s978[0], s978[1], s978[2], [scenes.env_image(64, 32)]), None, ([1.0, 1.0, 1.0, 1.0], 0)),
        'two_lights': (MANY_LIGHTS, scenes.scene_s34(), two_lights, None),
    }


@pytest.mark.parametrize('name', ['textured', 'clearcoat', 'glass', 'environment', 'two_lights'])
def test_a_scene_with_one_feature_takes_the_generic_instantiation(fresh, oracle_mod, name):
    '''one scene per feature bit: the mask names the bit, the launch reports the generic instantiation with shade_spec at its
    default, the film is the one shade_spec = 0 gives bit for bit, and it keeps the parity with the oracle the existing parity tests
    define (64 x 64, 16 spp, helpers.FAST)'''
    from helpers import setup_engine, setup_oracle, assert_parity, bounds
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import FilmTable
    bit, scene, lights, world = _feature_cases()[name]
    ref = setup_oracle(oracle_mod, scene, 64, 64, lights=lights, world=world)
    ref.render(16)
    reset_all()
    eng = setup_engine(scene, 64, 64, mode='fast', lights=lights, world=world)
    assert ctx().get_option('scene_feat') == bit, name
    spec, inst1, k1 = raw_film(eng, 16, 1)
    img = FilmTable().get_image()
    gen, inst0, k0 = raw_film(eng, 16, 0)
    assert k1 == 5 and k0 == 5, name + ': not the LDS-resident 4-wide kernel'
    assert inst1 == GENERIC and inst0 == GENERIC, name + ' must report the generic instantiation'
    assert_same_bits(spec, gen, name)
    assert_parity(img, ref.get_image(), *bounds('fast'), what='shade_spec %s fast' % name)
    reset_all()


def test_reloading_materials_flips_the_selection_both_ways(fresh):
    '''a live context: plain materials -> glass on one box -> plain again.  The mask follows every upload, the launch after it takes
    the other instantiation, and the film after the way back is the first one bit for bit; so do the light list and the world'''
    from helpers import setup_engine
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import MaterialPool, LightPool, WorldLight, ImagePool
    from ptina_amd.tools.matrix import translate
    v, m, mats, _ = scenes.scene_s34()
    eng = setup_engine((v, m, mats, []), 64, 64, mode='fast')
    c = ctx()
    assert c.get_option('shade_inst') == -1, 'nothing launched yet'
    first, inst, k = raw_film(eng, 8, 1)
    assert (c.get_option('scene_feat'), inst, k) == (PLAIN, PLAIN, 5)
    glass = list(mats)
    glass[4] = scenes.material(basecolor=(0.9, 0.95, 1.0), roughness=0.08, transmission=0.9, ior=1.5, specular=0.5)
    MaterialPool().load(glass)
    assert c.get_option('scene_feat') == TRANSMISSION
    with_glass, inst, k = raw_film(eng, 8, 1)
    assert (inst, k) == (GENERIC, 5)
    assert (with_glass != first).any(), 'the glass box changed nothing'
    MaterialPool().load(list(mats))
    assert c.get_option('scene_feat') == PLAIN
    back, inst, k = raw_film(eng, 8, 1)
    assert (inst, k) == (PLAIN, 5)
    assert_same_bits(back, first, 'plain -> glass -> plain')
    # a second light and back
    idx = LightPool().add(translate([-1.2, 3.0, 1.0]), np.array([6.0, 6.0, 9.0]), 0.2, 'POINT')
    assert idx == 1 and c.get_option('scene_feat') == MANY_LIGHTS
    assert raw_film(eng, 8, 1)[1] == GENERIC
    LightPool().clear()
    assert c.get_option('scene_feat') == MANY_LIGHTS                        # no light at all is not the one-light scene either
    assert raw_film(eng, 8, 1)[1] == GENERIC
    # an environment map and back
    ImagePool().load([scenes.env_image(32, 16)])
    WorldLight().set([1.0, 1.0, 1.0, 1.0], 0)
    assert c.get_option('scene_feat') == MANY_LIGHTS | WORLD_TEXTURE
    WorldLight().set([0.1, 0.1, 0.1, 1.0], -1)
    assert c.get_option('scene_feat') == MANY_LIGHTS
    reset_all()


def test_shade_spec_option_is_checked(fresh):
    from ptina_amd.things import init_things
    from ptina_amd.common import ctx
    init_things()
    c = ctx()
    for bad in (-1, 2):
        with pytest.raises(RuntimeError, match='shade_spec'):
            c.set_option('shade_spec', bad)
    assert c.get_option('shade_spec') == 1

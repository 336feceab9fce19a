'''
GPU tests of the lean variant of the plain SHADE instantiation (ptina_amd/csrc/shade_feat.h shade_lean_*; render_kernel_lds4<COUNT,
MPT_FEAT_PLAIN, LEAN>; pt_device.h disney_brdf / disney_bounce).

A plain scene -- untextured materials without clearcoat or transmission, one light, no environment map -- whose materials, the
default one included, all have sheen and subsurface exactly zero runs a kernel compiled without the two terms those parameters
multiply.  Its film must be the generic kernel's BIT FOR BIT (raw films compared as uint32, option shade_spec = 1 against 0); a plain
scene with sheen or subsurface keeps the plain kernel without the variant, and a scene with any feature the generic one.  Which
variant a launch took is read through mpt_get_shade_variant (Context.shade_variant()): (feature mask, lean).

The quilts (helpers.quilt_scene: 300 triangles in general position, every one in one of 61 materials drawn over a class of the
parameter cube, parameters at exactly 0 and 1 and -0.0 among them) put the claims tests/test_reference_disney_cube_gpu.py checks
function by function through the render kernel's own contraction context, at 64 x 64 x 8: the lean quilt must take (PLAIN, 1) and
the plain quilt (PLAIN, 0), each rendering the generic film bit for bit; the quilt over the full cube -- clearcoat, transmission,
roughness down to 0 -- holds the strict build to the oracle at helpers.STRICT and every production kernel to the strict film through
the accounting of helpers.compare_kernels (helpers.FAST, at most ceil(0.0005 x pixels) single-sample fireflies, each explained).
'''

import numpy as np
import pytest

from ptina_amd import scenes

pytestmark = pytest.mark.gpu

PLAIN, GENERIC, TRANSMISSION = 0, 31, 4


def seam_materials():
    '''five materials for the 34-triangle scene (three walls, two boxes) that walk through the opaque lobes the variant keeps: a
    pale wall with a specular tint, a rough dielectric with a full tint, a tinted dielectric at roughness 0 (alpha clamps to 0.001),
    a half-metal and a near-mirror metal on the boxes -- sheen and subsurface exactly 0 in all of them (sheenTint set: it must not
    matter)'''
    m = scenes.material
    return [m(basecolor=(0.8, 0.8, 0.8), metallic=0.1, roughness=0.3, specular=0.2, specularTint=0.8, sheenTint=0.7),
            m(basecolor=(0.5, 0.1, 0.4), metallic=0.0, roughness=0.95, specular=1.0, specularTint=1.0),
            m(basecolor=(0.2, 0.8, 0.3), metallic=0.25, roughness=0.0, specular=0.9, specularTint=0.5, sheenTint=0.1),
            m(**FIRST_BOX),
            m(basecolor=(0.9, 0.6, 0.2), metallic=1.0, roughness=0.03, specular=0.5, specularTint=0.0)]


FIRST_BOX = dict(basecolor=(0.7, 0.7, 0.75), metallic=0.6, roughness=0.6, specular=0.7, specularTint=0.3)


def seam_scene(**change_first_box):
    '''the 34-triangle scene in the seam materials; keywords change parameters of the first (tall) box's material'''
    v, m, mats, imgs = scenes.scene_s34()
    new = seam_materials()
    assert len(new) == len(mats) and int(m.max()) == len(new) - 1
    if change_first_box:
        new[3] = scenes.material(**dict(FIRST_BOX, **change_first_box))
    return v, m, new, imgs


def raw_film(eng, spp, spec):
    '''the raw film (uint32 view) of `spp` frames from the start of the Sobol sequence with option shade_spec = spec, and what the
    launch reported: (feature mask, lean) and the kernel'''
    from ptina_amd.common import ctx
    from ptina_amd.things import FilmTable
    from ptina_amd.sampling.sobol import SobolSampler
    c = ctx()
    c.set_option('shade_spec', spec)
    SobolSampler().reset()
    FilmTable().clear()
    eng.render(spp)
    film = FilmTable().get_raw().view(np.uint32).copy()
    feat, lean = c.shade_variant()
    assert feat == c.get_option('shade_inst'), 'the query and option shade_inst name the same launch'
    return film, (feat, lean), c.get_option('last_kernel')


def differing(a, b):
    return np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))


def special_vs_generic(scene, nx, ny, spp, what, want_variant, scene_feat=PLAIN, lights=None, world=None):
    '''renders `scene` with shade_spec = 1, then 0: the first launch reports `want_variant`, the second the generic kernel, and no
    film element differs'''
    from helpers import setup_engine
    from ptina_amd.common import ctx, reset_all
    reset_all()
    eng = setup_engine(scene, nx, ny, mode='fast', lights=lights, world=world)
    c = ctx()
    assert c.shade_variant() == (-1, -1), 'nothing launched yet'
    assert c.get_option('scene_feat') == scene_feat, what
    spec, variant1, k1 = raw_film(eng, spp, 1)
    gen, variant0, k0 = raw_film(eng, spp, 0)
    assert k1 == 5 and k0 == 5, what + ': not the LDS-resident 4-wide kernel'
    assert variant1 == want_variant, what
    assert variant0 == (GENERIC, 0), what + ': shade_spec = 0 must force the generic instantiation, which has no lean variant'
    assert spec[:, 3].view(np.float32).min() == spp
    bad = differing(spec, gen)
    print('%s: %d film elements, mean %.6f, %d differ' % (what, spec.shape[0], float(spec[:, :3].view(np.float32).mean()), bad.size))
    assert bad.size == 0, '%s: %d of %d film elements differ, first %d: %s vs %s' % (
        what, bad.size, spec.shape[0], bad[0], spec[bad[0]].view(np.float32), gen[bad[0]].view(np.float32))
    reset_all()
    return spec


@pytest.mark.parametrize('name', ['s978', 's34'])
def test_benchmark_scenes_take_the_lean_variant_and_render_the_generic_film(fresh, name):
    '''128 x 128 x 16: the shape at which the seams of the clearcoat and transmission regions showed on s978'''
    special_vs_generic(scenes.get_scene(name), 128, 128, 16, '%s 128x128 16 spp' % name, (PLAIN, 1))


@pytest.fixture(scope='module')
def seam_film():
    '''the seam scene's film, rendered once: the lean variant's, checked against the generic kernel's'''
    return special_vs_generic(seam_scene(), 128, 128, 16, 'seam scene 128x128 16 spp', (PLAIN, 1))


def test_seam_scene_takes_the_lean_variant_and_renders_the_generic_film(fresh, seam_film):
    assert seam_film.shape == (128 * 128, 4)


def test_sheen_in_one_material_keeps_the_plain_kernel_without_the_variant(fresh, seam_film):
    sheen = special_vs_generic(seam_scene(sheen=0.2), 128, 128, 16, 'seam scene, sheen 0.2 on one box', (PLAIN, 0))
    assert differing(seam_film, sheen).size > 0, 'the sheen changed nothing: the box is not seen'


def test_subsurface_in_one_material_keeps_the_plain_kernel_without_the_variant(fresh):
    special_vs_generic(seam_scene(metallic=0.0, roughness=0.5, subsurface=0.6), 64, 64, 16, 'seam scene, subsurface 0.6 on one box', (PLAIN, 0))


def test_transmission_in_one_material_takes_the_generic_kernel(fresh):
    special_vs_generic(seam_scene(metallic=0.0, roughness=0.08, transmission=0.9, ior=1.5), 64, 64, 16,
                       'seam scene, one glass box', (GENERIC, 0), scene_feat=TRANSMISSION)


def test_reloading_materials_moves_the_selection_both_ways(fresh):
    '''a live context: lean materials -> sheen on one box -> lean again; the choice follows every upload and the film after the way
    back is the first one bit for bit'''
    from helpers import setup_engine
    from ptina_amd.common import reset_all
    from ptina_amd.things import MaterialPool
    v, m, mats, imgs = seam_scene()
    eng = setup_engine((v, m, mats, imgs), 64, 64, mode='fast')
    first, variant, k = raw_film(eng, 8, 1)
    assert (variant, k) == ((PLAIN, 1), 5)
    MaterialPool().load(seam_scene(sheen=0.5, sheenTint=0.2)[2])
    with_sheen, variant, k = raw_film(eng, 8, 1)
    assert (variant, k) == ((PLAIN, 0), 5)
    assert differing(with_sheen, first).size > 0, 'the sheen changed nothing'
    MaterialPool().load(list(mats))
    back, variant, k = raw_film(eng, 8, 1)
    assert (variant, k) == ((PLAIN, 1), 5)
    assert differing(back, first).size == 0, 'lean -> sheen -> lean'
    reset_all()


def quilt(kind):
    from helpers import quilt_scene, QUILT_MATERIALS
    scene, lights, world = quilt_scene(kind)
    used = np.unique(scene[1])
    assert QUILT_MATERIALS >= 32 and len(scene[2]) == 3 + QUILT_MATERIALS and used.size == len(scene[2]), 'every material is on a face'
    return scene, lights, world


def test_lean_quilt_takes_the_lean_variant_and_renders_the_generic_film(fresh):
    scene, lights, world = quilt('lean')
    sheen = np.array([m[6][0] for m in scene[2]]), np.array([m[5][0] for m in scene[2]])
    assert all((x == 0).all() for x in sheen) and (np.signbit(sheen[0]) | np.signbit(sheen[1])).sum() >= 8, '-0.0 among the lean materials'
    special_vs_generic(scene, 64, 64, 8, 'lean quilt 64x64 8 spp', (PLAIN, 1), lights=lights, world=world)


def test_plain_quilt_keeps_the_plain_kernel_and_renders_the_generic_film(fresh):
    scene, lights, world = quilt('plain')
    sheen, subs = np.array([m[6][0] for m in scene[2]]), np.array([m[5][0] for m in scene[2]])
    assert (sheen == 1).any() and (subs == 1).any() and (sheen[3:] == 0).any() and ((sheen > 0) & (sheen < 1)).sum() >= 8
    special_vs_generic(scene, 64, 64, 8, 'plain quilt 64x64 8 spp', (PLAIN, 0), lights=lights, world=world)


def test_full_cube_quilt_strict_against_the_oracle_and_production_against_strict(fresh, oracle_mod):
    from helpers import STRICT, assert_parity, compare_kernels, setup_oracle
    scene, lights, world = quilt('cube')
    cc, tr, rough = (np.array([m[k][0] for m in scene[2][3:]]) for k in (8, 10, 2))
    assert (cc > 0).sum() >= 8 and (tr > 0).sum() >= 8 and (rough == 0).any() and (tr == 1).any() and (cc == 1).any()
    nx, ny, spp = 64, 64, 8
    films = {}
    ok, flies, msgs = compare_kernels(scene, lights, world, nx, ny, spp, [8, 8, 3, 8, 5], 'full-cube quilt', films=films)
    assert ok, msgs
    ref = setup_oracle(oracle_mod, scene, nx, ny, lights=lights, world=world)
    ref.render(spp)
    assert_parity(films['strict'], ref.get_image(), *STRICT, what='full-cube quilt %dx%dx%d, strict build against the oracle' % (nx, ny, spp))

'''
The plain instantiation of the LDS-resident kernel is compiled without the clearcoat and transmission lobes (FEAT = 0,
ptina_amd/csrc/shade_feat.h) and must still render the generic kernel's film BIT FOR BIT.  What stood in the way were two places where
-ffp-contract=fast fused a multiply-add differently once a lobe was gone (pt_device.h: GTR2's alpha^2 - 1, and the a + b of
smithGGX as Disney.brdf calls it); both are written out now.  The scenes here walk through them: materials with non-zero
metallic, subsurface, sheen, specularTint and low and high roughness, clearcoat and transmission exactly 0 -- plain against option
shade_spec = 0 (the generic instantiation), raw films compared as uint32.

The CPU test checks with the host's own header that every scene used has the empty feature mask and that the random ones cover
the parameters: with any other mask both runs would launch the generic kernel and the comparison would be vacuous.
'''

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from ptina_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ptina_amd', 'csrc')
SEEDS = list(range(101, 121))                                               # twenty seeded random plain scenes
PLAIN, GENERIC = 0, 31
METALLIC, ROUGHNESS, SPECTINT, SUBSURFACE, SHEEN, CLEARCOAT_K, TRANSMISSION_K = 1, 2, 4, 5, 6, 8, 10   # scenes.PARAM_NAMES

SHIM = '''
#include "shade_feat.h"
int t_material(const float *fac, const int32_t *tex) { return shade_feat_material(fac, tex); }
int t_scene(const unsigned char *bits, int nmats, int max_mtlid, int default_bits, int nlights, int world_tex) {
    return shade_feat_scene(bits, nmats, max_mtlid, default_bits, nlights, world_tex);
}
'''


def seam_scene():
    '''the 34-triangle scene with its boxes and walls in materials that use every parameter of the opaque lobes: a near-mirror and
    a rough metal, a subsurface / sheen cloth, a tinted dielectric at roughness 0 (alpha clamps to 0.001), a pale sheen wall'''
    v, m, mats, imgs = scenes.scene_s34()
    new = [scenes.material(basecolor=(0.8, 0.8, 0.8), metallic=0.1, roughness=0.3, specular=0.2, specularTint=0.8, sheen=0.2),
           scenes.material(basecolor=(0.5, 0.1, 0.4), metallic=0.0, roughness=0.6, subsurface=0.8, sheen=1.0, sheenTint=0.7),
           scenes.material(basecolor=(0.2, 0.8, 0.3), metallic=0.25, roughness=0.0, specular=0.9, specularTint=0.5, subsurface=0.3,
                           sheen=0.4, sheenTint=0.1),
           scenes.material(basecolor=(0.9, 0.6, 0.2), metallic=1.0, roughness=0.03, specular=0.5, specularTint=0.0),
           scenes.material(basecolor=(0.7, 0.7, 0.75), metallic=0.6, roughness=0.95, specular=1.0, specularTint=1.0)]
    assert len(mats) == len(new)
    return v, m, new, imgs


def all_scenes():
    '''(name, materials, highest material id, lights) of every scene the GPU tests below render'''
    from helpers import stress_scene
    for name, sc in (('seam', seam_scene()), ('s978', scenes.get_scene('s978'))):
        yield name, list(sc[2]), int(sc[1].max()), 1
    for seed in SEEDS:
        scene, lights, world, nx, ny, spp, batches = stress_scene(seed)
        assert world[1] == -1, 'a constant world light'
        yield 'random %d' % seed, list(scene[2]), int(scene[1].max()), len(lights[:1])


def test_the_chosen_scenes_are_plain_and_cover_the_opaque_parameters(tmp_path):
    src, so = str(tmp_path / 'shim.c'), str(tmp_path / 'shim.so')
    with open(src, 'w') as f:
        f.write(SHIM)
    cc = os.environ.get('CC') or shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or '/opt/rocm/lib/llvm/bin/clang'
    subprocess.run([cc, '-std=c99', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so], check=True)
    lib = C.CDLL(so)
    lib.t_material.argtypes = [C.c_void_p, C.c_void_p]
    lib.t_scene.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]

    def bits_of(mat):
        fac = np.zeros((12, 4), np.float32)
        tex = np.zeros(12, np.int32)
        for k, (val, t) in enumerate(mat):
            fac[k, :np.size(val)] = np.ravel(val)
            tex[k] = t
        return lib.t_material(fac.ctypes.data, tex.ctypes.data)

    default_bits = bits_of(scenes.material())
    seen = {k: [] for k in (METALLIC, ROUGHNESS, SPECTINT, SUBSURFACE, SHEEN)}
    for name, mats, max_id, nlights in all_scenes():
        bits = np.array([bits_of(m) for m in mats], np.uint8)
        assert lib.t_scene(bits.ctypes.data, len(mats), max_id, default_bits, nlights, -1) == PLAIN, name
        for m in mats[:max_id + 1]:
            assert m[CLEARCOAT_K][0] == 0.0 and m[TRANSMISSION_K][0] == 0.0, name
            if name.startswith('random'):
                for k in seen:
                    seen[k].append(float(m[k][0]))
    for k in (METALLIC, SPECTINT, SUBSURFACE, SHEEN):
        assert sum(x > 0.05 for x in seen[k]) >= 10, 'parameter %s hardly used by the random scenes' % scenes.PARAM_NAMES[k]
    assert min(seen[ROUGHNESS]) < 0.15 and max(seen[ROUGHNESS]) > 0.9, 'low and high roughness'


def raw_film(eng, spp, spec):
    '''the raw film (uint32 view) of `spp` frames from the start of the Sobol sequence with option shade_spec = spec, and the
    instantiation / kernel the launch reported'''
    from ptina_amd.common import ctx
    from ptina_amd.things import FilmTable
    from ptina_amd.sampling.sobol import SobolSampler
    c = ctx()
    c.set_option('shade_spec', spec)
    SobolSampler().reset()
    FilmTable().clear()
    eng.render(spp)
    film = FilmTable().get_raw().view(np.uint32).copy()
    return film, c.get_option('shade_inst'), c.get_option('last_kernel')


def plain_vs_generic(scene, nx, ny, spp, what, lights=None, world=None, batch=None):
    from helpers import setup_engine
    from ptina_amd.common import ctx, reset_all
    reset_all()
    eng = setup_engine(scene, nx, ny, mode='fast', lights=lights, world=world)
    c = ctx()
    if batch:
        c.set_option('batch', batch)
    assert c.get_option('scene_feat') == PLAIN, what
    spec, inst1, k1 = raw_film(eng, spp, 1)
    gen, inst0, k0 = raw_film(eng, spp, 0)
    assert k1 == 5 and k0 == 5, what + ': not the LDS-resident 4-wide kernel'
    assert inst1 == PLAIN and inst0 == GENERIC, what + ': plain, then the generic instantiation forced by shade_spec = 0'
    assert spec[:, 3].view(np.float32).min() == spp
    bad = np.flatnonzero((spec != gen).reshape(spec.shape[0], -1).any(axis=1))
    print('%s: %d film elements, mean %.6f, %d differ' % (what, spec.shape[0], float(spec[:, :3].view(np.float32).mean()), bad.size))
    assert bad.size == 0, '%s: %d of %d film elements differ, first %d: %s vs %s' % (
        what, bad.size, spec.shape[0], bad[0], spec[bad[0]].view(np.float32), gen[bad[0]].view(np.float32))
    reset_all()


@pytest.mark.gpu
def test_seam_scene_renders_the_generic_film_bit_for_bit(fresh):
    plain_vs_generic(seam_scene(), 128, 128, 16, 'seam scene 128x128 16 spp')


@pytest.mark.gpu
@pytest.mark.parametrize('n,spp', [(128, 16), (512, 32)])
def test_s978_renders_the_generic_film_bit_for_bit(fresh, n, spp):
    '''128 x 128 x 16 is the configuration that showed 181 differing film elements before the seams were pinned; 512 x 512 x 32 is
    the benchmark's'''
    plain_vs_generic(scenes.get_scene('s978'), n, n, spp, 's978 %dx%d %d spp' % (n, n, spp))


@pytest.mark.gpu
@pytest.mark.parametrize('seed', SEEDS)
def test_twenty_random_plain_scenes_render_the_generic_film_bit_for_bit(fresh, seed):
    from helpers import stress_scene
    scene, lights, world, nx, ny, spp, batches = stress_scene(seed)
    plain_vs_generic(scene, nx, ny, spp, 'random plain scene %d (%d triangles, %dx%d, %d spp)' % (seed, scene[1].shape[0], nx, ny, spp),
                     lights=lights[:1], world=world, batch=int(batches[0]))

'''
CPU test of the host-side feature mask (ptina_amd/csrc/shade_feat.h): which regions of the SHADE stage a scene needs, worked
out from the material table, the light list and the world light as mpt_load_materials / the launch site see them.  The header is
plain C with no dependencies; the test compiles its three functions into a scratch shared object and calls them on hand-made
tables packed the way MaterialPool packs them (fac[m][12][4], tex[m][12]).
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

TEXTURED, CLEARCOAT, TRANSMISSION, WORLD_TEXTURE, MANY_LIGHTS = 1, 2, 4, 8, 16
PLAIN, GENERIC = 0, 31

SHIM = '''
#include "shade_feat.h"
int t_bits(int k) {
    const int b[7] = { MPT_FEAT_TEXTURED_MATS, MPT_FEAT_CLEARCOAT, MPT_FEAT_TRANSMISSION, MPT_FEAT_WORLD_TEXTURE, MPT_FEAT_MANY_LIGHTS,
                       MPT_FEAT_PLAIN, MPT_FEAT_GENERIC };
    return b[k];
}
int t_material(const float *fac, const int32_t *tex) { return shade_feat_material(fac, tex); }
int t_scene(const unsigned char *bits, int nmats, int max_mtlid, int default_bits, int nlights, int world_tex) {
    return shade_feat_scene(bits, nmats, max_mtlid, default_bits, nlights, world_tex);
}
int t_inst(int scene_bits, int shade_spec) { return shade_feat_instantiation(scene_bits, shade_spec); }
'''


@pytest.fixture(scope='module')
def feat(tmp_path_factory):
    d = tmp_path_factory.mktemp('shade_feat')
    src, so = str(d / 'shim.c'), str(d / 'shim.so')
    with open(src, 'w') as f:
        f.write(SHIM)
    cc = os.environ.get('CC') or shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or '/opt/rocm/lib/llvm/bin/clang'
    subprocess.run([cc, '-std=c99', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so], check=True)
    lib = C.CDLL(so)
    lib.t_material.argtypes = [C.c_void_p, C.c_void_p]
    lib.t_scene.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    return lib


def pack(materials):
    '''(fac [m][12][4] f32, tex [m][12] i32) the way MaterialPool / ParameterPair.load pack a list of materials'''
    from ptina_amd.mtllib import MaterialPool, PARAMS
    pool = MaterialPool.__new__(MaterialPool)
    MaterialPool.__init__(pool, max(len(materials), 1))
    for i, mat in enumerate(materials):
        for (fac, tex), name in zip(mat, PARAMS):
            getattr(pool, name).load(i, fac, tex)
    return np.ascontiguousarray(pool._fac, np.float32), np.ascontiguousarray(pool._tex, np.int32)


def material_bits(lib, mat, with_tex=True):
    fac, tex = pack([mat])
    return lib.t_material(fac.ctypes.data, tex.ctypes.data if with_tex else None)


def scene_bits(lib, mats, max_mtlid, nlights=1, world_tex=-1, default_bits=None):
    fac, tex = pack(mats)
    bits = np.array([lib.t_material(fac[i].ctypes.data, tex[i].ctypes.data) for i in range(len(mats))], np.uint8)
    if default_bits is None:
        default_bits = material_bits(lib, scenes.material())          # PARAM_DEFAULTS are the default material's parameters (mtllib.py:82-93)
    return lib.t_scene(bits.ctypes.data if len(mats) else None, len(mats), max_mtlid, default_bits, nlights, world_tex)


def test_constants_are_the_documented_bits(feat):
    assert [feat.t_bits(k) for k in range(7)] == [TEXTURED, CLEARCOAT, TRANSMISSION, WORLD_TEXTURE, MANY_LIGHTS, PLAIN, GENERIC]
    assert TEXTURED | CLEARCOAT | TRANSMISSION | WORLD_TEXTURE | MANY_LIGHTS == GENERIC


def test_material_bits(feat):
    m = scenes.material
    assert material_bits(feat, m()) == 0                                             # the default material's parameters
    assert material_bits(feat, m(basecolor=(0.8, 0.6, 0.2), roughness=0.3, metallic=0.1, specular=0.5)) == 0
    assert material_bits(feat, m(sheen=1.0, sheenTint=0.8, subsurface=0.7, specularTint=1.0, clearcoatGloss=0.9, ior=2.0)) == 0
    assert material_bits(feat, scenes.gltf_compat_material((0.5, 0.5, 0.5), 0.5, 0.5)) == 0
    assert material_bits(feat, m(clearcoat=1.0)) == CLEARCOAT
    assert material_bits(feat, m(clearcoat=1e-30)) == CLEARCOAT                      # any non-zero value: the kernel compares with != 0
    assert material_bits(feat, m(clearcoat=-0.25)) == CLEARCOAT
    assert material_bits(feat, m(clearcoat=float('nan'))) == CLEARCOAT               # a NaN is != 0 on the device as well
    assert material_bits(feat, m(transmission=0.8, ior=1.5)) == TRANSMISSION
    assert material_bits(feat, m(transmission=0.5, clearcoat=0.5)) == CLEARCOAT | TRANSMISSION
    assert material_bits(feat, m(transmission=0.5), with_tex=False) == TRANSMISSION  # mpt_load_materials with tex = NULL


def test_textured_parameters(feat):
    for k, name in enumerate(scenes.PARAM_NAMES):
        mat = scenes.material()
        mat[k] = (mat[k][0], 3)
        want = TEXTURED | (CLEARCOAT if name == 'clearcoat' else 0) | (TRANSMISSION if name == 'transmission' else 0)
        assert material_bits(feat, mat) == want, name
    # parameter zero but textured: the lobe counts as used (the mask never looks into the image)
    mat = scenes.material(clearcoat=0.0, transmission=0.0)
    assert mat[8][0] == 0.0 and mat[10][0] == 0.0
    mat[8] = (0.0, 0)
    assert material_bits(feat, mat) == TEXTURED | CLEARCOAT
    mat[10] = (0.0, 7)
    assert material_bits(feat, mat) == TEXTURED | CLEARCOAT | TRANSMISSION
    # ... and without the texture table the same factors are plain
    assert material_bits(feat, mat, with_tex=False) == 0


def test_scene_mask_counts_only_the_materials_the_model_uses(feat):
    m = scenes.material
    mats = [m(), m(roughness=0.2), m(transmission=0.9), m(clearcoat=1.0)]
    assert scene_bits(feat, mats, max_mtlid=1) == PLAIN
    assert scene_bits(feat, mats, max_mtlid=2) == TRANSMISSION
    assert scene_bits(feat, mats, max_mtlid=3) == TRANSMISSION | CLEARCOAT
    assert scene_bits(feat, mats, max_mtlid=40) == TRANSMISSION | CLEARCOAT         # ids beyond the table: records never loaded, all zero
    assert scene_bits(feat, mats, max_mtlid=-1) == PLAIN                             # only the default material
    assert scene_bits(feat, [], max_mtlid=5) == PLAIN
    # the default material is always part of the scene (faces with material id -1 take it)
    assert scene_bits(feat, mats, max_mtlid=-1, default_bits=CLEARCOAT) == CLEARCOAT
    assert scene_bits(feat, mats, max_mtlid=1, default_bits=TEXTURED) == TEXTURED


def test_scene_mask_lights_and_world(feat):
    mats = list(scenes.scene_s978()[2])
    assert scene_bits(feat, mats, max_mtlid=3) == PLAIN
    assert scene_bits(feat, mats, max_mtlid=3, nlights=2) == MANY_LIGHTS
    assert scene_bits(feat, mats, max_mtlid=3, nlights=0) == MANY_LIGHTS            # no light at all is not "one light" either
    assert scene_bits(feat, mats, max_mtlid=3, nlights=64) == MANY_LIGHTS
    assert scene_bits(feat, mats, max_mtlid=3, world_tex=0) == WORLD_TEXTURE
    assert scene_bits(feat, mats, max_mtlid=3, nlights=3, world_tex=2) == WORLD_TEXTURE | MANY_LIGHTS


def test_benchmark_scenes_are_plain(feat):
    for name in ('s34', 's978'):
        v, mt, mats, imgs = scenes.get_scene(name)
        assert scene_bits(feat, list(mats), max_mtlid=int(mt.max())) == PLAIN, name


def test_two_instantiations_only(feat):
    for bits in range(32):
        assert feat.t_inst(bits, 1) == (PLAIN if bits == 0 else GENERIC)
        assert feat.t_inst(bits, 0) == GENERIC

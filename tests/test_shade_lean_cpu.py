'''
CPU test of the host-side choice of the lean SHADE variant (ptina_amd/csrc/shade_feat.h: shade_lean_material, shade_lean_scene,
shade_lean_instantiation).  The plain instantiation of the LDS-resident kernel has a variant compiled without the subsurface and
sheen terms of the diffuse lobe; a launch takes it when every material the model uses, and the default material, has both
parameters exactly zero and untextured.  The header is plain C: the test compiles the functions into a scratch shared object, as
test_shade_feat_cpu.py does, and calls them on tables packed the way MaterialPool packs them (fac[m][12][4], tex[m][12]).
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
PLAIN, GENERIC = 0, 31
SUBSURFACE, SHEEN = 5, 6                                                      # scenes.PARAM_NAMES

SHIM = '''
#include "shade_feat.h"
int t_feat(const float *fac, const int32_t *tex) { return shade_feat_material(fac, tex); }
int t_inst(int scene_bits, int shade_spec) { return shade_feat_instantiation(scene_bits, shade_spec); }
int t_lean_material(const float *fac, const int32_t *tex) { return shade_lean_material(fac, tex); }
int t_lean_scene(const unsigned char *lean, int nmats, int max_mtlid, int default_lean) {
    return shade_lean_scene(lean, nmats, max_mtlid, default_lean);
}
int t_lean_inst(int inst, int scene_lean, int lean_on) { return shade_lean_instantiation(inst, scene_lean, lean_on); }
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp('shade_lean')
    src, so = str(d / 'shim.c'), str(d / 'shim.so')
    with open(src, 'w') as f:
        f.write(SHIM)
    cc = os.environ.get('CC') or shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or '/opt/rocm/lib/llvm/bin/clang'
    subprocess.run([cc, '-std=c99', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so], check=True)
    lib = C.CDLL(so)
    lib.t_feat.argtypes = [C.c_void_p, C.c_void_p]
    lib.t_lean_material.argtypes = [C.c_void_p, C.c_void_p]
    lib.t_lean_scene.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    return lib


def pack(mat):
    '''(fac [12][4] f32, tex [12] i32) of one material the way ParameterPair.load packs it'''
    from ptina_amd.mtllib import MaterialPool, PARAMS
    pool = MaterialPool.__new__(MaterialPool)
    MaterialPool.__init__(pool, 1)
    for (fac, tex), name in zip(mat, PARAMS):
        getattr(pool, name).load(0, fac, tex)
    return np.ascontiguousarray(pool._fac[0], np.float32), np.ascontiguousarray(pool._tex[0], np.int32)


def lean_of(lib, mat, with_tex=True):
    fac, tex = pack(mat)
    return lib.t_lean_material(fac.ctypes.data, tex.ctypes.data if with_tex else None)


def scene_lean(lib, mats, max_mtlid, default_lean=None):
    flags = np.array([lean_of(lib, m) for m in mats], np.uint8)
    if default_lean is None:
        default_lean = lean_of(lib, scenes.material())
    return lib.t_lean_scene(flags.ctypes.data if len(mats) else None, len(mats), max_mtlid, default_lean)


def test_parameter_order():
    assert scenes.PARAM_NAMES[SUBSURFACE] == 'subsurface' and scenes.PARAM_NAMES[SHEEN] == 'sheen'


def test_zero_sheen_and_subsurface_is_lean(lib):
    m = scenes.material
    assert lean_of(lib, m()) == 1                                                    # the default material's parameters
    assert lean_of(lib, m(), with_tex=False) == 1                                    # mpt_load_materials with tex = NULL
    assert lean_of(lib, m(basecolor=(0.8, 0.6, 0.2), roughness=0.0, metallic=1.0, specular=0.9, specularTint=1.0, sheenTint=0.9)) == 1
    assert lean_of(lib, scenes.gltf_compat_material((0.5, 0.5, 0.5), 0.5, 0.5)) == 1
    # the other lobes do not matter here: such a scene is not plain, and lean is only offered to a plain one (below)
    assert lean_of(lib, m(clearcoat=1.0, transmission=0.5)) == 1
    # -0.0 is zero: the dropped terms are products with it
    assert lean_of(lib, m(sheen=-0.0, subsurface=-0.0)) == 1


@pytest.mark.parametrize('name', ['sheen', 'subsurface'])
@pytest.mark.parametrize('value', [1.0, 0.2, 1e-30, 1e-45, -0.25, -1e-30, float('nan'), float('inf'), float('-inf')])
def test_any_other_value_is_not_lean(lib, name, value):
    assert lean_of(lib, scenes.material(**{name: value})) == 0
    assert lean_of(lib, scenes.material(**{name: value}), with_tex=False) == 0


@pytest.mark.parametrize('k', [SUBSURFACE, SHEEN])
def test_zero_but_textured_is_not_lean(lib, k):
    mat = scenes.material()
    assert mat[k][0] == 0.0
    mat[k] = (0.0, 3)
    assert lean_of(lib, mat) == 0
    mat[k] = (0.0, 0)                                                                # image 0 is an image
    assert lean_of(lib, mat) == 0
    assert lean_of(lib, mat, with_tex=False) == 1                                    # ... and without the texture table the factors decide
    # a texture on any other parameter leaves the material lean (the scene is then not plain, by the feature mask)
    for j in range(12):
        if j not in (SUBSURFACE, SHEEN):
            other = scenes.material()
            other[j] = (other[j][0], 2)
            assert lean_of(lib, other) == 1, scenes.PARAM_NAMES[j]


def test_scene_counts_only_the_materials_the_model_uses(lib):
    m = scenes.material
    mats = [m(), m(roughness=0.2), m(sheen=0.3), m(subsurface=0.9)]
    assert scene_lean(lib, mats, max_mtlid=1) == 1                                   # records 2 and 3 are above max_mtlid: ignored
    assert scene_lean(lib, mats, max_mtlid=2) == 0
    assert scene_lean(lib, mats, max_mtlid=3) == 0
    assert scene_lean(lib, mats[:2] + mats[3:], max_mtlid=2) == 0                    # subsurface alone
    assert scene_lean(lib, mats, max_mtlid=-1) == 1                                  # only the default material
    assert scene_lean(lib, mats[:2], max_mtlid=40) == 1                              # ids beyond the table: records never loaded, all zero
    assert scene_lean(lib, [], max_mtlid=5) == 1


def test_the_default_material_is_counted(lib):
    m = scenes.material
    mats = [m(), m(roughness=0.2)]
    assert scene_lean(lib, mats, max_mtlid=1, default_lean=0) == 0
    assert scene_lean(lib, mats, max_mtlid=-1, default_lean=0) == 0
    assert scene_lean(lib, [], max_mtlid=-1, default_lean=0) == 0
    assert scene_lean(lib, [], max_mtlid=-1, default_lean=1) == 1


def test_lean_is_never_offered_with_a_feature_bit(lib):
    for bits in range(32):
        for spec in (0, 1):
            inst = lib.t_inst(bits, spec)
            for scene in (0, 1):
                for on in (0, 1):
                    want = 1 if (bits == PLAIN and spec == 1 and scene == 1 and on == 1) else 0
                    assert lib.t_lean_inst(inst, scene, on) == want, (bits, spec, scene, on)
    # whatever the caller passes for the instantiation, only the plain mask has the variant
    for inst in range(1, 32):
        assert lib.t_lean_inst(inst, 1, 1) == 0


def test_sheen_and_subsurface_leave_the_feature_mask_alone(lib):
    '''a scene with sheen or subsurface stays plain (tests/test_shade_feat_cpu.py pins it): it takes the plain kernel without the variant'''
    fac, tex = pack(scenes.material(sheen=1.0, subsurface=0.7))
    assert lib.t_feat(fac.ctypes.data, tex.ctypes.data) == PLAIN
    assert lib.t_lean_material(fac.ctypes.data, tex.ctypes.data) == 0


def test_benchmark_scenes_are_lean(lib):
    for name in ('s34', 's978'):
        v, mt, mats, imgs = scenes.get_scene(name)
        assert scene_lean(lib, list(mats), max_mtlid=int(mt.max())) == 1, name

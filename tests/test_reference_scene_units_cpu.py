'''
The C oracle's scene-reading functions held to vectors computed by the REFERENCE'S OWN function bodies
(tests/golden/reference_scene_units.npz, made by tests/golden/make_reference_scene_units_golden.py): lights_hit,
lights_sample, image_sample, world_at, material_get, camera_generate and the normal flip of get_geometries, through the
orc_unit_* entry points, which call the very functions orc_render calls on a context loaded through orc_add_light,
orc_add_image, orc_load_materials, orc_set_world, orc_set_camera_v2w and orc_load_model.

Both builds: the f64 oracle against the f64/ vectors (1e-12, discrete outputs equal), the f32 oracle against the f32/ ones
(the per-function bounds of tests/test_reference_l1_cpu.py, plus 4 x the reference's own f32-vs-f64 spread per output).
Bounds, masks and the checks themselves are in tests/scene_units.py, shared with the GPU file.  Every check prints its
worst error against its bound.
'''

import ctypes as C

import numpy as np
import pytest

import scene_units as SU


@pytest.fixture(scope='module')
def gold():
    return SU.load()


class OracleEval:
    def __init__(self, oracle_mod, gold, f64, state='five', world='env', camera=0):
        self.o = oracle_mod.Oracle(f64=f64, threads=1, sobol=False)
        self.lib, self.ctx, self.T, self.ct = self.o.lib, self.o.ctx, self.o.npreal, self.o.real
        self.o.load_images(SU.images_of(gold))
        self.o.load_materials(SU.materials_of(gold))
        self.o.clear_lights()
        for l in SU.lights_of(gold, state):
            self.o.add_light(*l)
        self.o.set_world_light(*SU.worlds_of(gold)[world])
        v2w = np.ascontiguousarray(gold['state/camera_v2w'][camera], np.float32)
        self.lib.orc_set_camera_v2w(self.ctx, v2w.ctypes.data_as(C.POINTER(C.c_float)))

    def _p(self, a):
        return a.ctypes.data_as(C.POINTER(self.ct))

    def _rows(self, rows, ncol, f):
        out = np.zeros((len(rows), ncol), self.T)
        for r, o in zip(np.ascontiguousarray(rows, self.T), out):
            rc = f(r, o)
            assert rc in (None, 0)
        return out

    def light_hit(self, rows):
        return self._rows(rows, 6, lambda r, o: self.lib.orc_unit_light_hit(self.ctx, self._p(r[0:3].copy()), self._p(r[3:6].copy()), self._p(o)))

    def light_sample(self, rows):
        return self._rows(rows, 8, lambda r, o: self.lib.orc_unit_light_sample(self.ctx, self._p(r[0:3].copy()), self._p(r[3:6].copy()), self._p(o)))

    def image_sample(self, rows):
        return self._rows(rows, 4, lambda r, o: self.lib.orc_unit_image_sample(self.ctx, int(r[0]), self.ct(r[1]), self.ct(r[2]), self._p(o)))

    def world_at(self, rows):
        return self._rows(rows, 3, lambda r, o: self.lib.orc_unit_world_at(self.ctx, self._p(r[0:3].copy()), self._p(o)))

    def material_get(self, rows):
        return self._rows(rows, 22, lambda r, o: self.lib.orc_unit_material_get(self.ctx, int(r[0]), self.ct(r[1]), self.ct(r[2]), self._p(o)))

    def camera_generate(self, rows):
        def f(r, o):
            self.lib.orc_camera_generate(self.ctx, self.ct(r[0]), self.ct(r[1]), self._p(o[0:3]), self._p(o[3:6]))
        return self._rows(rows, 6, f)

    def face_side(self, rows):
        '''rows: rd, vn0 vn1 vn2, s, t -- one face with these vertex normals and mtlid -1 is loaded per row'''
        zero = np.zeros(3, self.T)

        def f(r, o):
            v = np.zeros((3, 8), np.float32)
            v[:, 0:3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
            v[:, 3:6] = r[3:12].reshape(3, 3)
            self.o.load_model(v, np.array([-1], np.int32))
            return self.lib.orc_unit_face_side(self.ctx, 0, self.ct(r[12]), self.ct(r[13]), self._p(zero), self._p(r[0:3].copy()), self._p(o))
        return self._rows(rows, 4, f)


@pytest.fixture(scope='module', params=['f32', 'f64'])
def mode(request):
    return request.param


def test_fixture_covers_the_interesting_cases(gold):
    SU.check_coverage(gold)


@pytest.mark.parametrize('state', ['five', 'one', 'none'])
def test_lights_hit(gold, oracle_mod, mode, state):
    SU.check_light_hit(OracleEval(oracle_mod, gold, mode == 'f64', state=state), gold, mode, state)


@pytest.mark.parametrize('state', ['five', 'one', 'none'])
def test_lights_sample(gold, oracle_mod, mode, state):
    SU.check_light_sample(OracleEval(oracle_mod, gold, mode == 'f64', state=state), gold, mode, state)


def test_image_sample(gold, oracle_mod, mode):
    SU.check_image_sample(OracleEval(oracle_mod, gold, mode == 'f64'), gold, mode)


@pytest.mark.parametrize('state', ['plain', 'env'])
def test_world_at(gold, oracle_mod, mode, state):
    SU.check_world_at(OracleEval(oracle_mod, gold, mode == 'f64', world=state), gold, mode, state)


def test_material_get(gold, oracle_mod, mode):
    SU.check_material_get(OracleEval(oracle_mod, gold, mode == 'f64'), gold, mode)


@pytest.mark.parametrize('camera', [0, 1])
def test_camera_generate(gold, oracle_mod, mode, camera):
    SU.check_camera_generate(OracleEval(oracle_mod, gold, mode == 'f64', camera=camera), gold, mode, camera)


def test_face_side(gold, oracle_mod, mode):
    SU.check_face_side(OracleEval(oracle_mod, gold, mode == 'f64'), gold, mode)


def test_unit_entry_points_refuse_what_the_context_does_not_hold(gold, oracle_mod):
    ev = OracleEval(oracle_mod, gold, False)
    out = np.zeros(22, np.float32)
    assert ev.lib.orc_unit_image_sample(ev.ctx, 4, 0.5, 0.5, ev._p(out)) == -1
    assert ev.lib.orc_unit_material_get(ev.ctx, 3, 0.5, 0.5, ev._p(out)) == -1
    assert ev.lib.orc_unit_face_side(ev.ctx, 0, 0.25, 0.25, ev._p(out), ev._p(out), ev._p(out)) == -1      # no model loaded

#!/usr/bin/env python3
'''
Cross-check vectors of the brute-force engine: the reference's OWN BruteEngine source -- render / _render / trace
(engine/brute.py:24-74) with everything it calls (LinearBVH, GlobalStack, the pools, WorldLight, Camera, FilmTable,
SobolSampler) -- imported from the reference tree and executed as plain Python on numpy scalars under the `taichi`
stand-in of tests/golden/taichi_standin, in single and double precision.

Cases, scenes, camera and the stand-in set-up are those of make_reference_path_golden.py (its CASES and scene_of are
imported; the set-up of the stand-in's namespaces is restated here because that generator keeps it inside the function
that also renders the path films).  Per case the call sequence is exams/benchmark.py's with the engine swapped:
render(); clear(); spp x render().  The raw film sums (radiance sums and sample weights per pixel), the film size and
the Sobol `time` after the sequence go to tests/golden/reference_brute.npz; tests/test_brute_cpu.py checks the file's
own consistency and tests/test_brute_gpu.py holds the HIP kernel to it.

Nothing of the reference is copied: it is imported and run.  Build container only; takes a few minutes (the Sobol
set-up is a Python loop over 21201 dimensions).

usage: python3 tests/golden/make_reference_brute_golden.py            (spawns one child per precision)
'''

import os
import subprocess
import sys
import time
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_reference_path_golden as G   # noqa: E402  (CASES, scene_of, REF)

CASES = G.CASES


def child(prec):
    T = np.float64 if prec == 'f64' else np.float32
    sys.path.insert(0, os.path.join(HERE, 'taichi_standin'))
    sys.path.insert(0, G.REF)
    warnings.filterwarnings('ignore', category=RuntimeWarning)
    import taichi as ti
    assert 'taichi_standin' in ti.__file__
    ti.set_default_fp(T)

    # pysobol.data._sobol_data: flat [s, a, m_1 .. m_s] per dimension >= 1, served from the project's Joe-Kuo table
    z = np.load(os.path.join(ROOT, 'ptina_amd', 'data', 'joe_kuo_21201.npz'))
    flat = []
    for j in range(1, z['s'].shape[0]):
        s = int(z['s'][j])
        flat += [s, int(z['a'][j])] + [int(x) for x in z['m'][j][:s]]
    pysobol = types.ModuleType('pysobol')
    pysobol.data = types.ModuleType('pysobol.data')
    pysobol.data._sobol_data = flat
    sys.modules['pysobol'] = pysobol
    sys.modules['pysobol.data'] = pysobol.data

    import ptina.common as C
    from ptina.things import init_things, Camera, BVHTree, ImagePool, ModelPool, LightPool, WorldLight, \
        MaterialPool, FilmTable
    from ptina.engine.brute import BruteEngine
    from ptina.sampling.sobol import SobolSampler
    from ptina.image import Image
    import ptina.sampling as SAMP
    import ptina.tree.lbvh as LBVH
    import ptina.tools.matrix  # noqa: F401  (host code, imported lazily by Camera(): before the kernel-scope names below exist)
    # kernel-scope builtins, exactly the patches of the path generator and nothing more
    C.int, C.float, C.min, C.max = ti.ti_int, ti.ti_float, ti.min, ti.max
    SAMP.int = ti.ti_int
    LBVH.min, LBVH.max = ti.min, ti.max
    assert SAMP.wanghash2(3, 5) == -1977258872 and isinstance(SAMP.wanghash2(3, 5), ti.I32)
    # the `subscript` protocol of is_taichi_class objects
    ModelPool.__getitem__ = lambda self, i: self.subscript(i)
    FilmTable.__getitem__ = lambda self, ix: self.subscript(*ix)
    FilmTable.__setitem__ = lambda self, ix, v: self.root.__setitem__((ix[0], ix[1] * self.ny + ix[2]), v)
    ImagePool.__getitem__ = lambda self, ix: self.subscript(*ix)
    Image.__getitem__ = lambda self, I: self.subscript(*I)

    out = {}
    t0 = time.time()
    init_things(max_faces=2**10, max_texels=2**10, max_materials=2**4, max_textures=2**2, max_lights=2**3,
                max_filmsize=2**10, max_filmpasses=3)
    eng = BruteEngine()                       # SobolSampler(): vgrid + reset (64 skipped updates)
    sob = SobolSampler()
    print(prec, 'sobol ready after %.0f s, time =' % (time.time() - t0), sob.time[None], flush=True)
    assert int(sob.time[None]) == 64
    sobol_state = (sob.X.to_numpy(), sob.P.to_numpy(), int(sob.time[None]))

    for name, (key, nx, ny, spp) in CASES.items():
        scene, lights, world = G.scene_of(key)
        vertices, mtlids, materials, images = scene
        # rewind the sampler to its state after reset() (what a fresh process would have)
        sob.X.from_numpy(sobol_state[0])
        sob.P.from_numpy(sobol_state[1])
        sob.time[None] = sobol_state[2]

        FilmTable().set_size(nx, ny)
        n = mtlids.shape[0]
        ModelPool().vertices.from_numpy(np.asarray(vertices, np.float32).reshape(-1))
        ModelPool().mtlids.from_numpy(np.asarray(mtlids, np.int32))
        ModelPool().nfaces[None] = n
        MaterialPool().load(materials)
        # the reference's image loader's conversions, ids and offsets from its own allocators, texels stored directly
        pool = ImagePool()
        pool.mman.reset()
        pool.idman.reset()
        for arr in images:
            arr = np.asarray(arr)
            if arr.dtype == np.uint8:
                arr = arr.astype(np.float32) / 255
            if arr.ndim == 2:
                arr = arr[:, :, None]
            if arr.shape[2] == 1:
                arr = np.stack([arr[:, :, 0]] * 3, axis=2)
            if arr.shape[2] == 3:
                arr = np.concatenate([arr, np.ones(arr.shape[:2] + (1,))], axis=2)
            iid = pool.new(arr.shape[0], arr.shape[1])
            base = int(pool.base[iid])
            pool.root.data[base:base + arr.shape[0] * arr.shape[1]] = arr.astype(np.float32).reshape(-1, 4)
        BVHTree().build()
        from ptina_amd import scenes
        Camera().set_perspective(np.array(scenes.BENCH_CAMERA))
        WorldLight().set(*world)
        LightPool().clear()
        if lights is not None:
            for l in lights:
                LightPool().add(*l)
        else:                                 # back to the default light: a point light of colour 32 at (1, 2, 3), radius 0.5
            LightPool().color[0] = [32, 32, 32]
            LightPool().pos[0] = [1, 2, 3]
            LightPool().size[0] = 0.5
            LightPool().type[0] = LightPool.TYPES['POINT']
            LightPool().count[None] = 1

        if prec == 'f64':
            # the C ABI takes f32 scene parameters: the double-precision run starts from exactly those values
            def f32_values(fld):
                fld.data[...] = fld.data.astype(np.float32).astype(np.float64)
            mp = MaterialPool()
            for pair in (mp.basecolor, mp.metallic, mp.roughness, mp.specular, mp.specularTint, mp.subsurface, mp.sheen,
                         mp.sheenTint, mp.clearcoat, mp.clearcoatGloss, mp.transmission, mp.ior):
                f32_values(pair.fac)
            for fld in (Camera()._V2W, Camera()._W2V, LightPool().color, LightPool().pos, LightPool().axes, LightPool().size,
                        WorldLight().fac):
                f32_values(fld)

        t1 = time.time()
        eng.render()                          # warm-up frame, (read back), clear
        FilmTable().clear()
        for _ in range(spp):
            eng.render()
        film = FilmTable().root.to_numpy()[0, :nx * ny].astype(np.float64)
        assert np.all(film[:, 3] == spp) and not np.isnan(film).any()
        assert int(sob.time[None]) == 64 + 1 + spp
        out[f'{name}/film'] = film
        out[f'{name}/size'] = np.array([nx, ny, spp], np.int64)
        out[f'{name}/sobol_time'] = np.int64(sob.time[None])
        print(prec, name, 'rendered in %.0f s; mean radiance' % (time.time() - t1), film[:, :3].mean() / spp, flush=True)
    np.savez_compressed(os.path.join(HERE, f'_reference_brute_{prec}.npz'), **out)


def main():
    if len(sys.argv) > 1:
        return child(sys.argv[1])
    merged = {}
    procs = [(p, subprocess.Popen([sys.executable, os.path.abspath(__file__), p])) for p in ('f32', 'f64')]
    for p, proc in procs:
        if proc.wait() != 0:
            raise SystemExit(f'{p} run failed')
    for p, _ in procs:
        f = os.path.join(HERE, f'_reference_brute_{p}.npz')
        z = np.load(f)
        for k in z.files:
            merged[f'{p}/{k}'] = z[k]
        z.close()
        os.remove(f)
    dst = os.path.join(HERE, 'reference_brute.npz')
    np.savez_compressed(dst, **merged)
    print('wrote', dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()

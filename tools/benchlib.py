'''
What the feature benchmarks (tools/{mlt,brute,denoise,display,noise}_bench.py) share: the scene set up as exams/benchmark_amd.py
does, the median, and the wall-clock loop around one call.
'''
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def setup(size, scene='s978', preview=False):
    '''a fresh context with `scene` (a name of ptina_amd.scenes, or its (vertices, mtlids, materials, images)) loaded, the tree built,
    the benchmark camera and a size x size film (production build, the library's default mode); returns (PathEngine, FilmTable), or
    (PathEngine, PreviewEngine, FilmTable) with preview=True'''
    from ptina_amd import scenes
    from ptina_amd.common import reset_all
    from ptina_amd.things import init_things, FilmTable, ModelPool, MaterialPool, ImagePool, BVHTree, Camera
    from ptina_amd.engine.path import PathEngine
    from ptina_amd.engine.preview import PreviewEngine
    reset_all()
    init_things(max_filmsize=max(size * size, 2**21))
    path = PathEngine()
    FilmTable().set_size(size, size)
    vertices, mtlids, materials, images = scenes.get_scene(scene) if isinstance(scene, str) else scene
    ModelPool().load(vertices, mtlids)
    MaterialPool().load(materials)
    ImagePool().load(images)
    BVHTree().build()
    Camera().set_perspective(scenes.BENCH_CAMERA)
    return (path, PreviewEngine(), FilmTable()) if preview else (path, FilmTable())


def median(v):
    return sorted(v)[len(v) // 2]


def wall_ms(call, repeat, prepare=None, after=None):
    '''(median, least) wall time in ms of `repeat` calls after two warm-up calls; `prepare` runs before each call and `after`
    behind it, both outside the timed part'''
    ms = []
    for i in range(repeat + 2):
        if prepare:
            prepare()
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
        if after:
            after()
    ms = ms[2:]
    return round(median(ms), 4), round(min(ms), 4)

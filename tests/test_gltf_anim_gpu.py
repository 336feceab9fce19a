'''
GPU tests (-m gpu) of the animated-glTF loader (ptina_amd.scenes.load_gltf_scene): the fixture
tests/golden/animated_scene.gltf loaded, played and composed at the four times of tests/golden/animated_scene_expected.npz -- t = 0, a
key time, a time between keys, a time behind the last key -- and every object's world matrix, the strip's pose and its deformed
vertices held to what the generator's own walk of the node tree wrote, BIT FOR BIT: the fixture keeps its LINEAR rotation tracks off
the slerp's theta branch (make_gltf_anim_golden.py says why), so nothing here needs the bound that branch carries.
'''

import os

import numpy as np
import pytest

from test_anim_gpu import _same, _start

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLTF = os.path.join(ROOT, 'tests', 'golden', 'animated_scene.gltf')


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_the_loaded_scene_plays_to_what_the_generator_evaluated(fresh):
    from ptina_amd.scenes import load_gltf_scene
    want = np.load(os.path.join(ROOT, 'tests', 'golden', 'animated_scene_expected.npz'))
    pool = _start()
    H = load_gltf_scene(GLTF)
    assert H.animations == ['wave']
    assert sorted(H.objects) == [0, 1, 2, 3, 4, 7, 8] and [len(H.objects[n]) for n in sorted(H.objects)] == [1, 1, 1, 1, 1, 1, 2]
    strip, prop = H.objects[3][0], H.objects[7][0]
    # the calls the loader made, as the stats count them: one skeleton; one mesh clip and two object clips; six parent bindings, two deep
    a, b, h = pool.anim_stats(), pool.anim_blend_stats(), pool.hierarchy_stats()
    assert (a.skeletons, a.clips, b.object_clips, a.bound_objects, b.moved_objects) == (1, 3, 2, 0, 0)
    assert (h.bound_children, h.deepest) == (6, 2)
    assert pool.parent_of(prop) == (strip, 1) and pool.parent_of(strip) == (H.objects[4][0], None) and pool.parent_of(H.objects[4][0]) is None
    assert pool.parent_of(H.objects[2][0]) == (H.objects[1][0], None) and {pool.parent_of(o) for o in H.objects[8]} == {(H.objects[0][0], None)}
    H.play('wave', loop=False)
    a, b = pool.anim_stats(), pool.anim_blend_stats()
    assert (a.bound_objects, b.moved_objects) == (1, 2)
    seen = []
    for k, t in enumerate(want['times']):
        pool.set_time(float(t))
        pool.compose()
        for node, ids in H.objects.items():
            for obj in ids:
                got = pool.world_to_numpy(obj)
                assert _bits(got, want['world_%d' % k][node]), (k, node, float(np.abs(got - want['world_%d' % k][node]).max()))
        w, pal = pool.pose_to_numpy(strip)
        assert _bits(w, want['weights_%d' % k]) and _bits(pal, want['palette_%d' % k]), (k, float(np.abs(pal - want['palette_%d' % k]).max()))
        rec = pool.deformed_to_numpy(strip)
        assert _same(rec, want['deformed_%d' % k]), (k, float(np.abs(rec - want['deformed_%d' % k]).max()))
        seen.append(pool.to_numpy()[0].copy())
        if k > 0:                                                          # set_time moved the two animated nodes, the strip and all below them
            assert pool.hierarchy_stats().evaluated == 6 and pool.hierarchy_stats().launches == 1 and pool.anim_blend_stats().evaluated_moved == 1
    assert not _same(seen[0], seen[1]) and not _same(seen[1], seen[2]) and not _same(seen[2], seen[3])
    assert np.isfinite(seen[3]).all() and seen[3].shape[0] == 3 * (1 + 4 + 1 + 2)
    # nothing bound: every object back at its node's own transform, the strip at its rest pose
    H.play(None)
    pool.compose()
    assert pool.anim_blend_stats().moved_objects == 0 and pool.anim_stats().bound_objects == 0
    assert _bits(pool.world_to_numpy(H.objects[0][0]), want['local'][0])

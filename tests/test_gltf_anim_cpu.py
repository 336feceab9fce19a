'''
CPU tests of the animated-glTF reader (ptina_amd.tools.readgltf.read_gltf_scene): the fixture
tests/golden/animated_scene.gltf against the arrays its generator wrote beside it (tests/golden/make_gltf_anim_golden.py:
animated_scene_expected.npz), and every NotImplementedError on a small variant of the fixture written to tmp_path.
'''

import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLTF = os.path.join(ROOT, 'tests', 'golden', 'animated_scene.gltf')


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def want():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'animated_scene_expected.npz'))


@pytest.fixture(scope='module')
def desc():
    from ptina_amd.tools.readgltf import read_gltf_scene
    return read_gltf_scene(GLTF)


def test_the_fixture_is_small_and_readgltf_still_flattens_it():
    from ptina_amd.tools.readgltf import readgltf
    assert os.path.getsize(GLTF) < 16384
    verts, mtlids, materials, images = readgltf(GLTF)                       # the old door is as it was: everything flattened, nothing animated
    assert verts.shape == (3 * (1 + 4 + 1 + 2), 8) and len(materials) == 2


def test_nodes_meshes_and_skins_are_what_the_generator_wrote(desc, want):
    nodes = desc['nodes']
    assert [n['parent'] for n in nodes] == want['parents'].tolist()
    assert [n['name'] for n in nodes] == ['base', 'arm', 'lamp', 'strip', 'rig', 'joint0', 'joint1', 'prop', 'pair']
    for i, n in enumerate(nodes):
        assert _bits(n['local'], want['local'][i]), n['name']
        assert n['matrix'] is None
    assert [n['mesh'] for n in nodes] == [-1, -1, 0, 1, -1, -1, -1, 0, 2] and [n['skin'] for n in nodes] == [-1, -1, -1, 0, -1, -1, -1, -1, -1]
    assert desc['roots'] == [0, 3, 4]
    tri, strip, pair = desc['meshes']
    assert [len(m['primitives']) for m in desc['meshes']] == [1, 1, 2]
    s = strip['primitives'][0]
    for key, got in (('strip_p', s['p']), ('strip_n', s['n']), ('strip_t', s['t']), ('strip_joints', s['joints']), ('strip_weights', s['weights']),
                     ('strip_dp', s['dp']), ('strip_dn', s['dn'])):
        assert _bits(got, want[key]), key
    assert _bits(tri['primitives'][0]['p'], want['tri_p']) and _bits(pair['primitives'][1]['p'], want['tri2_p'])
    assert tri['primitives'][0]['joints'] is None and tri['primitives'][0]['dp'] is None
    assert (tri['primitives'][0]['material'], s['material'], pair['primitives'][1]['material']) == (0, 1, -1)
    assert strip['weights'].tolist() == [0.0]
    skin, = desc['skins']
    assert skin['joints'] == [5, 6] and skin['parents'].tolist() == [-1, 0] and skin['root_parent'] == 4
    assert _bits(skin['inverse_bind'], want['inverse_bind'])
    assert desc['joint_of'] == {5: (0, 0), 6: (0, 1)} and desc['carriers'] == [0, 1, 2, 4, 7, 8]


def test_animations_are_tracks_as_tools_anim_takes_them(desc, want):
    from ptina_amd.tools.anim import track
    anim, = desc['animations']
    assert anim['name'] == 'wave' and [c['node'] for c in anim['channels']] == want['channel_nodes'].tolist()
    assert {c['interpolation'] for c in anim['channels']} == {'STEP', 'LINEAR', 'CUBICSPLINE'}
    assert [c['path'] for c in anim['channels']] == ['translation', 'rotation', 'rotation', 'scale', 'translation', 'rotation', 'weights']
    assert _bits(anim['channels'][1]['values'], want['rotation_keys']) and anim['channels'][1]['values'].shape == (4, 3, 4)
    assert _bits(anim['channels'][6]['values'], want['weight_keys'])
    for c in anim['channels']:
        tr = track(-1 if c['path'] == 'weights' else 0, c['path'], c['times'], c['values'], c['interpolation'])
        assert tr.times.size == c['times'].size


def _variant(tmp_path, edit):
    doc = json.load(open(GLTF))
    edit(doc)
    path = str(tmp_path / 'variant.gltf')
    json.dump(doc, open(path, 'w'))
    return path


def _sparse(d):
    d['accessors'][0]['sparse'] = dict(count=1, indices=dict(bufferView=0, componentType=5123), values=dict(bufferView=0))


def _split_roots(d):                                   # joint 6 out from under joint 5: two root joints with different parents
    d['nodes'][5]['children'] = []
    d['nodes'][0]['children'].append(6)


def _between(d):                                       # a node that is no joint between the two joints
    d['nodes'].append(dict(name='spacer', children=[6]))
    d['nodes'][5]['children'] = [9]


def _second_set(d):
    at = d['meshes'][1]['primitives'][0]['attributes']
    at['JOINTS_1'], at['WEIGHTS_1'] = at['JOINTS_0'], at['WEIGHTS_0']


def _stray_channel(d):                                 # a node that leads to no mesh, animated
    d['nodes'].append(dict(name='stray'))
    d['scenes'][0]['nodes'].append(9)
    d['animations'][0]['channels'].append(dict(sampler=0, target=dict(node=9, path='translation')))


def _many_joints(d):
    d['skins'][0]['joints'] = [5, 6] + [5] * 255
    d['skins'][0].pop('inverseBindMatrices')


def _many_targets(d):
    pr = d['meshes'][1]['primitives'][0]
    pr['targets'] = pr['targets'] * 65


@pytest.mark.parametrize('edit, words', [
    (_sparse, 'sparse accessors'),
    (lambda d: d.update(extensionsRequired=['KHR_draco_mesh_compression']), 'required extensions'),
    (lambda d: (d.update(cameras=[dict(type='perspective', perspective=dict(yfov=1.0, znear=0.1))]), d['nodes'][4].update(camera=0)), 'cameras'),
    (_split_roots, 'root joints with different parents'),
    (_between, 'no joint between two joints'),
    (_second_set, r'second set of influences \(JOINTS_1\)'),
    (_stray_channel, 'channel on node 9, which leads to no mesh'),
    (_many_joints, '257 joints in skin 0, more than the 256'),
    (_many_targets, '65 morph targets on mesh 1, more than the 64'),
], ids=['sparse', 'extensions', 'cameras', 'split roots', 'between joints', 'JOINTS_1', 'stray channel', 'joints', 'targets'])
def test_what_is_not_loaded_is_refused_by_name(tmp_path, edit, words):
    from ptina_amd.tools.readgltf import read_gltf_scene
    with pytest.raises(NotImplementedError, match='variant.gltf: .*' + words):
        read_gltf_scene(_variant(tmp_path, edit))
    read_gltf_scene(_variant(tmp_path, lambda d: None))                     # ... and the fixture itself, written the same way, is read


def test_the_generator_writes_the_committed_files_again(tmp_path):
    '''the fixture is what its generator makes: run again into tmp_path, it writes the same bytes of glTF and the same arrays'''
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_gltf_anim_golden', os.path.join(ROOT, 'tests', 'golden', 'make_gltf_anim_golden.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.HERE = str(tmp_path)
    gen.main()
    assert open(tmp_path / 'animated_scene.gltf').read() == open(GLTF).read()
    a, b = np.load(tmp_path / 'animated_scene_expected.npz'), np.load(os.path.join(ROOT, 'tests', 'golden', 'animated_scene_expected.npz'))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].tobytes() == b[k].tobytes(), k

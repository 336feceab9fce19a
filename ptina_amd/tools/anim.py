'''
keyframe clips written by hand (glTF 2.0, "Animations"): what ModelPool().add_skeleton and add_clip take.  numpy on the host, once:
the clips stay on the device and are evaluated there at every ModelPool().set_time (csrc/anim.hip).
'''

import collections

import numpy as np

PATHS = {'T': 0, 'R': 1, 'S': 2, 'W': 3, 'translation': 0, 'rotation': 1, 'scale': 2, 'weights': 3}
INTERPOLATIONS = {'STEP': 0, 'LINEAR': 1, 'CUBICSPLINE': 2}

Track = collections.namedtuple('Track', 'target path interpolation times values')
Track.__doc__ = '''a track of a clip: target (a joint, or -1: the morph weights), path 0..3 (T R S W), interpolation 0..2 (STEP LINEAR
CUBICSPLINE), times [n] f32, values [n,C] f32 -- CUBICSPLINE: [n,3,C], in-tangent, value, out-tangent'''


def track(target, path, times, values, interpolation='LINEAR'):
    '''a Track: `target` a joint index (None or -1 for path 'W', the morph weights), `path` 'T', 'R', 'S' or 'W' (or glTF's
    'translation', 'rotation', 'scale', 'weights'), key times [n], values [n,C] with C = 3, 4 (x y z w), 3 or the mesh's morph
    targets -- [n,3,C] (in-tangent, value, out-tangent) for interpolation 'CUBICSPLINE'.  Times and values are stored as f32'''
    if path not in PATHS:
        raise ValueError('path %r: one of %s' % (path, ', '.join(PATHS)))
    if interpolation not in INTERPOLATIONS:
        raise ValueError('interpolation %r: one of %s' % (interpolation, ', '.join(INTERPOLATIONS)))
    p, i = PATHS[path], INTERPOLATIONS[interpolation]
    target = -1 if target is None else int(target)
    times = np.ascontiguousarray(times, np.float32).reshape(-1)
    values = np.ascontiguousarray(values, np.float32)
    n = times.size
    want = (n, 3, -1) if i == 2 else (n, -1)
    if n < 1 or values.size % (n * (3 if i == 2 else 1)):
        raise ValueError('%d key times and values of shape %s do not go together' % (n, values.shape))
    values = values.reshape(want)
    C = values.shape[-1]
    if p != 3 and C != (4 if p == 1 else 3):
        raise ValueError('a %s track has %d values per key, got %d' % ('TRSW'[p], 4 if p == 1 else 3, C))
    return Track(target, p, i, times, values)


def pack_clip(tracks):
    '''(spec [n,4] int32 of target, path, interpolation, nkeys; times f32; values f32, the tracks' arrays back to back): the flat
    form of a list of Tracks that the library takes (mpt_mesh_add_clip, mpt_clip_check, mpt_anim_rule)'''
    tracks = [t if isinstance(t, Track) else track(*t) for t in tracks]
    spec = np.array([[t.target, t.path, t.interpolation, t.times.size] for t in tracks], np.int32).reshape(-1, 4)
    times = np.concatenate([t.times for t in tracks]) if tracks else np.zeros(0, np.float32)
    values = np.concatenate([t.values.reshape(-1) for t in tracks]) if tracks else np.zeros(0, np.float32)
    return spec, np.ascontiguousarray(times, np.float32), np.ascontiguousarray(values, np.float32)


def quaternion(axis, angle):
    '''the rotation by `angle` radians about `axis` as x y z w, f64'''
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.array([*(np.sin(0.5 * angle) * axis), np.cos(0.5 * angle)])


def rest_pose(n, translation=None, rotation=None, scale=None):
    '''(translation [n,3], rotation [n,4], scale [n,3]) f64 of n joints: zeros, identity rotations and ones where None'''
    t = np.zeros((n, 3)) if translation is None else np.array(translation, np.float64).reshape(n, 3)
    r = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)) if rotation is None else np.array(rotation, np.float64).reshape(n, 4)
    s = np.ones((n, 3)) if scale is None else np.array(scale, np.float64).reshape(n, 3)
    return t, r, s


def local_matrices(translation, rotation, scale):
    '''[n,4,4] f64: the joints' local transforms T . R . S, what tools.skin.joint_matrices takes'''
    t, q, s = (np.asarray(a, np.float64) for a in (translation, rotation, scale))
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    out = np.zeros((t.shape[0], 4, 4))
    out[:, :3, :3] = R * s[:, None, :]
    out[:, :3, 3] = t
    out[:, 3, 3] = 1.0
    return out

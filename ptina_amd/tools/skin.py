'''
the joint palette of a skin (glTF 2.0, "Skins"): what ModelPool().set_joints takes.  numpy f64, on the host: a palette is a few
KB per pose, the corners it moves stay on the device (csrc/deform.hip).
'''

import numpy as np


def joint_matrices(parents, local, inverse_bind):
    '''globalJoint[j] . inverseBind[j] for every joint, [n,4,4] f64: parents [n] names each joint's parent (-1: a root), local
    [n,4,4] its transform relative to the parent, inverse_bind [n,4,4] the skin's inverse bind matrices.  Parents come before
    their children (the order glTF exporters write); ValueError otherwise.  The bottom rows come out exactly 0 0 0 1 when the
    inputs' are'''
    parents = np.asarray(parents)
    local, inverse_bind = np.asarray(local, np.float64), np.asarray(inverse_bind, np.float64)
    n = parents.shape[0] if parents.ndim == 1 else -1
    if local.shape != (n, 4, 4) or inverse_bind.shape != (n, 4, 4):
        raise ValueError('parents [n], local and inverse_bind [n,4,4] expected, got %s, %s and %s' % (parents.shape, local.shape, inverse_bind.shape))
    if n and not np.issubdtype(parents.dtype, np.integer):
        raise ValueError('parents must be integers, got %s' % parents.dtype)
    glob = np.empty((n, 4, 4), np.float64)
    for j in range(n):
        p = int(parents[j])
        if p < -1 or p >= j:
            raise ValueError('joint %d has parent %d: parents must come before their children (-1: a root)' % (j, p))
        glob[j] = local[j] if p < 0 else glob[p] @ local[j]
    return np.stack([glob[j] @ inverse_bind[j] for j in range(n)]) if n else glob


def attach(inverse_bind_j, local):
    '''the local matrix [4,4] f64 to give an object that ModelPool().set_parent binds to a joint, for `local` given in the joint's own
    frame: inverse(inverse_bind_j) . local.  The device multiplies a bound child by the joint's skinning matrix global . inverseBind
    (DESIGN.md section 3.17.3); with the bind matrix folded in, the child sits at global . local'''
    ib, local = np.asarray(inverse_bind_j, np.float64), np.asarray(local, np.float64)
    if ib.shape == (3, 4):
        ib = np.concatenate([ib, [[0.0, 0.0, 0.0, 1.0]]])
    if ib.shape != (4, 4) or local.shape != (4, 4):
        raise ValueError('inverse_bind_j [4,4] (or [3,4]) and local [4,4] expected, got %s and %s' % (ib.shape, local.shape))
    return np.linalg.inv(ib) @ local

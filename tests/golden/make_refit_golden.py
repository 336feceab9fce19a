'''
Records tests/golden/refit_records.npz from this project's own tree build (needs the GPU): for n = 5, 33, 300 and 1025 random
triangles (scenes.scene_random_tris(n, seed=n, edge=0.05)) the start positions, BVHTree().to_numpy()'s arrays and the 4-wide
records exact and quantised, as the default builders leave them.  tests/test_refit_cpu.py holds tests/refit_ref.py to these
bytes: a refit to the SAME vertices must give the build's records back.

    python tests/golden/make_refit_golden.py [out.npz]
'''

import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIZES = (5, 33, 300, 1025)


def main(out):
    from ptina_amd import scenes, _lib
    from ptina_amd.common import ctx, reset_all
    from ptina_amd.things import init_things, ModelPool, BVHTree
    rec = {'sizes': np.array(SIZES, np.int32)}
    for n in SIZES:
        reset_all()
        init_things()
        v, m, _, _ = scenes.scene_random_tris(n, seed=n, edge=0.05)
        ModelPool().load(v, m)
        BVHTree().build()
        t = BVHTree().to_numpy()
        nw = C.c_int(0)
        ctx().call('mpt_get_wide', None, None, 0, C.byref(nw))
        w = np.zeros((nw.value, 8, 4), np.float32)
        q = np.zeros((nw.value, 4, 4), np.float32)
        ctx().call('mpt_get_wide', _lib.fptr(w), _lib.fptr(q), nw.value, C.byref(nw))
        rec[f'pos_{n}'] = np.ascontiguousarray(np.asarray(v, np.float32).reshape(n, 3, 8)[:, :, :3])
        for k in ('child', 'leaf', 'bmin', 'bmax', 'mc'):
            rec[f'{k}_{n}'] = t[k]
        rec[f'depth_{n}'] = np.int32(t['depth'])
        rec[f'wnode_{n}'] = w.view(np.uint32)
        rec[f'qnode_{n}'] = q.view(np.uint32)
    reset_all()
    np.savez_compressed(out, **rec)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'refit_records.npz'))

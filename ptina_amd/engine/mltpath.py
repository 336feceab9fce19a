'''
Metropolis light transport over the path integrator (reference engine/mltpath.py): nchains chains
of 32-dim primary-sample vectors; each render() iteration every chain proposes a large step (all
dims fresh, probability LSP) or a small one (X + Sigma * normal, mod 1), traces the proposal's path,
splats it into film pass 0 with weight 1 and accepts it with probability
min(1, avg(L_new) / avg(L_old)).  The chain kernel and the deterministic splat pass are
csrc/mlt_kernel.hip.

The reference's ti.random() is a hash of (seed, chain, iteration, slot) here, so a run repeats bit
for bit.  Single GPU only.
'''

from .path import *                   # noqa: F401,F403  (the reference star-imports engine.path)
from ..common import Singleton, register, ctx, np
from ..sampling.sobol import SobolSampler
import ctypes as C


class _Scalar:
    '''a 0-d field as the reference's ti.field(float, ()): read and written as f[None]'''

    def __init__(self, value, on_set):
        self._value = float(np.float32(value))
        self._on_set = on_set

    def __getitem__(self, key):
        return self._value

    def __setitem__(self, key, value):
        self._value = float(np.float32(value))
        self._on_set()

    def to_numpy(self):
        return np.array(self._value, np.float32)


@register
class MLTPathEngine(metaclass=Singleton):
    def __init__(self, nchains=2**18, seed=0):
        SobolSampler()                    # (the context's render parameters need the sampler, as PreviewEngine's do)
        self.nchains = int(nchains)       # mltpath.py:12-13
        self.ndims = 32
        self.seed = int(seed) & 0xffffffff
        self.LSP = _Scalar(0.25, self._push_params)      # mltpath.py:26-27
        self.Sigma = _Scalar(0.01, self._push_params)
        self._push_params()
        self.reset()                      # ti.materialize_callback(self.reset), mltpath.py:21

    def _push_params(self):
        ctx().call('mpt_mlt_set_param', C.c_float(self.LSP[None]), C.c_float(self.Sigma[None]))

    def reset(self):
        '''mltpath.py:31-37: every X_old[i, j] = random(), L_old = 0 (draws of self.seed's reset stream)'''
        ctx().call('mpt_mlt_reset', self.nchains, C.c_uint32(self.seed))

    def render(self, iterations=1):
        '''mltpath.py:85-87, `iterations` times, asynchronously.  Consecutive calls are fused into one launch at the next
        read-back'''
        ctx().call('mpt_mlt_render', int(iterations))

    # test doors (include/miptina.h)
    def get_state(self):
        X = np.empty((self.nchains, 32), np.float32)
        L = np.empty((self.nchains, 3), np.float32)
        it = C.c_int(0)
        ctx().call('mpt_mlt_get_state', _f(X), _f(L), C.byref(it))
        return X, L, it.value

    def set_state(self, X, L, iteration=0):
        X = np.ascontiguousarray(X, np.float32).reshape(self.nchains, 32)
        L = np.ascontiguousarray(L, np.float32).reshape(self.nchains, 3)
        ctx().call('mpt_mlt_set_state', _f(X), _f(L), int(iteration))


def mlt_trace(X):
    '''camera + path_trace of given [n][32] vectors by the context's build (test door mpt_mlt_trace): [n][3]'''
    X = np.ascontiguousarray(X, np.float32).reshape(-1, 32)
    out = np.empty((X.shape[0], 3), np.float32)
    ctx().call('mpt_mlt_trace', _f(X), _f(out), int(X.shape[0]))
    return out


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))

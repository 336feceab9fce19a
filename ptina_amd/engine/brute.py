'''
brute-force integrator (reference engine/brute.py: "should be used for testing only"): the walk of
path_trace with no light sampling and no MIS -- a light is found only when a bounce ray hits it -- one
random3 per bounce, one sample per pixel and frame into film pass 0 with weight 1, on the Sobol sampler
PathEngine and PreviewEngine advance.  The kernel is csrc/brute_kernel.hip.

Unlike PathEngine.render, the frames are launched at the call; frames of this engine, of PathEngine and
Metropolis iterations add to the film in call order.
'''

from . import *                       # noqa: F401,F403
from ..sampling import *              # noqa: F401,F403  (the reference star-imports ptina.sampling and .sobol)
from ..sampling.sobol import *        # noqa: F401,F403
from ..common import Singleton, register, ctx, np
from ..sampling.sobol import SobolSampler


@register
class BruteEngine(metaclass=Singleton):
    def __init__(self):
        SobolSampler()

    def render(self, nframes=1):
        '''brute.py:24-26, `nframes` times'''
        ctx().call('mpt_render_brute', int(nframes))

    def render_until(self, noise, max_spp, min_spp=16, fraction=0.0):
        '''render until the film's noise estimate passes `noise` or `max_spp` frames are spent (engine.render_until)'''
        return render_until(self, noise, max_spp, min_spp, fraction)

    def kernel_time(self):
        '''(milliseconds, launches) of the brute kernels since the last call (HIP events)'''
        return ctx().timer('mpt_brute_kernel_time')

'''
unidirectional path integrator (reference engine/path.py).  path_trace / do_render
(path.py:18-93) are the render megakernel in csrc/render_kernel.hip.
'''

from . import *                       # noqa: F401,F403
from ..common import Singleton, register, ctx, np
from ..sampling import *              # noqa: F401,F403
from ..sampling.sobol import *        # noqa: F401,F403
from ..sampling.sobol import SobolSampler


@register
class PathEngine(metaclass=Singleton):
    def __init__(self):
        SobolSampler()
        self._film_cls = None

    def render(self, nframes=1):
        '''reference path.py:75-77: one Sobol update + one sample per pixel, asynchronously.
        Consecutive calls are fused into one launch at the next read-back.'''
        if self._film_cls is None:
            from ..filmtable import FilmTable
            self._film_cls = FilmTable
        self._film_cls()._hint()          # (where get_image() will want the image: a launch may write it while it drains)
        ctx().call('mpt_render', int(nframes))

    def render_until(self, noise, max_spp, min_spp=16, fraction=0.0):
        '''render until the film's noise estimate passes `noise` or `max_spp` frames are spent (engine.render_until)'''
        return render_until(self, noise, max_spp, min_spp, fraction)

    def render_selected(self, nframes=1, remark=False):
        '''nframes samples for the pixels of the film's selection only (FilmTable.select / set_selection; mpt_render_selected): the
        same path as render(), traced by the list kernel (csrc/adapt_kernel.hip), launched at the call.  remark=True first moves the
        mark of the listed pixels to their film as it is, so that this call's samples are their second group'''
        ctx().call('mpt_render_selected', int(nframes), 1 if remark else 0)

    def render_adaptive(self, noise, max_spp, min_spp=16, fraction=0.0, dilate=1, switch=None):
        '''render until every pixel's noise estimate passes `noise`, sampling only the pixels that have not (engine.render_adaptive)'''
        return render_adaptive(self, noise, max_spp, min_spp, fraction, dilate, switch)

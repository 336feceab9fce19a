'''
integrators (reference engine/__init__.py:5-13 is the star-import hub every integrator pulls
its scene singletons from)
'''

from ..camera import *                # noqa: F401,F403
from ..model import *                 # noqa: F401,F403
from ..light import *                 # noqa: F401,F403
from ..light.world import *           # noqa: F401,F403
from ..filmtable import *             # noqa: F401,F403
from ..mtllib import *                # noqa: F401,F403
from ..stack import *                 # noqa: F401,F403
from ..tree import *                  # noqa: F401,F403
from ..image import *                 # noqa: F401,F403


from collections import namedtuple as _namedtuple

RenderUntil = _namedtuple('RenderUntil', 'spp converged history')


def render_until(engine, noise, max_spp, min_spp=16, fraction=0.0, film=None, keep_mark=False):
    '''render with `engine` (PathEngine, BruteEngine: one sample per pixel and frame) until the film's noise estimate passes
    (FilmTable.get_noise) or `max_spp` frames are spent, on a doubling schedule: `min_spp` frames and a mark; then, per check, as
    many frames again as the film holds -- capped so that the total never exceeds `max_spp` -- and get_noise(noise, remark=True).
    It stops at the first check with above <= fraction * valid, or with the total at `max_spp`.

    Returns RenderUntil(spp, converged, history): the frames rendered, whether the last check passed, and [(spp, NoiseResult)] per
    check.  The loop counts the frames itself and expects a cleared film (FilmTable.clear()): then every check but a capped last
    one compares two equal halves -- the first spp / 2 samples against the second -- for which the estimate is exactly Cycles'
    criterion and `noise` its noise threshold; a capped last check compares unequal groups by the general form (the factor k of
    include/miptina.h).  One kernel pass and 32 bytes over PCIe per check.  `film`: the film table (default FilmTable()).

    keep_mark=True (here and in worker.render_until; the engines' methods keep their four arguments): the checks leave the mark alone (get_noise(noise, remark=False)) and mark() is called only when the loop goes on,
    so at return the mark still holds the first group of the last comparison and FilmTable.get_denoised(variance=...) works at once.
    Same film, spp and history; one device copy of pass 0 more per check that does not end the loop'''
    noise, max_spp, min_spp, fraction = float(noise), int(max_spp), int(min_spp), float(fraction)
    if min_spp < 1:
        raise ValueError('render_until: min_spp must be at least 1, got %d' % min_spp)
    if max_spp < 2 * min_spp:
        raise ValueError('render_until: max_spp must be at least 2 * min_spp = %d (one check), got %d' % (2 * min_spp, max_spp))
    if film is None:
        film = FilmTable()                    # noqa: F405
    engine.render(min_spp)
    film.mark()
    spp, history = min_spp, []
    while True:
        frames = min(spp, max_spp - spp)
        engine.render(frames)
        spp += frames
        stats = film.get_noise(noise, remark=not keep_mark)
        history.append((spp, stats))
        converged = stats.above <= fraction * stats.valid
        if converged or spp >= max_spp:
            return RenderUntil(spp, converged, history)
        if keep_mark:
            film.mark()

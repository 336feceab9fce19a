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


RenderAdaptive = _namedtuple('RenderAdaptive', 'spp converged history samples')

# The share of active pixels above which a pass over the whole film by the production kernels is cheaper than a list pass: the
# list kernel's samples/s over the PathEngine's with every pixel listed, rounded down to a multiple of 0.05.  Measured
# (tools/adaptive_bench.py, MI355X, s978 512x512 x 32 frames): 593 against 3827 Msamples/s, 0.155
DEFAULT_SWITCH = 0.15


def render_adaptive(engine, noise, max_spp, min_spp=16, fraction=0.0, dilate=1, switch=None, film=None):
    '''adaptive sampling: render_until's doubling schedule, but a pixel stops being sampled once its own estimate has passed -- what
    Blender's "noise threshold" means (Cycles stops each pixel once it passes).  With `engine` a PathEngine, on a cleared film:
      1. engine.render(min_spp), film.mark(), engine.render(min_spp); level = 2 * min_spp
      2. stats, active = film.select(noise, dilate)     (FilmTable.select: the pixels still above `noise`, and with dilate=1 their
                                                          neighbours, listed on the device)
      3. stop, converged, when stats.above <= fraction * stats.valid; stop, not converged, when level >= max_spp
      4. frames = min(level, max_spp - level)
      5. active > switch * valid: a FULL pass, film.mark() and engine.render(frames) -- the production kernels, faster per sample,
         and every pixel is re-marked
      6. otherwise a LIST pass: engine.render_selected(frames, remark=True) -- only the listed pixels are sampled and re-marked
      7. level += frames; back to 2.
    `switch` in [0, 1] (default DEFAULT_SWITCH): 0 = always full passes, which is render_until's loop; 1 = always list passes.

    Returns RenderAdaptive(spp, converged, history, samples): spp = the level reached, the most samples any pixel can hold;
    history = [(level, NoiseResult, active, kind)] per check, kind = 'full' or 'list', the pass that brought the film to that level
    (the first check follows step 1: 'full'); samples = the samples taken in all, a Python int (render_until would have taken
    spp * valid).  FilmTable.get_samples() shows where they went.  The pixels of the last pass keep a mark with samples since, and
    so do the pixels that stopped earlier: FilmTable.get_denoised(variance=...) works at once on return.

    What adaptive sampling is known to do:
      - the stopping rule makes the estimate slightly biased, as in Cycles: a pixel stops when its two groups happen to agree, so
        the pixels that stop early are, on average, a little too sure of a value a little off;
      - min_spp guards against a pixel whose two tiny groups agree by chance: on the CPU oracle's films min_spp=2, dilate=0 lets
        15 % of the pixels of the 34-triangle scene stop at 4 samples -- hence the defaults 16 and 1;
      - a pixel listed only because of dilation is compared in unequal groups (what its mark holds against the pass just added);
        the estimate's factor k (include/miptina.h) covers that.
    MLTPathEngine and BruteEngine have no such loop: the list kernel traces the PathEngine's path.'''
    noise, max_spp, min_spp, fraction, dilate = float(noise), int(max_spp), int(min_spp), float(fraction), int(dilate)
    switch = DEFAULT_SWITCH if switch is None else float(switch)
    if min_spp < 1:
        raise ValueError('render_adaptive: min_spp must be at least 1, got %d' % min_spp)
    if max_spp < 2 * min_spp:
        raise ValueError('render_adaptive: max_spp must be at least 2 * min_spp = %d (one check), got %d' % (2 * min_spp, max_spp))
    if not 0.0 <= switch <= 1.0:
        raise ValueError('render_adaptive: switch must be in [0, 1], got %r' % switch)
    if dilate not in (0, 1):
        raise ValueError('render_adaptive: dilate must be 0 or 1, got %d' % dilate)
    if film is None:
        film = FilmTable()                    # noqa: F405
    engine.render(min_spp)
    film.mark()
    engine.render(min_spp)
    level, history, samples, kind = 2 * min_spp, [], None, 'full'
    while True:
        stats, active = film.select(noise, dilate)
        if samples is None:
            samples = level * stats.valid         # (step 1 sampled every pixel of this context's share: the valid ones)
        history.append((level, stats, active, kind))
        converged = stats.above <= fraction * stats.valid
        if converged or level >= max_spp:
            return RenderAdaptive(level, converged, history, samples)
        frames = min(level, max_spp - level)
        if active > switch * stats.valid:
            kind = 'full'
            film.mark()
            engine.render(frames)
            samples += frames * stats.valid
        else:
            kind = 'list'
            engine.render_selected(frames, remark=True)
            samples += frames * active
        level += frames

'''
numpy restatement of adaptive sampling (include/miptina.h, mpt_adapt_select / mpt_render_selected) on top
of noise_ref.noise_map: which pixels a selection lists, in which order the device lists them, and engine.render_adaptive's loop on
per-frame radiances.  tests/test_adaptive_cpu.py holds this file to brute-force loops and to the CPU oracle's films;
tests/test_adaptive_gpu.py holds the GPU to it.
'''

import collections

import numpy as np

from noise_ref import noise_map, noise_stats, f32

TILE = 16           # MPT_TILE: one workgroup of the selection covers one TILE x TILE tile of the whole film


def masks(F, M, nx, ny, threshold, dilate):
    '''(active, above, valid) [nx, ny] bool of the accumulators F and M [nx*ny][4]: above = valid and e > threshold (f32, >);
    active = valid and (above or, with dilate = 1, a pixel of the 3x3 neighbourhood inside the film is above)'''
    assert dilate in (0, 1)
    e, valid = noise_map(F, M)
    valid = valid.reshape(nx, ny)
    above = valid & (e.reshape(nx, ny) > f32(threshold))
    near = above.copy()
    if dilate:
        pad = np.zeros((nx + 2, ny + 2), bool)                 # (a rim of "not above": the film's edges do not wrap around)
        pad[1:-1, 1:-1] = above
        for di in (0, 1, 2):
            for dj in (0, 1, 2):
                near |= pad[di:di + nx, dj:dj + ny]
    return valid & near, above, valid


def select(F, M, nx, ny, threshold, dilate):
    '''the film indices i * ny + j of the active pixels, ascending'''
    return np.flatnonzero(masks(F, M, nx, ny, threshold, dilate)[0].ravel()).astype(np.int32)


def device_order(pix, ny):
    '''the film indices `pix` in the order the device lists them: by TILE x TILE tile of the whole film, tile (ti, tj) before
    (ti, tj + 1) before (ti + 1, 0) -- the workgroups -- and within a tile by i - TILE ti, then j -- the lanes'''
    pix = np.asarray(pix, np.int64)
    i, j = pix // ny, pix % ny
    return pix[np.lexsort((j % TILE, i % TILE, j // TILE, i // TILE))].astype(np.int32)


def select_ordered(F, M, nx, ny, threshold, dilate):
    '''the list as mpt_adapt_select and mpt_adapt_eval leave it'''
    return device_order(select(F, M, nx, ny, threshold, dilate), ny)


Loop = collections.namedtuple('Loop', 'film mark history samples spp converged lists')


def run_loop(R, nx, ny, noise, max_spp, min_spp=16, fraction=0.0, dilate=1, switch=0.15):
    '''engine.render_adaptive on the per-frame radiances R[f][nx*ny][4] (frame f's raw one-sample film: what frame f adds to every
    pixel it samples; the sampler advances by every frame of every pass, so frame f is frame f whoever renders it).  The film is
    summed in f32, one add per frame in frame order.  Returns Loop(film, mark, history, samples, spp, converged, lists): history =
    [(level, valid, above, active, kind)] per check, lists = the ascending selection of every check'''
    R = np.asarray(R, f32)
    assert R.shape[1:] == (nx * ny, 4) and R.shape[0] >= max_spp and max_spp >= 2 * min_spp and min_spp >= 1
    film = np.zeros((nx * ny, 4), f32)
    for f in range(min_spp):
        film += R[f]
    mark = film.copy()
    for f in range(min_spp, 2 * min_spp):
        film += R[f]
    level, history, lists, samples, kind = 2 * min_spp, [], [], None, 'full'
    while True:
        e, valid = noise_map(film, mark)
        st = noise_stats(e, valid, noise)
        L = select(film, mark, nx, ny, noise, dilate)
        if samples is None:
            samples = level * st.valid
        history.append((level, st.valid, st.above, int(L.size), kind))
        lists.append(L)
        converged = st.above <= fraction * st.valid
        if converged or level >= max_spp:
            return Loop(film, mark, history, samples, level, converged, lists)
        frames = min(level, max_spp - level)
        if L.size > switch * st.valid:
            kind = 'full'
            mark = film.copy()
            for f in range(level, level + frames):
                film += R[f]
            samples += frames * st.valid
        else:
            kind = 'list'
            mark[L] = film[L]
            for f in range(level, level + frames):
                film[L] += R[f][L]
            samples += frames * int(L.size)
        level += frames

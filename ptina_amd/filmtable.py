'''
film that records the rendering result (reference filmtable.py): float4 per pixel and pass,
element x*ny + y, rgb sums + sample count in w.
'''

from .common import *                 # noqa: F401,F403
from .common import Singleton, register, ctx, np
from ._lib import fptr, host_array
import ctypes as C


@register
class FilmTable(metaclass=Singleton):
    def __init__(self, size=2**21, count=3):
        self.size = size
        self.count = count
        self._next = None             # the array the next get_image(0) will return, already known to the library (_hint)
        self._size = None
        self.last_exposure = None     # the exposure the last get_display used (metered, or the one given)

    def _res(self):
        # (the size only changes through set_size below: remembered, so that render() / get_image() do not ask the library twice a step)
        if self._size is None:
            nx, ny = C.c_int(0), C.c_int(0)
            ctx().call('mpt_get_size', C.byref(nx), C.byref(ny))
            self._size = (nx.value, ny.value)
        return self._size

    @property
    def nx(self):
        return self._res()[0]

    @property
    def ny(self):
        return self._res()[1]

    def set_size(self, nx, ny):
        ctx().call('mpt_set_size', int(nx), int(ny))
        self._size = (int(nx), int(ny))

    def clear(self, id=0):
        '''zeroes every pass whatever `id` says, as the reference does (filmtable.py:44-45)'''
        ctx().call('mpt_clear', int(id))

    def _hint(self):
        '''called by PathEngine.render() before it enqueues frames: allocate the array the next get_image(0) will return and tell
        the library (mpt_hint_image), so that a render launch can write the resolved image while it drains.  The reference
        allocates that array inside get_image (filmtable.py:48); it is the same fresh array, made a little earlier'''
        shape = self._res() + (4,)
        if self._next is None or self._next.shape != shape:
            if self._next is not None:
                ctx().call('mpt_hint_image', 0, None)       # (waits for a launch that may be writing into the old one)
            self._next = host_array(shape)
            ctx().call('mpt_hint_image', 0, fptr(self._next))

    def get_image(self, id=0):
        '''reference filmtable.py:47-63: [nx, ny, 4] f32, rgb / w, w -> 1; empty -> (.9,.4,.9,0)'''
        nx, ny = self._res()
        arr = None
        if int(id) == 0 and self._next is not None:
            arr, self._next = self._next, None               # (the hint is spent by the call below)
            if arr.shape != (nx, ny, 4):
                ctx().call('mpt_hint_image', 0, None)
                arr = None
        if arr is None:
            arr = host_array((nx, ny, 4))      # a fresh array, as in the reference; page-locked -> one DMA
        try:
            ctx().call('mpt_get_image', int(id), fptr(arr))
        except Exception:
            # the call may have failed before the library let go of the hinted address (a flush that fails): `arr` is about to be
            # dropped and its page-locked buffer recycled for another array of the same size, so the library must forget it first
            # (mpt_hint_image(None) also waits for a launch that may still be writing into it)
            try:
                ctx().call('mpt_hint_image', 0, None)
            except Exception:
                pass
            raise
        return arr

    def get_denoised(self, *denoise_args, variance=None, **denoise_kw):
        '''pass 0 filtered on the device by the edge-avoiding A-Trous wavelet, guided by the albedo and normal passes the
        PreviewEngine renders (mpt_get_denoised, include/miptina.h): [nx, ny, 4] f32 like get_image, a fresh array.  The arguments
        and their defaults are _lib.denoise_params': iterations, sigma_color, sigma_albedo, sigma_normal, demodulate.
        variance=sigma (4 is a good start) guides the colour tolerance by every pixel's own standard error instead of sigma_color:
        it needs a mark() with samples rendered since (render_until(..., keep_mark=True) leaves one); None = the fixed filter.  No
        reference counterpart: its add-on hands the Albedo pass to Blender's denoiser'''
        from ._lib import denoise_params
        nx, ny = self._res()
        ctx().set_denoise_variance(variance)
        arr = host_array((nx, ny, 4))
        ctx().call('mpt_get_denoised', C.byref(denoise_params(*denoise_args, **denoise_kw)), fptr(arr))
        return arr

    def denoise_kernel_time(self):
        '''(ms, calls): HIP-event time of the filter's kernels in the get_denoised calls since the last call'''
        return ctx().timer('mpt_denoise_kernel_time')

    def get_display(self, id=0, denoised=False, op='aces', transfer='srgb', layout='film', dither=True, exposure=None, key=0.18,
                    white=4.0, gamma=2.2, variance=None, **denoise_kw):
        '''film pass `id` -- or, with denoised=True, pass 0 through get_denoised's filter (its keywords in denoise_kw, and variance) -- as a screen
        or a PNG wants it: metered (exposure=None: log-average luminance to `key`) or exposed by `exposure`, tone-mapped (op: 'linear',
        'ptina', 'reinhard', 'aces'), transfer-encoded ('srgb', or 'gamma' with `gamma`), ordered-dithered and quantised on the device
        (mpt_get_display, include/miptina.h).  A fresh page-locked uint8 array: [nx, ny, 4] for layout='film' (indexed like
        get_image), [ny, nx, 4] with rows top-down for layout='display' (what image.write_png takes).  The exposure used is kept as
        last_exposure.  No reference counterpart: its scripts show linear radiance (ptina/wip/tonemapping.py was never wired in)'''
        from ._lib import denoise_params, display_params, DISPLAY_DENOISED, LAYOUTS
        nx, ny = self._res()
        if not denoised and int(id) < 0:
            raise RuntimeError('display: film pass %d out of range' % int(id))
        p = display_params(DISPLAY_DENOISED if denoised else id, op, transfer, layout, dither, exposure, key, white, gamma)
        dn = None
        if denoised:
            dn = C.byref(denoise_params(who='get_display', **denoise_kw))
            ctx().set_denoise_variance(variance)
        elif denoise_kw or variance is not None:
            raise TypeError('get_display: %s only apply with denoised=True' % sorted(list(denoise_kw) + ['variance'] * (variance is not None)))
        arr = host_array((ny, nx, 4) if p.layout == LAYOUTS['display'] else (nx, ny, 4), np.uint8)
        used = C.c_float(0)
        ctx().call('mpt_get_display', C.byref(p), dn, arr.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(used))
        self.last_exposure = float(used.value)
        return arr

    def display_kernel_time(self):
        '''(ms, calls): HIP-event time of the kernels of the get_display calls since the last call'''
        return ctx().timer('mpt_display_kernel_time')

    def mark(self):
        '''remember pass 0 as it is now, on the device (mpt_film_mark): the samples rendered from here on are the second group
        get_noise() compares with the first.  clear() and set_size() drop the mark'''
        ctx().call('mpt_film_mark')

    def get_noise(self, threshold, map=False, remark=False):
        '''how noisy pass 0 still is, estimated on the device from the film and the mark (mpt_get_noise, include/miptina.h): per
        pixel e = the standard error of the mean from the two groups of samples, relative to the brightness -- Cycles' adaptive
        sampling criterion when the groups are equal halves, so `threshold` is Blender's noise threshold.  Returns a NoiseResult:
        valid, above (pixels with e > threshold), mean, max, fraction and, with map=True, map [nx, ny] f32 (0 where not valid).
        remark=True also moves the mark to the film as it is now, in the same pass.  Only the statistics cross PCIe unless the
        map is asked for.  No reference counterpart'''
        from ._lib import NoiseStats, NoiseResult
        nx, ny = self._res()
        e = host_array((nx, ny)) if map else None
        st = NoiseStats()
        ctx().call('mpt_get_noise', float(threshold), 1 if remark else 0, None if e is None else fptr(e), C.byref(st))
        return NoiseResult(st, e)

    def get_mark(self):
        '''test door (mpt_get_mark): the mark's raw accumulators [nx*ny, 4], like get_raw'''
        nx, ny = self._res()
        arr = np.empty((nx * ny, 4), np.float32)
        ctx().call('mpt_get_mark', fptr(arr))
        return arr

    def noise_kernel_time(self):
        '''(ms, calls): HIP-event time of the kernels of the get_noise calls since the last call'''
        return ctx().timer('mpt_noise_kernel_time')

    def select(self, noise, dilate=1):
        '''adaptive sampling's selection (mpt_adapt_select, include/miptina.h): the pixels of pass 0 that still need samples, from
        the film and the mark, kept on the device as THE SELECTION for PathEngine.render_selected.  A pixel is above when it is
        valid and its estimate e > noise; it is active -- listed -- when it is valid and above or, with dilate=1 (Cycles' filter), a
        neighbour of an above pixel.  Pixels without samples on both sides of the mark (columns another GPU renders) are never
        listed.  Returns (NoiseResult, count): exactly get_noise(noise)'s statistics, and the length of the list.  Only those 40
        bytes cross PCIe.  clear() and set_size() drop the selection.  No reference counterpart'''
        from ._lib import NoiseStats, NoiseResult
        st, n = NoiseStats(), C.c_int(0)
        ctx().call('mpt_adapt_select', float(noise), int(dilate), C.byref(st), C.byref(n))
        return NoiseResult(st), n.value

    def get_selection(self):
        '''the selection's film indices x*ny + y, int32[count], in the device's order: by 16x16 tile (tile rows along y first), within
        a tile by x, then y (mpt_adapt_get_list)'''
        n = C.c_int(0)
        ctx().call('mpt_adapt_get_list', None, 0, C.byref(n))
        out = np.empty(n.value, np.int32)
        if n.value:
            ctx().call('mpt_adapt_get_list', out.ctypes.data_as(C.POINTER(C.c_int32)), out.size, None)
        return out

    def set_selection(self, pixels):
        '''a selection from the host (mpt_adapt_set_list): a bool mask [nx, ny], or film indices x*ny + y, strictly ascending (so
        that no pixel is listed twice), inside the film and inside this context's slab or stripes -- a region, a user mask'''
        nx, ny = self._res()
        a = np.asarray(pixels)
        if a.dtype == np.bool_:
            if a.shape != (nx, ny):
                raise ValueError('set_selection: the mask is %s, the film (%d, %d)' % (a.shape, nx, ny))
            a = np.flatnonzero(a.ravel())
        if a.size and (a.min() < -2**31 or a.max() >= 2**31):
            raise ValueError('set_selection: an index does not fit 32 bits')
        a = np.ascontiguousarray(a.reshape(-1), np.int32)
        ctx().call('mpt_adapt_set_list', a.ctypes.data_as(C.POINTER(C.c_int32)), int(a.size))

    def get_samples(self):
        '''pass 0's sample weight per pixel, float32 [nx, ny]: after adaptive sampling, how many samples each pixel took'''
        nx, ny = self._res()
        return np.ascontiguousarray(self.get_raw(0)[:, 3]).reshape(nx, ny)

    def adapt_kernel_time(self):
        '''(select_ms, render_ms, calls): HIP-event time of the select() calls and of the render_selected() calls since the last call'''
        return ctx().timer('mpt_adapt_kernel_time', 2)

    # ---- reprojection (csrc/film_history.cpp; no reference counterpart: its add-on clears the film at
    #      every change of the view):   render ... -> keep_history() -> edit the scene / camera -> compose() -> tree.update() -> reproject() -> render ...
    def keep_history(self):
        '''remember the view as it stands, on the device (mpt_history_keep): the camera, the model's positions and what every
        pixel's centre ray sees.  Needs a tree built for the model as it stands.  Writes nothing a render reads'''
        ctx().call('mpt_history_keep')

    def reproject(self, max_history=32, depth_tol=0.02):
        '''after the camera and / or the model changed (and the tree was built or refitted for it): resample pass 0 into the new
        view on the device (mpt_history_reproject, include/miptina.h) -- every pixel takes the accumulators of the place where the
        surface point it sees now lay in the kept view, bilinearly from the taps that saw the same object at the expected distance
        (depth_tol, relative); pixels whose surface was hidden, off-screen or replaced start from zero.  A pixel's history counts
        for at most max_history samples (inf: all of it), so that new samples can outweigh the old view.  Passes 1 and 2 are
        cleared, the mark and the selection dropped, the sampler left alone; the history is spent.  Lighting that changed -- an
        edited light, the shadow of a moved object -- is not detected: it lags by at most max_history samples.  Returns a
        HistoryResult.  Raises, naming the cause and leaving the film alone, without a history, after a change of the film size or
        of the face count, with a stale tree or a bad parameter'''
        from ._lib import HistoryStats, HistoryResult, history_params
        st = HistoryStats()
        ctx().call('mpt_history_reproject', C.byref(history_params(max_history, depth_tol)), C.byref(st))
        return HistoryResult(st)

    def get_motion(self):
        '''the motion vectors of the last reproject(), as a compositor's vector pass: (vector [nx, ny, 2] f32 = where the pixel's
        surface point lay in the kept view minus where it is now, in pixels (0 where not valid); valid [nx, ny] bool: the point
        had a place in the kept view; static [nx, ny] bool: neither the camera nor its triangle moved)'''
        rec = self.get_motion_records()
        i, j = np.meshgrid(np.arange(rec.shape[0], dtype=np.float32), np.arange(rec.shape[1], dtype=np.float32), indexing='ij')
        valid = (rec['flags'] >= 0) & np.isfinite(rec['fx']) & np.isfinite(rec['fy'])
        vector = np.zeros(rec.shape + (2,), np.float32)
        vector[..., 0] = np.where(valid, rec['fx'] - i, 0)
        vector[..., 1] = np.where(valid, rec['fy'] - j, 0)
        from ._lib import MOTION_STATIC
        return vector, valid, valid & (rec['flags'] == MOTION_STATIC)

    def get_motion_records(self):
        '''the last reproject()'s records as the device holds them (mpt_history_get_motion): _lib.MOTION_DTYPE [nx, ny] of the
        film as it was kept -- cur_id, fx, fy, d_exp, flags'''
        from ._lib import MOTION_DTYPE
        rec = np.empty(self._res(), MOTION_DTYPE)
        ctx().call('mpt_history_get_motion', rec.ctypes.data_as(C.c_void_p))
        return rec

    def get_gbuffer(self):
        '''test door (mpt_history_get_gbuffer): the kept view's (face, id, depth), [nx, ny] int32, int32, f32'''
        from ._lib import iptr
        nx, ny = self._res()
        face, obj, depth = np.empty((nx, ny), np.int32), np.empty((nx, ny), np.int32), np.empty((nx, ny), np.float32)
        ctx().call('mpt_history_get_gbuffer', iptr(face), iptr(obj), fptr(depth))
        return face, obj, depth

    def drop_history(self):
        '''forget the kept view and release its device memory (mpt_history_drop)'''
        ctx().call('mpt_history_drop')

    def history_kernel_time(self):
        '''(keep_ms, reproject_ms, calls): HIP-event time of the keep_history() and of the reproject() calls since the last call'''
        return ctx().timer('mpt_history_kernel_time', 2)

    def fast_export_image(self, out, id=0):
        '''reference filmtable.py:66-79: flat RGB f32 at (y * nx + x) * 3 into the caller's buffer'''
        nx, ny = self._res()
        assert out.dtype == np.float32 and out.size >= nx * ny * 3 and out.flags['C_CONTIGUOUS']
        ctx().call('mpt_fast_export_image', int(id), fptr(out))

    def get_raw(self, id=0):
        nx, ny = self._res()
        arr = np.empty((nx * ny, 4), np.float32)
        ctx().call('mpt_get_film_raw', int(id), fptr(arr))
        return arr

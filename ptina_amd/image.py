'''
texture atlas (reference image.py + allocator.py).  Texels live in one float4 device array;
Image.__call__ / bilerp (image.py:137-148, common.py:183-192) are csrc/pt_device.h image_sample.
'''

from .common import *                 # noqa: F401,F403
from .common import Singleton, register, ctx, np
from ._lib import fptr
import ctypes as C


@register
class ImagePool(metaclass=Singleton):
    def __init__(self, size=2**22, count=2**6):
        self.size = size
        self.count = count
        self._shapes = []

    def _prepare(self, arr):
        '''reference image.py:69-82'''
        if isinstance(arr, str):
            from PIL import Image as PILImage
            arr = np.swapaxes(np.array(PILImage.open(arr)), 0, 1)[:, ::-1]
        arr = np.asarray(arr)
        if arr.dtype == np.uint8:
            arr = arr.astype(np.float32) / 255
        nx, ny = arr.shape[0], arr.shape[1]
        if len(arr.shape) == 2:
            arr = arr[:, :, None]
        if arr.shape[2] == 1:
            arr = np.stack([arr[:, :, 0]] * 3, axis=2)
        if arr.shape[2] == 3:
            arr = np.concatenate([arr, np.ones((nx, ny, 1))], axis=2)
        return np.ascontiguousarray(arr, np.float32)

    def load_one(self, arr):
        arr = self._prepare(arr)
        id = C.c_int(-1)
        ctx().call('mpt_load_image', fptr(arr), arr.shape[0], arr.shape[1], C.byref(id))
        self._shapes.append(arr.shape[:2])
        return id.value

    def load(self, images):
        '''reference image.py:90-94: reset both allocators, then load in order'''
        ctx().call('mpt_reset_images')
        self._shapes = []
        for arr in images:
            self.load_one(arr)

    def nx(self, id):
        return self._shapes[id][0]

    def ny(self, id):
        return self._shapes[id][1]


class Image:
    def __init__(self, id):
        self.id = id

    @classmethod
    def load(cls, arr):
        return cls(ImagePool().load_one(arr))

    @property
    def nx(self):
        return ImagePool().nx(self.id)

    @property
    def ny(self):
        return ImagePool().ny(self.id)


def write_png(path, rgba8):
    '''an 8-bit [rows, columns, 4] (RGBA) or [rows, columns, 3] (RGB) array, rows top-down -- FilmTable.get_display(layout='display')
    -- as a PNG file, with zlib and struct alone (ti.imwrite needs PIL)'''
    import struct
    import zlib
    a = np.ascontiguousarray(rgba8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('write_png takes a uint8 array shaped [rows, columns, 3 or 4], got %s %s' % (a.dtype, a.shape))
    rows, cols, ch = a.shape

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    lines = np.empty((rows, 1 + cols * ch), np.uint8)
    lines[:, 0] = 0                                      # filter type 0 (none) in front of every scanline
    lines[:, 1:] = a.reshape(rows, cols * ch)
    head = struct.pack('>IIBBBBB', cols, rows, 8, 6 if ch == 4 else 2, 0, 0, 0)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', head) + chunk(b'IDAT', zlib.compress(lines.tobytes(), 6)) + chunk(b'IEND', b''))

'''edge creases for ModelPool.add_subdivision: Blender states an edge crease between 0 and 1, the
subdivision states sharpness in levels'''

import numpy as np


def blender_crease(c):
    '''the sharpness of Blender's edge crease c (a number or an array of them): c * c * 10, and inf from 1 on -- the mapping of
    Blender's subdivision surface modifier onto OpenSubdiv's sharpness.  f32, as add_subdivision stores it'''
    c = np.asarray(c, np.float32)
    with np.errstate(invalid='ignore'):
        s = np.where(c >= 1, np.float32(np.inf), c * c * np.float32(10))
    return s.astype(np.float32) if s.ndim else np.float32(s)

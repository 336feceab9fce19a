'''
CPU tests of the brute-force engine's boundary (BruteEngine, ptina_amd/engine/brute.py; csrc/brute_kernel.hip): the C ABI
declares, exports and binds its calls, the reference's module name resolves and star-exports what the reference's module
does, and the fixture made from the reference's executed source (tests/golden/reference_brute.npz, generator
tests/golden/make_reference_brute_golden.py) is consistent with itself.
'''

import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'reference_brute.npz')

BRUTE_CALLS = ('mpt_render_brute', 'mpt_brute_kernel_time')


def test_header_and_ctypes_table_carry_the_brute_calls():
    from ptina_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'miptina.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(mpt_[a-z0-9_]+)\s*\(', src))
    for name in BRUTE_CALLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name


def test_library_exports_the_brute_calls():
    from ptina_amd import _lib
    lib = _lib.load_library()
    for name in BRUTE_CALLS:
        assert hasattr(lib, name), name


def test_reference_module_name_resolves_and_star_exports():
    import ptina  # noqa: F401
    import importlib
    m = importlib.import_module('ptina.engine.brute')
    import ptina_amd.engine.brute as real
    assert m is real
    ns = {}
    exec('from ptina.engine.brute import *', ns)           # the first line of the reference's exams/matball.py
    for name in ('BruteEngine', 'FilmTable', 'ModelPool', 'MaterialPool', 'ImagePool', 'BVHTree', 'Camera', 'LightPool',
                 'WorldLight', 'SobolSampler'):
        assert name in ns, name
    assert not hasattr(real.BruteEngine, 'get_rng')        # omitted, as in the other ports
    from ptina_amd.common import _singletons
    assert real.BruteEngine in _singletons                 # @register: common.reset_all drops it


def test_reference_brute_fixture_is_self_consistent():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import make_reference_path_golden as G
    z = np.load(GOLD)
    assert len(G.CASES) == 3
    for name, (_, nx, ny, spp) in G.CASES.items():
        for prec in ('f32', 'f64'):
            film = z[f'{prec}/{name}/film']
            assert [int(x) for x in z[f'{prec}/{name}/size']] == [nx, ny, spp]
            assert film.shape == (nx * ny, 4) and film.dtype == np.float64
            assert not np.isnan(film).any()
            assert np.all(film[:, 3] == spp)
            assert (film[:, :3] >= 0).all() and film[:, :3].sum() > 0
            assert int(z[f'{prec}/{name}/sobol_time']) == 64 + 1 + spp
        # the two precisions rendered the same picture
        a, b = z[f'f32/{name}/film'][:, :3], z[f'f64/{name}/film'][:, :3]
        assert abs(a.mean() - b.mean()) <= 1e-3 * b.mean()

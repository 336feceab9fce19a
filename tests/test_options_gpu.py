'''
The option door of a context on the device (mpt_set_option / mpt_get_option) held to tests/option_table.py: defaults, what is
accepted, stored and refused, the read-only keys, and which sets leave a built tree to be built again.  Scene s34, a 16 x 16 film.
'''

import numpy as np
import pytest

from ptina_amd import scenes
from option_table import OPTIONS, READ_ONLY, BUILD_PHASE_KEYS, RETIRED, UNKNOWN

pytestmark = pytest.mark.gpu


def _ctx():
    from ptina_amd.common import ctx
    return ctx()


def _get(key):
    return _ctx().get_option(key)


def _engine():
    from helpers import setup_engine
    return setup_engine(scenes.scene_s34(), 16, 16, mode='fast')


def test_defaults_accepted_and_refused_values(fresh):
    from ptina_amd.things import init_things
    init_things()
    c = _ctx()
    for key, row in OPTIONS.items():
        assert _get(key) == row['default'], key
    for key, row in OPTIONS.items():
        for given, stored in row['accepted'].items():
            c.set_option(key, given)
            assert _get(key) == stored, (key, given)
            for bad in row['refused']:
                with pytest.raises(RuntimeError, match='^%s must be ' % key):
                    c.set_option(key, bad)
                assert _get(key) == stored, (key, given, bad)
        c.set_option(key, row['default'])
    for key, row in OPTIONS.items():                         # no set has touched another key
        assert _get(key) == row['default'], key


def test_reserve_cus_is_bounded_by_the_device(fresh):
    from ptina_amd.things import init_things
    init_things()
    c = _ctx()
    n = _get('num_cus')
    assert n >= 2
    c.set_option('reserve_cus', n - 1)
    assert _get('reserve_cus') == n - 1
    for bad in (n, n + 1, -1):
        with pytest.raises(RuntimeError, match=r'^reserve_cus must be in 0\.\.%d$' % (n - 1)):
            c.set_option('reserve_cus', bad)
        assert _get('reserve_cus') == n - 1
    c.set_option('reserve_cus', 0)


def test_read_only_keys(fresh):
    from ptina_amd.things import FilmTable
    eng = _engine()
    c = _ctx()
    c.set_option('build_phases', 1)
    from ptina_amd.things import BVHTree
    BVHTree().build()
    eng.render()
    assert np.all(FilmTable().get_image()[..., 3] == 1.0)
    values = {key: _get(key) for key in READ_ONLY + BUILD_PHASE_KEYS}
    assert all(isinstance(v, int) for v in values.values())
    assert values['num_cus'] > 0 and values['clock_khz'] > 0 and values['nranks'] == 1 and values['rank'] == 0 and values['device'] == 0
    assert values['pending'] == 0 and values['launch_seq'] >= 1 and values['fast_depth'] > 0 and values['tree_depth'] > 0
    assert values['build_phase_us_5'] > 0 and values['build_phase_us_5'] >= values['build_phase_us_1']
    for key in READ_ONLY + BUILD_PHASE_KEYS + RETIRED + UNKNOWN:
        if key == 'launch_seq':
            continue
        with pytest.raises(RuntimeError, match="^unknown option '%s'$" % key):
            c.set_option(key, 0)
    for key in RETIRED + UNKNOWN:
        with pytest.raises(RuntimeError, match="^unknown option '%s'$" % key):
            _get(key)
    assert {key: _get(key) for key in READ_ONLY + BUILD_PHASE_KEYS} == values        # no refusal changed anything
    c.set_option('launch_seq', 7)
    assert _get('launch_seq') == 7
    with pytest.raises(RuntimeError, match='^launch_seq must be >= 0$'):
        c.set_option('launch_seq', -1)
    assert _get('launch_seq') == 7


def test_which_sets_invalidate_the_tree(fresh):
    from ptina_amd.things import BVHTree, FilmTable
    eng = _engine()
    c = _ctx()

    def renders():
        eng.render()
        return bool(np.all(FilmTable().get_image()[..., 3] > 0))

    def needs_a_build():
        with pytest.raises(RuntimeError, match='BVH not built'):
            eng.render()
        BVHTree().build()
        assert renders()

    assert renders()
    for key, row in OPTIONS.items():
        cur = _get(key)
        assert cur == row['default'], key
        if row['tree'] == 'never':
            c.set_option(key, cur)
            eng.render()                                     # (a refusal would be raised here: the readiness check is at the call)
        elif row['tree'] == 'change':
            c.set_option(key, cur)
            if key in ('gpu_build', 'wide_build'):
                c.set_option(key, 5)                         # another value given, the same value stored
            assert renders(), key
            other = next(v for v, s in row['accepted'].items() if s != cur)
            c.set_option(key, other)
            needs_a_build()
            c.set_option(key, cur)
            needs_a_build()
        else:
            c.set_option(key, cur)
            needs_a_build()
    assert renders()

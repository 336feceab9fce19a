'''
CPU test of the option table (ptina_amd/csrc/mpt_options.h): the one place mpt_set_option and mpt_get_option take every settable
option's key, default, domain, stored value, tree-invalidation rule and refusal from.  The header is plain C++17 with nothing of HIP;
the test compiles it into a scratch shared object behind a small shim and holds it, and the option comment of include/miptina.h,
to the restatement in tests/option_table.py.
'''

import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from option_table import OPTIONS, READ_ONLY, BUILD_PHASE_KEYS, RETIRED, UNKNOWN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ptina_amd', 'csrc')

OK, UNKNOWN_KEY, REFUSED = 0, 1, 2

SHIM = '''
#include "mpt_options.h"
#include <new>
extern "C" {
int t_status(int k) { const int v[3] = { MPT_OPT_OK, MPT_OPT_UNKNOWN, MPT_OPT_REFUSED }; return v[k]; }
int t_count(void) { return MPT_OPTION_COUNT; }
const char *t_key(int i) { return MPT_OPTION_TABLE[i].key; }
int t_size(void) { return (int)sizeof(MptOptions); }
void t_init(void *o) { new (o) MptOptions(); }
int t_set(void *o, const char *key, int value, char *msg, int msg_size, int *tree_invalid) {
    bool inv = false;
    const int r = mpt_option_set(*(MptOptions *)o, key, value, msg, (size_t)msg_size, &inv);
    *tree_invalid = inv;
    return r;
}
int t_get(const void *o, const char *key, int *value) { return mpt_option_get(*(const MptOptions *)o, key, value); }
}
'''


def host_cxx():
    return (os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
            or '/opt/rocm/lib/llvm/bin/clang++')


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp('mpt_options')
    src, so = str(d / 'shim.cpp'), str(d / 'shim.so')
    with open(src, 'w') as f:
        f.write(SHIM)
    subprocess.run([host_cxx(), '-std=c++17', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so], check=True)
    lib = C.CDLL(so)
    lib.t_key.restype = C.c_char_p
    lib.t_init.argtypes = [C.c_void_p]
    lib.t_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.t_get.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    assert [lib.t_status(k) for k in range(3)] == [OK, UNKNOWN_KEY, REFUSED]
    return lib


class Opts:
    '''one MptOptions in a buffer of this side, so that its bytes can be compared'''

    def __init__(self, lib):
        self.lib = lib
        self.buf = C.create_string_buffer(lib.t_size())
        lib.t_init(self.buf)

    def bytes(self):
        return self.buf.raw

    def set(self, key, value):
        '''(status, message, tree invalid)'''
        msg, inv = C.create_string_buffer(b'untouched', 256), C.c_int(-1)
        r = self.lib.t_set(self.buf, key.encode(), value, msg, len(msg), C.byref(inv))
        return r, msg.value.decode(), inv.value

    def get(self, key):
        '''(status, value)'''
        v = C.c_int(-12345)
        r = self.lib.t_get(self.buf, key.encode(), C.byref(v))
        return r, v.value


def test_the_table_has_the_restatements_keys_once_each(lib):
    keys = [lib.t_key(i).decode() for i in range(lib.t_count())]
    assert len(keys) == len(set(keys)), sorted(k for k in keys if keys.count(k) > 1)
    assert set(keys) == set(OPTIONS)
    assert not set(keys) & set(READ_ONLY) and not set(keys) & set(RETIRED)
    assert lib.t_size() == 4 * len(keys)                     # an int per row and nothing else


def test_defaults(lib):
    o = Opts(lib)
    for key, row in OPTIONS.items():
        assert o.get(key) == (OK, row['default']), key


@pytest.mark.parametrize('key', list(OPTIONS))
def test_accepted_values_are_stored_as_stated(lib, key):
    for given, stored in OPTIONS[key]['accepted'].items():
        o = Opts(lib)
        others = {k: o.get(k) for k in OPTIONS if k != key}
        r, msg, _ = o.set(key, given)
        assert (r, msg) == (OK, 'untouched'), (key, given, msg)
        assert o.get(key) == (OK, stored), (key, given)
        assert {k: o.get(k) for k in OPTIONS if k != key} == others, (key, given)


@pytest.mark.parametrize('key', list(OPTIONS))
def test_refused_values_leave_the_struct_untouched(lib, key):
    row = OPTIONS[key]
    for start in (row['default'], *row['accepted']):         # from the default and from every other accepted state
        o = Opts(lib)
        assert o.set(key, start)[0] == OK
        before = o.bytes()
        for bad in row['refused']:
            r, msg, inv = o.set(key, bad)
            assert r == REFUSED and inv == 0, (key, bad)
            assert msg.startswith(key + ' must be ') and len(msg) > len(key + ' must be '), (key, bad, msg)
            assert o.bytes() == before, (key, bad)


def test_refusals_spell_the_domain_out(lib):
    o = Opts(lib)
    assert o.set('mode', 2)[1] == 'mode must be 0 (fast) or 1 (strict)'
    assert o.set('batch', 65)[1] == 'batch must be in 1..64'
    assert o.set('pipe_depth', 1)[1] == 'pipe_depth must be 0 (auto) or 2..6'
    assert o.set('tile_h_shift', 4)[1] == 'tile_h_shift must be in 0..3'
    assert o.set('lds_block', 64)[1] == 'lds_block must be 0 (auto), 256, 512, 768 or 1024'
    assert o.set('sah_build', 2)[1] == 'sah_build must be -1 (auto), 0 (host) or 1 (device)'
    assert o.set('finalise', 3)[1] == 'finalise must be 0 (combine pass), 1 (tail finalisation) or 2 (the same without the early image: A/B)'
    assert o.set('sah_exact_max', 1)[1] == 'sah_exact_max must be >= 2'


@pytest.mark.parametrize('key', list(OPTIONS))
def test_tree_invalidation_follows_the_rule(lib, key):
    row = OPTIONS[key]
    for start, start_stored in row['accepted'].items():
        for given, stored in row['accepted'].items():
            o = Opts(lib)
            assert o.set(key, start)[0] == OK
            want = {'never': False, 'change': stored != start_stored, 'always': True}[row['tree']]
            assert o.set(key, given)[2] == int(want), (key, start, given)
    if row['tree'] != 'never':                               # the cases by name: the current value again, then another one
        o = Opts(lib)
        other = next(v for v, s in row['accepted'].items() if s != row['default'])
        assert o.set(key, row['default'])[2] == int(row['tree'] == 'always')
        assert o.set(key, other)[2] == 1
        assert o.set(key, other)[2] == int(row['tree'] == 'always')


def test_unknown_and_retired_keys(lib):
    o = Opts(lib)
    before = o.bytes()
    for key in UNKNOWN + RETIRED + READ_ONLY + BUILD_PHASE_KEYS:
        for value in (0, 1):
            r, msg, inv = o.set(key, value)
            assert (r, msg, inv) == (UNKNOWN_KEY, "unknown option '%s'" % key, 0), key
        assert o.get(key) == (UNKNOWN_KEY, -12345), key
    assert o.bytes() == before


def option_comment():
    '''the comment in front of mpt_set_option's declaration'''
    with open(os.path.join(ROOT, 'include', 'miptina.h')) as f:
        text = f.read()
    end = text.index('int mpt_set_option(')
    start = text.rindex('/*', 0, end)
    assert text.index('*/', start) < end and not text[text.index('*/', start) + 2:end].strip()
    return text[start:end]


def test_the_header_documents_every_key():
    doc = option_comment()
    quoted = re.findall(r'"([A-Za-z0-9_]+)"', doc)
    for key in list(OPTIONS) + list(READ_ONLY):
        assert key in quoted, key
    assert quoted.count('build_phase_us_N') == 1 and not any(k in quoted for k in BUILD_PHASE_KEYS)
    for key in RETIRED:
        assert key not in quoted, key
    # settable keys first, then the read-only ones; each has an entry of its own
    entries = re.findall(r'^ \*   "([A-Za-z0-9_]+)"', doc, re.M)
    assert sorted(entries) == sorted(set(OPTIONS) | set(READ_ONLY) | {'build_phase_us_N'}), sorted(set(entries) ^ (set(OPTIONS) | set(READ_ONLY) | {'build_phase_us_N'}))
    first_read_only = min(entries.index(k) for k in READ_ONLY if k != 'launch_seq')
    assert all(entries.index(k) < first_read_only for k in OPTIONS)

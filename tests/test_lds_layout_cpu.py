'''
CPU test of the LDS-resident kernels' layout, fit rule and the kernel choice (ptina_amd/csrc/lds_layout.h): the one place the host
(how many bytes a launch asks for, which kernel serves a scene) and the kernels (where each region starts) take them from.  The
header is plain C with no dependencies; the test compiles it into a scratch shared object behind a small shim and holds it to a
restatement written here, in bytes, from the documented layouts:

  binary nodes (render_kernel_lds):  (n-1) node records 72 B apart, the region padded to 16 | n triangles of 48 B |
      (default material's index + 1) material records of 96 B | one byte per triangle, padded to 16 | 2 KiB per stack level
  4-wide nodes (render_kernel_lds4): nwide node records of 112 B | (n+1) triangles of 48 B | (materials the model uses + 1)
      records of 96 B | one byte per triangle, padded to 16 | 2 KiB per stack level

A scene fits when that is at most a CU's 160 KiB and every id fits its field: binary -- leaf ids and node ids (byte offset / 8)
in an int16 stack, the default material's index in a byte; 4-wide -- a node's id is its record's LDS byte address and a leaf's
16 x slot + 1 in 16 bits, the default material's index (the number of materials the model uses) in a byte below 255.
'''

import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ptina_amd', 'csrc')

BUDGET = 160 * 1024
GATHER, LDS, WIDE, LDS4 = 0, 1, 2, 5          # the public "last_kernel" numbers (include/miptina.h); 3 and 4 are retired

SHIM = '''
#include "lds_layout.h"
int t_const(int k) {
    const int v[10] = { MPT_LDS_BUDGET, MPT_LDS_MAT_VEC4, MPT_LDS_NODE_STRIDE, MPT_LDS4_NODE_STRIDE, MPT_LDS_LEVEL_BYTES,
                        MPT_KERNEL_GATHER, MPT_KERNEL_LDS, MPT_KERNEL_WIDE, MPT_KERNEL_LDS4, (int)sizeof(MptKernelFacts) };
    return v[k];
}
static void put(MptLdsRegions r, int *out) { out[0] = r.nnode4; out[1] = r.ntri4; out[2] = r.nmat4; out[3] = r.nmtl4; }
void t_regions(int n, int default_mtl, int *out) { put(mpt_lds_regions(n, default_mtl), out); }
void t_regions4(int n, int nwide, int nmats, int *out) { put(mpt_lds4_regions(n, nwide, nmats), out); }
int t_bytes(const int *r, int levels) {
    MptLdsRegions x; x.nnode4 = r[0]; x.ntri4 = r[1]; x.nmat4 = r[2]; x.nmtl4 = r[3];
    return mpt_lds_launch_bytes(x, levels);
}
int t_fit(int n, int max_materials, int fast_depth) { return mpt_lds_fit_bytes(n, max_materials, fast_depth); }
int t_fit4(int n, int nwide, int wide_stack, int nmats) { return mpt_lds4_fit_bytes(n, nwide, wide_stack, nmats); }
int t_choose(int fast, int use_lds, int lds_wide, int use_wide, int nfaces, int wide_nodes, int wide_stack, int have_wnode,
             int max_mtlid, int max_materials, int fast_depth, int *lds_bytes) {
    MptKernelFacts f;
    f.fast = fast; f.use_lds = use_lds; f.lds_wide = lds_wide; f.use_wide = use_wide; f.nfaces = nfaces;
    f.wide_nodes = wide_nodes; f.wide_stack = wide_stack; f.have_wnode = have_wnode; f.max_mtlid = max_mtlid;
    f.max_materials = max_materials; f.fast_depth = fast_depth;
    MptKernelChoice ch = mpt_choose_kernel(&f);
    *lds_bytes = ch.lds_bytes;
    return ch.kernel;
}
int t_stack_levels(int depth) { return mpt_gather_stack_levels(depth); }
'''


@pytest.fixture(scope='module')
def lay(tmp_path_factory):
    d = tmp_path_factory.mktemp('lds_layout')
    src, so = str(d / 'shim.c'), str(d / 'shim.so')
    with open(src, 'w') as f:
        f.write(SHIM)
    cc = os.environ.get('CC') or shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or '/opt/rocm/lib/llvm/bin/clang'
    subprocess.run([cc, '-std=c99', '-O1', '-Wall', '-Werror', '-shared', '-fPIC', '-I', CSRC, src, '-o', so], check=True)
    lib = C.CDLL(so)
    lib.t_regions.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.t_regions4.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.t_bytes.argtypes = [C.c_void_p, C.c_int]
    lib.t_choose.argtypes = [C.c_int] * 11 + [C.c_void_p]
    return lib


# ------------------------------------------------------------------ the restatement, in bytes
def pad16(x):
    return (x + 15) // 16 * 16


def regions_py(n, default_mtl):
    '''binary nodes: bytes of the node, triangle, material and material-id regions'''
    return [pad16((n - 1) * 72), n * 48, (default_mtl + 1) * 96, pad16(n)]


def regions4_py(n, nwide, nmats):
    return [nwide * 112, (n + 1) * 48, (nmats + 1) * 96, pad16(n)]


def fit_py(n, max_materials, fast_depth):
    '''launch bytes of render_kernel_lds if it can serve the scene, else 0'''
    if n < 2:
        return 0
    if n >= 32768 or (n - 1) * 72 // 8 >= 32768:           # leaf slots and node ids (byte offset / 8) in an int16
        return 0
    if max_materials > 255:                                # the default material's index in a byte
        return 0
    total = sum(regions_py(n, max_materials)) + (fast_depth + 1) * 2048
    return total if total <= BUDGET else 0


def fit4_py(n, nwide, wide_stack, nmats):
    if n < 2 or nwide < 1 or wide_stack < 1:
        return 0
    if n >= 4095 or nwide * 112 >= 65536:                  # leaf ids 16 x slot + 1 (slot n: the unused slots' leaf) and node addresses in 16 bits
        return 0
    if nmats > 254:
        return 0
    total = sum(regions4_py(n, nwide, nmats)) + wide_stack * 2048
    return total if total <= BUDGET else 0


def choose_py(fast, use_lds, lds_wide, use_wide, nfaces, wide_nodes, wide_stack, have_wnode, max_mtlid, max_materials, fast_depth):
    if not fast:
        return GATHER, 0
    if use_lds and lds_wide and use_wide and have_wnode:
        b = fit4_py(nfaces, wide_nodes, wide_stack, max_mtlid + 1)
        if b:
            return LDS4, b
    if use_lds:
        b = fit_py(nfaces, max_materials, fast_depth)
        if b:
            return LDS, b
    if use_wide and wide_nodes > 0:
        return WIDE, 0
    return GATHER, 0


def regions(lib, n, default_mtl):
    out = (C.c_int * 4)()
    lib.t_regions(n, default_mtl, out)
    return list(out)


def regions4(lib, n, nwide, nmats):
    out = (C.c_int * 4)()
    lib.t_regions4(n, nwide, nmats, out)
    return list(out)


def choose(lib, *facts):
    b = C.c_int(-1)
    k = lib.t_choose(*facts, C.byref(b))
    return k, b.value


def boundary(fits, values):
    '''(last value that fits, first that does not) of a predicate that is true up to a point of `values` and false from there on'''
    flags = [bool(fits(v)) for v in values]
    assert flags[0] and not flags[-1], 'the sweep must start inside and end outside'
    first_out = flags.index(False)
    assert not any(flags[first_out:]), 'one boundary only'
    return values[first_out - 1], values[first_out]


# ------------------------------------------------------------------ tests
def test_constants(lay):
    assert [lay.t_const(k) for k in range(9)] == [BUDGET, 6, 72, 112, 2048, GATHER, LDS, WIDE, LDS4]
    assert lay.t_const(9) == 11 * 4                         # the facts of the choice: eleven ints, nothing hidden


def test_regions_match_the_documented_layout(lay):
    for n, mtl in itertools.product(list(range(2, 70)) + [255, 256, 257, 978, 1000, 1337, 4094], (0, 1, 3, 63, 64, 255)):
        r = regions(lay, n, mtl)
        assert [16 * x for x in r] == regions_py(n, mtl), (n, mtl)
        for levels in (1, 2, 21, 40):
            assert lay.t_bytes((C.c_int * 4)(*r), levels) == sum(regions_py(n, mtl)) + levels * 2048
    for n, nw, nm in itertools.product(list(range(2, 40)) + [978, 1000, 4094], (1, 2, 7, 330, 585), (0, 1, 4, 64, 254)):
        r = regions4(lay, n, nw, nm)
        assert [16 * x for x in r] == regions4_py(n, nw, nm), (n, nw, nm)
        for levels in (1, 17, 30):
            assert lay.t_bytes((C.c_int * 4)(*r), levels) == sum(regions4_py(n, nw, nm)) + levels * 2048


def test_fit_sweep_binary(lay):
    for mtl, depth in itertools.product((0, 3, 64, 255, 256, 1000), (0, 1, 10, 20, 31, 60, 78, 79, 80, 200)):
        for n in itertools.chain(range(0, 1500), range(3600, 3700), (4094, 4095, 32767, 32768, 32769, 100000)):
            assert lay.t_fit(n, mtl, depth) == fit_py(n, mtl, depth), (n, mtl, depth)


def test_fit_sweep_wide(lay):
    for nm, stack in itertools.product((0, 4, 64, 254, 255), (0, 1, 8, 24, 60, 79, 80, 81)):
        for nw in (0, 1, 2, 100, 330, 585, 586, 1000):
            for n in itertools.chain(range(0, 40), range(900, 1100, 7), range(3100, 3500, 13), (4094, 4095, 4096, 32768)):
                assert lay.t_fit4(n, nw, stack, nm) == fit4_py(n, nw, stack, nm), (n, nw, stack, nm)


def test_fit_boundaries_from_both_sides(lay):
    # binary kernel: the byte budget bounds n and the depth; the material count is bounded by its byte (256 records fit the budget)
    for mtl, depth in ((3, 20), (64, 10), (0, 0), (255, 31)):
        last, first = boundary(lambda n: fit_py(n, mtl, depth), list(range(2, 4000)))
        assert lay.t_fit(last, mtl, depth) == fit_py(last, mtl, depth) > 0 and lay.t_fit(first, mtl, depth) == 0, (mtl, depth, last, first)
    for n, mtl in ((2, 3), (500, 3), (978, 4), (1000, 64)):
        last, first = boundary(lambda d: fit_py(n, mtl, d), list(range(0, 200)))
        assert lay.t_fit(n, mtl, last) > 0 and lay.t_fit(n, mtl, first) == 0, (n, mtl, last, first)
    for n, depth in ((2, 0), (100, 5), (978, 10)):
        last, first = boundary(lambda m: fit_py(n, m, depth), list(range(0, 2000)))
        assert lay.t_fit(n, last, depth) > 0 and lay.t_fit(n, first, depth) == 0, (n, depth, last, first)
    assert boundary(lambda m: fit_py(2, m, 0), list(range(0, 2000))) == (255, 256)       # ... the byte, not the budget
    # 4-wide kernel: the budget bounds n and the stack; nwide by its 16-bit address (585 x 112 = 65520) or the budget; materials by the byte
    for nw, stack, nm in ((330, 17, 4), (1, 1, 0), (585, 3, 0), (100, 30, 254)):
        last, first = boundary(lambda n: fit4_py(n, nw, stack, nm), list(range(2, 5000)))
        assert lay.t_fit4(last, nw, stack, nm) > 0 and lay.t_fit4(first, nw, stack, nm) == 0, (nw, stack, nm, last, first)
    for n, stack, nm in ((2, 1, 0), (978, 17, 4), (1500, 8, 4)):
        last, first = boundary(lambda w: fit4_py(n, w, stack, nm), list(range(1, 2000)))
        assert lay.t_fit4(n, last, stack, nm) > 0 and lay.t_fit4(n, first, stack, nm) == 0, (n, stack, nm, last, first)
    assert boundary(lambda w: fit4_py(2, w, 1, 0), list(range(1, 2000))) == (585, 586)   # the 16-bit address
    for n, nw, nm in ((2, 1, 0), (978, 330, 4), (1500, 500, 4)):
        last, first = boundary(lambda s: fit4_py(n, nw, s, nm), list(range(1, 200)))
        assert lay.t_fit4(n, nw, last, nm) > 0 and lay.t_fit4(n, nw, first, nm) == 0, (n, nw, nm, last, first)
    for n, nw, stack in ((2, 1, 1), (978, 330, 17)):
        last, first = boundary(lambda m: fit4_py(n, nw, stack, m), list(range(0, 2000)))
        assert lay.t_fit4(n, nw, stack, last) > 0 and lay.t_fit4(n, nw, stack, first) == 0, (n, nw, stack, last, first)
    assert boundary(lambda m: fit4_py(2, 1, 1, m), list(range(0, 2000))) == (254, 255)


def test_gather_stack_levels(lay):
    '''the kernels that gather the binary tree keep the sentinel and one pending sibling per level: depth + 2 entries, in the
    32-level instantiation while they fit and in the 64-level one from depth 31 on (the deepest tree that one serves: 62)'''
    assert [lay.t_stack_levels(d) for d in (0, 30, 31, 62)] == [32, 32, 64, 64]
    for d in (0, 30, 31, 62):
        assert d + 2 <= lay.t_stack_levels(d)


def test_smallest_and_largest_face_counts(lay):
    assert lay.t_fit(0, 3, 0) == 0 and lay.t_fit(1, 3, 0) == 0                 # no tree without a node
    assert lay.t_fit(2, 3, 0) == fit_py(2, 3, 0) == 80 + 96 + 4 * 96 + 16 + 2048
    assert lay.t_fit4(0, 1, 1, 0) == 0 and lay.t_fit4(1, 1, 1, 0) == 0
    assert lay.t_fit4(2, 1, 1, 0) == fit4_py(2, 1, 1, 0) == 112 + 3 * 48 + 96 + 16 + 2048
    # the largest face count the API accepts: (n - 1) x 72 does not fit 32 bits; the rule must say "does not fit", not wrap into one that does
    big = (1 << 26) - 1
    for n in (big, big - 1, 29826162, 29826163, (1 << 31) - 1):                 # (29826162 x 72 is the first product past 2^31)
        assert lay.t_fit(n, 3, 10) == 0 and lay.t_fit4(n, 330, 17, 4) == 0 and lay.t_fit4(n, big, 17, 4) == 0, n
    assert choose(lay, 1, 1, 1, 1, big, big // 3, 40, 1, 3, 64, 30) == (WIDE, 0)
    assert choose(lay, 1, 1, 1, 0, big, big // 3, 40, 1, 3, 64, 30) == (GATHER, 0)


# (nfaces, wide_nodes, wide_stack, have_wnode, max_mtlid, max_materials, fast_depth)
SCENES = {
    'fits both': (978, 330, 17, 1, 3, 64, 14),
    'fits only the binary kernel (4-wide stack too deep)': (978, 330, 70, 1, 3, 64, 14),
    'fits only the 4-wide kernel (the default material beyond a byte)': (978, 330, 17, 1, 3, 1000, 14),
    'fits neither': (100000, 33000, 40, 1, 3, 64, 30),
    '4-wide tree not built': (978, 0, 0, 0, 3, 64, 14),
    '4-wide tree not built, too large for LDS': (100000, 0, 0, 0, 3, 64, 30),
}


def test_scenes_are_what_their_names_say():
    fits = {name: (bool(fit_py(s[0], s[5], s[6])), bool(fit4_py(s[0], s[1], s[2], s[4] + 1))) for name, s in SCENES.items()}
    assert list(fits.values()) == [(True, True), (True, False), (False, True), (False, False), (True, False), (False, False)]


@pytest.mark.parametrize('name', list(SCENES))
def test_kernel_choice_every_option_combination(lay, name):
    scene = SCENES[name]
    for fast, use_lds, lds_wide, use_wide in itertools.product((1, 0), repeat=4):
        got = choose(lay, fast, use_lds, lds_wide, use_wide, *scene)
        assert got == choose_py(fast, use_lds, lds_wide, use_wide, *scene), (name, fast, use_lds, lds_wide, use_wide)
        if not fast:
            assert got == (GATHER, 0)                        # the strict build has one kernel


def test_kernel_choice_by_hand(lay):
    both, only2, only4, neither, unbuilt = [SCENES[k] for k in list(SCENES)[:5]]
    b2, b4 = fit_py(978, 64, 14), fit4_py(978, 330, 17, 4)
    assert b2 > 0 and b4 > 0 and b2 != b4
    #                  fast lds lds_wide wide
    assert choose(lay, 1, 1, 1, 1, *both) == (LDS4, b4)
    assert choose(lay, 1, 1, 0, 1, *both) == (LDS, b2)       # option "lds_wide" = 0: the binary nodes
    assert choose(lay, 1, 1, 1, 0, *both) == (LDS, b2)       # option "wide" = 0 keeps every kernel off the 4-wide nodes
    assert choose(lay, 1, 0, 1, 1, *both) == (WIDE, 0)
    assert choose(lay, 1, 0, 1, 0, *both) == (GATHER, 0)
    assert choose(lay, 1, 1, 1, 1, *only2) == (LDS, b2)
    assert choose(lay, 1, 1, 1, 1, *only4) == (LDS4, b4)
    assert choose(lay, 1, 1, 0, 1, *only4) == (WIDE, 0)
    assert choose(lay, 1, 1, 1, 1, *neither) == (WIDE, 0)
    assert choose(lay, 1, 1, 1, 0, *neither) == (GATHER, 0)
    assert choose(lay, 1, 1, 1, 1, *unbuilt) == (LDS, b2)
    assert choose(lay, 1, 0, 1, 1, *unbuilt) == (GATHER, 0)  # no 4-wide nodes to gather either
    # the records of the 4-wide tree are not on the device (have_wnode = 0) although it was built: not the LDS copy of them
    assert choose(lay, 1, 1, 1, 1, 978, 330, 17, 0, 3, 64, 14) == (LDS, b2)

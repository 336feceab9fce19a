'''
tools/tree_rules_check.cpp for the tests: the host passes of the tree build (ptina_amd/csrc/tree_host.h on tree_rules.h) compiled
into a stand-alone program with the host compiler and run on a model's positions -- no GPU, no library, nothing loaded into the
interpreter.  Shared by tests/test_tree_rules_cpu.py (against recorded bytes and the numpy checkers) and
tests/test_tree_rules_gpu.py (against what the device passes leave).
'''

import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32


def compile_tool(folder):
    '''-> the program's path; plain -O2 -ffp-contract=off, as tests/test_record_checks_cpu.py compiles tri_records_check'''
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = os.path.join(str(folder), 'tree_rules_check')
    subprocess.run([cxx, '-std=c++17', '-O2', '-ffp-contract=off', '-pthread', os.path.join(ROOT, 'tools', 'tree_rules_check.cpp'), '-o', exe],
                   check=True, capture_output=True, text=True)
    return exe


def run_tool(exe, folder, pos, tree=1, sah_exact_max=8192):
    '''the host passes over positions [n][3][3] -> dict of child, leaf, mc, bmin, bmax (as BVHTree().to_numpy() gives them), depth,
    fast_depth, snode, fnode, wnode, qnode (uint32 words), nw, wide_depth, wide_stack'''
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3, 3)
    n = pos.shape[0]
    model, out = os.path.join(str(folder), 'model.bin'), os.path.join(str(folder), 'out.bin')
    with open(model, 'wb') as f:
        f.write(np.int32(n).tobytes() + pos.tobytes() + np.array([tree, sah_exact_max], np.int32).tobytes())
    subprocess.run([exe, model, out], check=True, capture_output=True)
    words = np.fromfile(out, U)
    head = words[:8].view(np.int32)
    assert head[0] == n and head[1] == max(n - 1, 0)
    ni, nw = int(head[1]), int(head[4])
    got = dict(depth=int(head[2]), fast_depth=int(head[3]), nw=nw, wide_depth=int(head[5]), wide_stack=int(head[6]))
    at = 8
    for name, shape, kind in (('child', (ni, 2), np.int32), ('leaf', (n,), np.int32), ('mc', (n,), np.int32), ('bmin', (ni, 3), F),
                              ('bmax', (ni, 3), F), ('snode', (ni, 2, 4), U), ('fnode', (ni, 4, 4), U), ('wnode', (nw, 8, 4), U),
                              ('qnode', (nw, 4, 4), U)):
        count = int(np.prod(shape))
        got[name] = words[at:at + count].view(kind).reshape(shape)
        at += count
    assert at == words.size, f'out.bin holds {words.size} words, its head accounts for {at}'
    return got


def coincident(count=8):
    '''`count` copies of one triangle: every centre, every Morton code equal -- the face index alone orders the keys'''
    tri = np.array([[0.25, 0.5, 0.75], [0.5, 0.25, 0.125], [0.375, 0.625, 0.5]], F)
    return np.repeat(tri[None], count, axis=0)


def flat(count=64, seed=64):
    '''`count` axis-aligned triangles in the plane z = 0.5, and among them groups that share a line x = const too: boxes of no
    extent along one and two axes, where the quantisation takes its "flat node still needs a positive step" branch'''
    rng = np.random.default_rng(seed)
    pos = np.zeros((count, 3, 3), F)
    corner = rng.uniform(0, 1, (count, 2)).astype(F)
    size = rng.uniform(0.01, 0.05, (count, 2)).astype(F)
    pos[:, :, 0] = corner[:, 0:1] + size[:, 0:1] * np.array([0, 1, 0], F)
    pos[:, :, 1] = corner[:, 1:2] + size[:, 1:2] * np.array([0, 0, 1], F)
    pos[:, :, 2] = F(0.5)
    pos[:8, :, 0] = F(0.25)                                  # eight of them degenerate to segments on the line x = 0.25, z = 0.5
    return pos

'''
The context options (mpt_set_option / mpt_get_option of include/miptina.h) restated as plain data: the one place the tests say what
every key defaults to, accepts, refuses, stores and does to a built tree.  tests/test_options_cpu.py holds the table of
ptina_amd/csrc/mpt_options.h and the header's comment to it, tests/test_options_gpu.py a context on the device.

Per settable key:
  default   what a new context reads
  accepted  {value given: value stored}, both ends of the domain among them
  refused   values just outside the domain
  tree      what a set does to a built tree: 'never' invalidates it, 'change' when the stored value changes, 'always'
'''

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
MAX_BATCH, MAX_PIPE = 64, 6


def _flag(default, tree='never'):
    '''any int is taken; non-zero is stored as 1'''
    return dict(default=default, accepted={0: 0, 1: 1, 2: 1, -1: 1, INT_MIN: 1, INT_MAX: 1}, refused=(), tree=tree)


def _ints(default, lo, hi, tree='never', also=()):
    '''lo..hi, stored as given'''
    inside = {lo, hi, default, *also}
    refused = tuple(v for v in (lo - 1, hi + 1, INT_MIN, INT_MAX) if INT_MIN <= v <= INT_MAX and not lo <= v <= hi)
    return dict(default=default, accepted={v: v for v in sorted(inside)}, refused=refused, tree=tree)


OPTIONS = {
    'mode': _ints(0, 0, 1),
    'batch': _ints(32, 1, MAX_BATCH, also=(2, 63)),
    'chunk': _ints(0, 0, INT_MAX, also=(1, 7)),
    'count': _flag(0),
    'timeline': _flag(0),
    'build_phases': _flag(0),
    'lane_hist': _flag(0),
    'lds': _flag(1),
    'zero_copy': _flag(1),
    'denoise_lds': _flag(1),
    'wide': _flag(1),
    'wide_quant': _flag(1),
    'lds_wide': _ints(1, 0, 1),
    'shade_spec': _ints(1, 0, 1),
    'skip_dark': _ints(-1, -1, 1, also=(0,)),
    'spin_us': _ints(20000, 0, INT_MAX, also=(1,)),
    'finalise': _ints(1, 0, 2),
    'pipe_depth': dict(default=0, accepted={v: v for v in (0, 2, 3, MAX_PIPE)}, refused=(-1, 1, MAX_PIPE + 1, INT_MIN, INT_MAX), tree='never'),
    'grid_div': _ints(0, 0, 8, also=(1,)),
    'lds_block': dict(default=0, accepted={v: v for v in (0, 256, 512, 768, 1024)},
                      refused=(-256, -1, 1, 64, 255, 257, 1023, 1025, 1280, 2048, INT_MIN, INT_MAX), tree='never'),
    # the upper end is the context's num_cus - 1 (tests/test_options_gpu.py); the table by itself has none
    'reserve_cus': dict(default=0, accepted={0: 0, 1: 1, 7: 7}, refused=(-1, INT_MIN), tree='never'),
    'tile_w_shift': _ints(3, 0, 3, also=(1,)),
    'tile_h_shift': _ints(3, 0, 3, also=(2,)),
    'tree': _ints(1, 0, 1, tree='change'),
    'sah_build': _ints(-1, -1, 1, tree='change', also=(0,)),
    'gpu_build': _flag(1, tree='change'),
    'wide_build': _flag(1, tree='change'),
    'sah_exact_max': _ints(8192, 2, INT_MAX, tree='always', also=(3, 32)),
    'sah_max': dict(default=1 << 22, accepted={v: v for v in (INT_MIN, -1, 0, 1, 1 << 22, INT_MAX)}, refused=(), tree='always'),
    'sah_inject_fail': _flag(0, tree='always'),
}

# what mpt_get_option reads and mpt_set_option does not know -- but for "launch_seq", state of the context that a test door sets
READ_ONLY = (
    'tree_depth', 'fast_depth', 'pending', 'last_finalised', 'launch_seq', 'tag_wraps', 'scene_feat', 'shade_inst',
    'cur_depth', 'cur_div', 'last_div', 'last_kernel', 'num_cus', 'sah_fallback',
    'sah_levels', 'sah_kelems', 'sah_chunks', 'sah_segments', 'sah_part_kwords', 'sah_tasks_small', 'sah_tasks_big',
    'sah_t_sort_k', 'sah_t_loop_k', 'sah_t_max_k', 'sah_task_levels', 'sah_task_levels_max',
    'wide_nodes', 'wide_stack', 'wide_ratio_permille', 'wide_depth',
    'nranks', 'rank', 'device', 'clock_khz', 'hw_queues',
)
BUILD_PHASE_KEYS = tuple('build_phase_us_%d' % k for k in range(6))       # one pattern of mpt_get_option; the header names the family once

RETIRED = ('pool', 'pool_shaders', 'wide8', 'node_soa')
UNKNOWN = ('', 'Mode', 'mode ', 'batch2', 'build_phase_us_', 'build_phase_us_6', 'build_phase_us_00', 'no_such_option')

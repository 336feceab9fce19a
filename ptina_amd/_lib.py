'''
ctypes binding of libmiptina.so (include/miptina.h) -- the only door between PTina's
Python object API and the gfx950 kernels.  There is NO CPU fallback: if the library is
missing or no MI355X is visible, every entry point raises.
'''

import ctypes as C
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MIPTINA_LIB: another build of the same library (A/B runs of compiler flags, tools/gpu_round.sh)
LIB_PATH = os.environ.get('MIPTINA_LIB') or os.path.join(HERE, 'libmiptina.so')

MODE_FAST, MODE_STRICT = 0, 1
LIGHT_TYPES = {'POINT': 1, 'AREA': 2}          # LightPool.TYPES, light/__init__.py:11


# kinds of mpt_unit_eval (include/miptina.h, enum MPT_UNIT_*): name -> (kind, input columns, output columns)
UNIT_KINDS = {
    'schlick': (0, 1, 1), 'dielectric': (1, 3, 1), 'gtr1': (2, 2, 1), 'gtr2': (3, 2, 1), 'smithggx': (4, 2, 1),
    'sample_gtr1': (5, 3, 3), 'sample_gtr2': (6, 3, 3), 'tanspace': (7, 6, 3), 'spherical': (8, 2, 3),
    'dir2tex': (9, 3, 2), 'reflect': (10, 6, 3), 'refract': (11, 7, 4), 'box': (12, 12, 3), 'face': (13, 30, 9),
    'sphere': (14, 10, 1), 'area': (15, 15, 4), 'disney_brdf': (16, 24, 3), 'disney_bounce': (17, 24, 7),
    'power_heuristic': (18, 2, 1), 'wanghash': (19, 1, 1), 'wanghash2': (20, 2, 1),
    # the kinds that read the context's scene (lights, images, materials, world light, camera)
    'light_hit': (21, 6, 6), 'light_sample': (22, 6, 8), 'image_sample': (23, 3, 4), 'world_at': (24, 3, 3),
    'material_get': (25, 3, 22), 'camera_generate': (26, 2, 6), 'face_side': (27, 14, 4),
    # Disney.brdf / .bounce as the plain and the plain + lean SHADE instantiate them (production build only)
    'disney_brdf_plain': (28, 24, 3), 'disney_bounce_plain': (29, 24, 7), 'disney_brdf_lean': (30, 24, 3), 'disney_bounce_lean': (31, 24, 7),
}


class Caps(C.Structure):
    _fields_ = [(k, C.c_int32) for k in
                ('max_faces', 'max_texels', 'max_materials', 'max_textures', 'max_lights',
                 'max_filmsize', 'max_filmpasses')]


class DenoiseParams(C.Structure):
    _fields_ = [('iterations', C.c_int32), ('sigma_color', C.c_float), ('sigma_albedo', C.c_float), ('sigma_normal', C.c_float),
                ('demodulate', C.c_int32)]


class DisplayParams(C.Structure):
    '''mpt_display_params (include/miptina.h): what FilmTable.get_display hands to mpt_get_display'''
    _fields_ = [('source', C.c_int32), ('op', C.c_int32), ('transfer', C.c_int32), ('layout', C.c_int32), ('dither', C.c_int32),
                ('exposure', C.c_float), ('key', C.c_float), ('white', C.c_float), ('gamma', C.c_float)]


class NoiseStats(C.Structure):
    '''mpt_noise_stats (include/miptina.h): what mpt_get_noise and mpt_noise_eval hand back'''
    _fields_ = [('valid', C.c_int64), ('above', C.c_int64), ('sum', C.c_double), ('max', C.c_float), ('threshold', C.c_float)]


class NoiseResult:
    '''FilmTable.get_noise's answer: over the `valid` pixels, `above` of them with e > threshold, the `mean` of e (sum / valid, 0.0
    when nothing is valid), its `max`, `fraction` = above / valid (0.0 when nothing is valid), and the `map` [nx, ny] or None'''
    __slots__ = ('valid', 'above', 'sum', 'max', 'threshold', 'map')

    def __init__(self, stats, map=None):
        self.valid, self.above, self.sum = int(stats.valid), int(stats.above), float(stats.sum)
        self.max, self.threshold, self.map = float(stats.max), float(stats.threshold), map

    @property
    def mean(self):
        return self.sum / self.valid if self.valid else 0.0

    @property
    def fraction(self):
        return self.above / self.valid if self.valid else 0.0

    def __repr__(self):
        return 'NoiseResult(valid=%d, above=%d, mean=%.6g, max=%.6g, fraction=%.6g, threshold=%.6g)' % (
            self.valid, self.above, self.mean, self.max, self.fraction, self.threshold)


class ComposeInfo(C.Structure):
    '''mpt_compose_info (include/miptina.h): what mpt_compose_stats hands back'''
    _fields_ = [('faces', C.c_int64), ('recomposed', C.c_int64), ('dirty_objects', C.c_int64), ('host_fetches', C.c_int64),
                ('scene_cen', C.c_double * 3), ('scene_rad', C.c_double)]


class DeformInfo(C.Structure):
    '''mpt_deform_info (include/miptina.h): what mpt_deform_stats hands back'''
    _fields_ = [('deformable_objects', C.c_int64), ('deformed_objects', C.c_int64), ('deformed_corners', C.c_int64), ('copy_verts', C.c_int64)]


class AnimInfo(C.Structure):
    '''mpt_anim_info (include/miptina.h): what mpt_anim_stats hands back'''
    _fields_ = [('skeletons', C.c_int64), ('clips', C.c_int64), ('tracks', C.c_int64), ('bound_objects', C.c_int64), ('evaluated_objects', C.c_int64)]


class AnimBlendInfo(C.Structure):
    '''mpt_anim_blend_info (include/miptina.h): what mpt_anim_blend_stats hands back'''
    _fields_ = [('object_clips', C.c_int64), ('blended_objects', C.c_int64), ('moved_objects', C.c_int64), ('evaluated_blended', C.c_int64),
                ('evaluated_moved', C.c_int64)]


class SubdivInfo(C.Structure):
    '''mpt_subdiv_info (include/miptina.h): what mpt_subdiv_stats hands back'''
    _fields_ = [('subdivided_objects', C.c_int64), ('copies', C.c_int64), ('refined_copies', C.c_int64), ('refined_faces', C.c_int64),
                ('copy_verts', C.c_int64)]


class ScatterParams(C.Structure):
    '''mpt_scatter_params (include/miptina.h)'''
    _fields_ = [('smin', C.c_double), ('smax', C.c_double), ('up', C.c_double * 3), ('align', C.c_int32), ('random_yaw', C.c_int32),
                ('density_image', C.c_int32), ('channel', C.c_int32)]


class ScatterInfo(C.Structure):
    '''mpt_scatter_info (include/miptina.h): what mpt_scatter_stats hands back'''
    _fields_ = [('scatters', C.c_int64), ('instances', C.c_int64), ('selected_scatters', C.c_int64), ('placed_scatters', C.c_int64),
                ('placed_instances', C.c_int64), ('weight_launches', C.c_int64), ('scan_launches', C.c_int64), ('select_launches', C.c_int64),
                ('place_launches', C.c_int64), ('host_fetches', C.c_int64)]


class ScatterSpacingInfo(C.Structure):
    '''mpt_scatter_spacing_info (include/miptina.h): what mpt_scatter_spacing_stats hands back'''
    _fields_ = [('scatters', C.c_int64), ('candidates', C.c_int64), ('kept', C.c_int64), ('rounds', C.c_int64), ('grid_launches', C.c_int64),
                ('round_launches', C.c_int64), ('compact_launches', C.c_int64), ('host_reads', C.c_int64)]


class DisplaceInfo(C.Structure):
    '''mpt_displace_info (include/miptina.h): what mpt_displace_stats hands back'''
    _fields_ = [('displaced_meshes', C.c_int64), ('copies', C.c_int64), ('displaced_copies', C.c_int64), ('displaced_verts', C.c_int64),
                ('image_generation', C.c_int64)]


class RefitInfo(C.Structure):
    '''mpt_refit_info (include/miptina.h): what mpt_refit_stats hands back'''
    _fields_ = [('faces', C.c_int64), ('wide_nodes', C.c_int64), ('refits', C.c_int64), ('host_fetches', C.c_int64), ('allowed', C.c_int64),
                ('cost_built', C.c_double), ('cost_now', C.c_double), ('growth', C.c_double)]


class HistoryParams(C.Structure):
    '''mpt_history_params (include/miptina.h): what FilmTable.reproject hands to mpt_history_reproject'''
    _fields_ = [('max_history', C.c_float), ('depth_tol', C.c_float)]


class HistoryStats(C.Structure):
    '''mpt_history_stats (include/miptina.h): what mpt_history_reproject and mpt_history_eval hand back'''
    _fields_ = [(k, C.c_int64) for k in ('kept', 'statics', 'background_kept', 'disoccluded', 'offscreen', 'background_reset')]


class HierarchyInfo(C.Structure):
    '''mpt_hierarchy_info (include/miptina.h): what mpt_hierarchy_stats hands back'''
    _fields_ = [('bound_children', C.c_int64), ('deepest', C.c_int64), ('evaluated', C.c_int64), ('levels', C.c_int64), ('launches', C.c_int64)]


# mpt_history_motion (include/miptina.h) as a numpy record, and its flags
MOTION_DTYPE = np.dtype([('cur_id', np.int32), ('fx', np.float32), ('fy', np.float32), ('d_exp', np.float32), ('flags', np.int32)])
MOTION_NONE, MOTION_STATIC, MOTION_BACKGROUND = 0, 1, 2


class HistoryResult:
    '''FilmTable.reproject's answer: what became of the pixels of this context's share.  `kept` took over history through the
    taps (`static` of them word for word in place), `background_kept` kept their own sums behind an unchanged camera,
    `disoccluded` found every tap rejected, `offscreen` lay outside the kept view, `background_reset` see nothing under a changed
    camera; `pixels` is their sum and `kept_fraction` = (kept + background_kept) / pixels (0.0 for an empty share)'''
    __slots__ = ('kept', 'static', 'background_kept', 'disoccluded', 'offscreen', 'background_reset')

    def __init__(self, stats):
        self.kept, self.static, self.background_kept = int(stats.kept), int(stats.statics), int(stats.background_kept)
        self.disoccluded, self.offscreen, self.background_reset = int(stats.disoccluded), int(stats.offscreen), int(stats.background_reset)

    @property
    def pixels(self):
        return self.kept + self.background_kept + self.disoccluded + self.offscreen + self.background_reset

    @property
    def kept_fraction(self):
        return (self.kept + self.background_kept) / self.pixels if self.pixels else 0.0

    def astuple(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __repr__(self):
        return 'HistoryResult(kept=%d, static=%d, background_kept=%d, disoccluded=%d, offscreen=%d, background_reset=%d)' % self.astuple()


def history_params(max_history=32.0, depth_tol=0.02):
    '''HistoryParams from the arguments FilmTable.reproject takes, and their defaults (include/miptina.h states the same ones
    for a NULL mpt_history_params)'''
    return HistoryParams(float(max_history), float(depth_tol))


def history_allowed(have, kept_size, size, kept_faces, nfaces, tree_valid, max_history=32.0, depth_tol=0.02):
    '''mpt_history_allowed (no context, no GPU): (verdict, words); verdict 0 allows a reproject'''
    why = C.create_string_buffer(256)
    rc = load_library().mpt_history_allowed(int(bool(have)), int(kept_size[0]), int(kept_size[1]), int(size[0]), int(size[1]), int(kept_faces),
                                            int(nfaces), int(bool(tree_valid)), float(max_history), float(depth_tol), why, len(why))
    return rc, why.value.decode()


DISPLAY_DENOISED = -1
TONE_OPS = {'linear': 0, 'ptina': 1, 'reinhard': 2, 'aces': 3}
TRANSFERS = {'srgb': 0, 'gamma': 1}
LAYOUTS = {'film': 0, 'display': 1}


class Counters(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in
                ('samples', 'rays', 'n_box', 'n_tri', 'n_shade', 'n_draws', 'bounces', 'n_node',
                 'it_node', 'it_leaf', 'it_shade', 'it_new',
                 'pl_local', 'pl_batches', 'pl_batch_lanes', 'pl_prim', 'pl_tidle', 'pl_sidle', 'pl_trips', 'pl_taken')]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# every symbol include/miptina.h declares: name -> (restype, argtypes)
_vp, _i, _fp, _ip = C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int32)
SIGNATURES = {
    'mpt_last_error': (C.c_char_p, []),
    'mpt_device_count': (_i, []),
    'mpt_version': (_i, []),
    'mpt_create': (_vp, [C.POINTER(Caps), _i]),
    'mpt_destroy': (None, [_vp]),
    'mpt_set_option': (_i, [_vp, C.c_char_p, _i]),
    'mpt_get_option': (_i, [_vp, C.c_char_p, C.POINTER(_i)]),
    'mpt_set_size': (_i, [_vp, _i, _i]),
    'mpt_get_size': (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    'mpt_set_slab': (_i, [_vp, _i, _i]),
    'mpt_set_stripes': (_i, [_vp, _i, _i, _i]),
    'mpt_load_model': (_i, [_vp, _fp, _ip, _i]),
    'mpt_load_materials': (_i, [_vp, _fp, _ip, _i]),
    'mpt_reset_images': (_i, [_vp]),
    'mpt_load_image': (_i, [_vp, _fp, _i, _i, C.POINTER(_i)]),
    'mpt_build_tree': (_i, [_vp]),
    'mpt_get_tree': (_i, [_vp, _ip, _ip, _fp, _fp, _ip, _ip]),
    'mpt_get_wide': (_i, [_vp, _fp, _fp, _i, C.POINTER(_i)]),
    'mpt_get_records': (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _i, C.POINTER(_i)]),
    'mpt_sah_workspace': (_i, [_i, C.c_int64, C.POINTER(C.c_int64)]),
    'mpt_set_camera': (_i, [_vp, _fp, _fp]),
    'mpt_clear_lights': (_i, [_vp]),
    'mpt_add_light': (_i, [_vp, _i, _fp, _fp, _fp, C.c_float, C.POINTER(_i)]),
    'mpt_set_world_light': (_i, [_vp, _fp, _i]),
    'mpt_sobol_init': (_i, [_vp, _ip, _i, _i]),
    'mpt_sobol_reset': (_i, [_vp, _i]),
    'mpt_sobol_update': (_i, [_vp, _i]),
    'mpt_sobol_get': (_i, [_vp, _ip, _fp, _ip]),
    'mpt_render': (_i, [_vp, _i]),
    'mpt_render_preview': (_i, [_vp, _i]),
    'mpt_mlt_reset': (_i, [_vp, _i, C.c_uint32]),
    'mpt_mlt_set_param': (_i, [_vp, C.c_float, C.c_float]),
    'mpt_mlt_render': (_i, [_vp, _i]),
    'mpt_mlt_get_state': (_i, [_vp, _fp, _fp, C.POINTER(_i)]),
    'mpt_mlt_set_state': (_i, [_vp, _fp, _fp, _i]),
    'mpt_mlt_trace': (_i, [_vp, _fp, _fp, _i]),
    'mpt_mlt_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_render_brute': (_i, [_vp, _i]),
    'mpt_brute_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_flush': (_i, [_vp]),
    'mpt_synchronize': (_i, [_vp]),
    'mpt_clear': (_i, [_vp, _i]),
    'mpt_get_image': (_i, [_vp, _i, _fp]),
    'mpt_hint_image': (_i, [_vp, _i, _fp]),
    'mpt_fast_export_image': (_i, [_vp, _i, _fp]),
    'mpt_get_film_raw': (_i, [_vp, _i, _fp]),
    'mpt_resolve': (_i, [_vp, _i]),
    'mpt_get_denoised': (_i, [_vp, C.POINTER(DenoiseParams), _fp]),
    'mpt_denoise_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_denoise_set_variance': (_i, [_vp, C.c_float]),
    'mpt_denoise_get_variance': (_i, [_vp, _fp]),
    'mpt_denoise_eval': (_i, [_vp, C.POINTER(DenoiseParams), C.c_float, _fp, _fp, _fp, _fp, _i, _i, _fp, _fp]),
    'mpt_get_display': (_i, [_vp, C.POINTER(DisplayParams), C.POINTER(DenoiseParams), C.POINTER(C.c_uint8), _fp]),
    'mpt_display_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_display_eval': (_i, [_vp, C.POINTER(DisplayParams), _fp, _i, _i, C.POINTER(C.c_uint8), _fp]),
    'mpt_film_mark': (_i, [_vp]),
    'mpt_get_noise': (_i, [_vp, C.c_float, _i, _fp, C.POINTER(NoiseStats)]),
    'mpt_get_mark': (_i, [_vp, _fp]),
    'mpt_noise_eval': (_i, [_vp, C.c_float, _fp, _fp, _i, _i, _fp, _fp, C.POINTER(NoiseStats)]),
    'mpt_noise_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_adapt_select': (_i, [_vp, C.c_float, _i, C.POINTER(NoiseStats), C.POINTER(_i)]),
    'mpt_adapt_get_list': (_i, [_vp, _ip, _i, C.POINTER(_i)]),
    'mpt_adapt_set_list': (_i, [_vp, _ip, _i]),
    'mpt_render_selected': (_i, [_vp, _i, _i]),
    'mpt_adapt_eval': (_i, [_vp, C.c_float, _i, _fp, _fp, _i, _i, _ip, _i, C.POINTER(_i), C.POINTER(NoiseStats)]),
    'mpt_adapt_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_mesh_add': (_i, [_vp, _fp, _i, C.POINTER(_i)]),
    'mpt_object_add': (_i, [_vp, _i, C.POINTER(C.c_double), _i, C.POINTER(_i)]),
    'mpt_object_set_world': (_i, [_vp, _i, C.POINTER(C.c_double)]),
    'mpt_object_set_material': (_i, [_vp, _i, _i]),
    'mpt_scene_clear': (_i, [_vp, _i]),
    'mpt_compose': (_i, [_vp]),
    'mpt_compose_stats': (_i, [_vp, C.POINTER(ComposeInfo)]),
    'mpt_get_model': (_i, [_vp, _fp, _ip, _i, C.POINTER(_i)]),
    'mpt_compose_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_compose_plan': (_i, [_ip, _ip, _i, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i]),
    'mpt_mesh_set_morph': (_i, [_vp, _i, _fp, _i]),
    'mpt_mesh_set_skin': (_i, [_vp, _i, C.POINTER(C.c_uint16), _fp, _i]),
    'mpt_object_set_morph_weights': (_i, [_vp, _i, C.POINTER(C.c_double), _i]),
    'mpt_object_set_joints': (_i, [_vp, _i, C.POINTER(C.c_double), _i]),
    'mpt_get_deformed': (_i, [_vp, _i, _fp, _i]),
    'mpt_deform_stats': (_i, [_vp, C.POINTER(DeformInfo)]),
    'mpt_deform_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_deform_plan': (_i, [_ip, _ip, _i, _ip, C.POINTER(C.c_int64), _i, C.POINTER(C.c_int64)]),
    'mpt_skin_check': (_i, [C.POINTER(C.c_uint16), _fp, C.c_int64, _i, C.c_char_p, _i]),
    'mpt_mesh_set_skeleton': (_i, [_vp, _i, _i, _ip, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'mpt_mesh_add_clip': (_i, [_vp, _i, _i, _ip, _fp, C.c_int64, _fp, C.c_int64, C.POINTER(_i)]),
    'mpt_object_set_animation': (_i, [_vp, _i, _i, C.c_double, C.c_double, _i]),
    'mpt_scene_set_time': (_i, [_vp, C.c_double]),
    'mpt_get_pose': (_i, [_vp, _i, C.POINTER(C.c_double), _i]),
    'mpt_anim_stats': (_i, [_vp, C.POINTER(AnimInfo)]),
    'mpt_anim_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_anim_rule': (_i, [_i, _i, _ip, C.POINTER(C.c_double), C.POINTER(C.c_double), _i, _ip, _fp, C.c_int64, _fp, C.c_int64, C.c_double, C.c_double, _i,
                           C.c_double, C.POINTER(C.c_double)]),
    'mpt_clip_check': (_i, [_i, _i, _i, _ip, _fp, C.c_int64, _fp, C.c_int64, C.c_char_p, _i]),
    'mpt_anim_trig': (_i, [_vp, C.POINTER(C.c_double), _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'mpt_object_set_animation_blend': (_i, [_vp, _i, _i, C.c_double, C.c_double, _i, C.c_double, C.c_double, C.c_double, C.c_double]),
    'mpt_scene_add_object_clip': (_i, [_vp, _i, _ip, _fp, C.c_int64, _fp, C.c_int64, C.POINTER(_i)]),
    'mpt_object_set_motion': (_i, [_vp, _i, _i, C.c_double, C.c_double, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'mpt_get_object_world': (_i, [_vp, _i, C.POINTER(C.c_double)]),
    'mpt_anim_blend_stats': (_i, [_vp, C.POINTER(AnimBlendInfo)]),
    'mpt_motion_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_anim_blend_rule': (_i, [_i, _i, _ip, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 _i, _ip, _fp, C.c_int64, _fp, C.c_int64, C.c_double, C.c_double, _i,
                                 _i, _ip, _fp, C.c_int64, _fp, C.c_int64, C.c_double, C.c_double, _i,
                                 C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    'mpt_motion_rule': (_i, [_i, _ip, _fp, C.c_int64, _fp, C.c_int64, C.c_double, C.c_double, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                             C.POINTER(C.c_double)]),
    'mpt_object_set_parent': (_i, [_vp, _i, _i, _i]),
    'mpt_object_get_parent': (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    'mpt_hierarchy_stats': (_i, [_vp, C.POINTER(HierarchyInfo)]),
    'mpt_hierarchy_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_parent_check': (_i, [_i, _ip, _ip, _ip, _i, _i, _i, C.c_char_p, _i]),
    'mpt_hierarchy_rule': (_i, [_i, C.POINTER(C.c_double), _ip, _ip, _fp, C.POINTER(C.c_int64), _fp, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                C.POINTER(C.c_double), _ip, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double)]),
    'mpt_mesh_set_subdivision': (_i, [_vp, _i, _i]),
    'mpt_get_subdivided': (_i, [_vp, _i, _fp, _i]),
    'mpt_subdiv_stats': (_i, [_vp, C.POINTER(SubdivInfo)]),
    'mpt_subdiv_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_subdiv_topology': (_i, [_fp, _i, _i, C.POINTER(C.c_int64), _ip, _ip, C.c_int64, C.POINTER(C.c_int64), C.c_char_p, _i]),
    'mpt_mesh_set_subdivision_creased': (_i, [_vp, _i, _i, _fp, C.POINTER(C.c_uint8)]),
    'mpt_subdiv_topology_creased': (_i, [_fp, _i, _i, _fp, C.POINTER(C.c_uint8), C.POINTER(C.c_int64), _ip, _ip, C.c_int64, C.POINTER(C.c_int64), C.c_char_p, _i]),
    'mpt_mesh_set_subdivision_cc': (_i, [_vp, _i, _i, _ip, _i, _fp, C.POINTER(C.c_uint8)]),
    'mpt_subdiv_topology_cc': (_i, [_fp, _i, _i, _ip, _i, _fp, C.POINTER(C.c_uint8), C.POINTER(C.c_int64), _ip, _ip, C.c_int64, C.POINTER(C.c_int64), C.c_char_p, _i]),
    'mpt_subdiv_plan': (_i, [_ip, _ip, _i, _ip, C.POINTER(C.c_int64), _i, C.POINTER(C.c_int64)]),
    'mpt_mesh_set_displacement': (_i, [_vp, _i, _i, _i, _i, C.c_double, C.c_double]),
    'mpt_mesh_set_displacement_params': (_i, [_vp, _i, C.c_double, C.c_double]),
    'mpt_displace_stats': (_i, [_vp, C.POINTER(DisplaceInfo)]),
    'mpt_displace_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_displace_corners': (_i, [_ip, C.c_int64, C.c_int32, _ip]),
    'mpt_scatter_add': (_i, [_vp, _i, _i, _i, C.c_uint64, _i, C.POINTER(ScatterParams), C.POINTER(_i), C.POINTER(_i)]),
    'mpt_scatter_set_params': (_i, [_vp, _i, C.POINTER(ScatterParams)]),
    'mpt_scatter_rescatter': (_i, [_vp, _i, C.c_uint64]),
    'mpt_scatter_stats': (_i, [_vp, C.POINTER(ScatterInfo)]),
    'mpt_scatter_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_scatter_get': (_i, [_vp, _i, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    'mpt_scatter_rule': (_i, [C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_int64, C.POINTER(ScatterParams), C.c_uint64, C.c_int64, C.c_int64,
                              C.c_void_p, C.POINTER(C.c_double)]),
    'mpt_scatter_set_spacing': (_i, [_vp, _i, C.c_double, C.c_int64]),
    'mpt_scatter_get_spacing': (_i, [_vp, _i, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int64)]),
    'mpt_scatter_spacing_stats': (_i, [_vp, C.POINTER(ScatterSpacingInfo)]),
    'mpt_scatter_spacing_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_scatter_space_rule': (_i, [C.POINTER(C.c_double), C.c_int64, C.c_double, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]),
    'mpt_scatter_space_points': (_i, [_vp, C.POINTER(C.c_double), C.c_int64, C.c_double, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]),
    'mpt_refit_tree': (_i, [_vp]),
    'mpt_refit_stats': (_i, [_vp, C.POINTER(RefitInfo)]),
    'mpt_refit_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_refit_allowed': (_i, [_i, _i, _i, _i, C.c_char_p, _i]),
    'mpt_refit_growth': (C.c_double, [C.c_uint64, C.c_uint64]),
    'mpt_query_closest': (_i, [_vp, _i, _fp, _fp, _ip, _ip, _fp, _ip, _fp, _fp, _ip, _i]),
    'mpt_query_occluded': (_i, [_vp, _i, _fp, _fp, _fp, _ip, _ip, _i]),
    'mpt_query_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_walk_trace': (_i, [_vp, _i, _i, _fp, _fp, _ip, _fp, _ip, _fp, _ip, _fp, _fp, _i]),
    'mpt_history_keep': (_i, [_vp]),
    'mpt_history_reproject': (_i, [_vp, C.POINTER(HistoryParams), C.POINTER(HistoryStats)]),
    'mpt_history_drop': (_i, [_vp]),
    'mpt_history_get_motion': (_i, [_vp, _vp]),
    'mpt_history_get_gbuffer': (_i, [_vp, _ip, _ip, _fp]),
    'mpt_history_eval': (_i, [_vp, C.POINTER(HistoryParams), _fp, _ip, _ip, _fp, _vp, _i, _i, _fp, C.POINTER(HistoryStats)]),
    'mpt_history_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_history_allowed': (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.c_float, C.c_float, C.c_char_p, _i]),
    'mpt_host_alloc': (_vp, [C.c_size_t]),
    'mpt_host_free': (None, [_vp]),
    'mpt_get_counters': (_i, [_vp, C.POINTER(Counters)]),
    'mpt_get_timeline': (_i, [_vp, C.POINTER(C.c_ulonglong), _i, C.POINTER(_i)]),
    'mpt_reset_counters': (_i, [_vp]),
    'mpt_get_shade_variant': (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    'mpt_get_lane_hist': (_i, [_vp, C.POINTER(C.c_uint64), _i]),
    'mpt_probe_kernel': (_i, [_vp, _i, _i, C.POINTER(C.c_double)]),
    'mpt_stress_copies': (_i, [_vp, _i, _i]),
    'mpt_kernel_time': (_i, [_vp, C.POINTER(C.c_double), C.POINTER(_i)]),
    'mpt_unit_eval': (_i, [_vp, _i, _vp, _i, _vp, _i, _i]),
    'mpt_comm_unique_id': (_i, [C.c_char_p]),
    'mpt_comm_init': (_i, [_vp, C.c_char_p, _i, _i]),
    'mpt_comm_plan': (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i]),
    'mpt_comm_gather_film': (_i, [_vp, _i, _i]),
    'mpt_comm_selftest': (_i, [_vp, _i, _i, _i, _fp, _fp]),
    'mpt_comm_barrier': (_i, [_vp]),
    'mpt_comm_allreduce_max': (_i, [_vp, C.POINTER(C.c_double)]),
    'mpt_comm_destroy': (_i, [_vp]),
}

_lib = None
_lock = threading.Lock()


def load_library():
    '''dlopen libmiptina.so and bind every declared symbol (no GPU needed for this)'''
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    f'{LIB_PATH} not found: build it with `make -C ptina_amd/csrc` '
                    '(or __graft_entry__.build()); there is no CPU fallback')
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                f = getattr(lib, name)
                f.restype = res
                f.argtypes = args
            _lib = lib
    return _lib


def last_error():
    return load_library().mpt_last_error().decode('utf-8', 'replace')


def check(rc):
    if rc != 0:
        raise RuntimeError(last_error())


class HostBuffer:
    '''a page-locked host buffer of libmiptina; goes back to the pool when the last numpy view dies'''
    _pool = {}                                  # bytes -> [addresses]
    _pool_cap = 4

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        free = HostBuffer._pool.get(self.nbytes)
        if free:
            self.addr = free.pop()
        else:
            self.addr = load_library().mpt_host_alloc(self.nbytes)
            if not self.addr:
                raise MemoryError(last_error())

    def __del__(self):
        try:
            free = HostBuffer._pool.setdefault(self.nbytes, [])
            if len(free) < HostBuffer._pool_cap:
                free.append(self.addr)
            else:
                load_library().mpt_host_free(self.addr)
        except Exception:
            pass


def host_array(shape, dtype=np.float32):
    '''a fresh numpy array on page-locked memory (read-backs into it are a single DMA); the buffer is
    recycled as soon as the array and every view of it are gone (plain reference counting: the array's
    base is a ctypes buffer that owns the HostBuffer, and nothing points back)'''
    count = int(np.prod(shape))
    hb = HostBuffer(max(count * np.dtype(dtype).itemsize, 1))
    buf = (C.c_char * hb.nbytes).from_address(hb.addr)
    buf._owner = hb
    return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


def display_params(source=0, op='aces', transfer='srgb', layout='film', dither=True, exposure=None, key=0.18, white=4.0, gamma=2.2):
    '''DisplayParams from the names FilmTable.get_display takes (an integer is passed through, so that a test can name an
    operator the library does not know); exposure None = auto'''
    def code(table, v, what):
        if isinstance(v, str):
            if v.lower() not in table:
                raise ValueError('unknown %s %r: one of %s' % (what, v, sorted(table)))
            return table[v.lower()]
        return int(v)
    return DisplayParams(int(source), code(TONE_OPS, op, 'op'), code(TRANSFERS, transfer, 'transfer'), code(LAYOUTS, layout, 'layout'),
                         1 if dither else 0, 0.0 if exposure is None else float(exposure), float(key), float(white), float(gamma))


def denoise_params(*args, who='get_denoised', **kw):
    '''DenoiseParams from the arguments FilmTable.get_denoised takes (in this order, or by name), and their defaults (include/miptina.h states the same ones for
    a NULL mpt_denoise_params); `who` names the caller in the TypeError an unknown keyword raises'''
    d = dict(iterations=5, sigma_color=1.0, sigma_albedo=0.1, sigma_normal=0.3, demodulate=True)
    unknown = set(kw) - set(d)
    if unknown or len(args) > len(d):
        raise TypeError('%s: unknown keyword(s) %s' % (who, sorted(unknown)) if unknown else '%s: too many arguments' % who)
    d.update(zip(d, args), **kw)
    return DenoiseParams(int(d['iterations']), float(d['sigma_color']), float(d['sigma_albedo']), float(d['sigma_normal']),
                         1 if d['demodulate'] else 0)


def fptr(a):
    return a.ctypes.data_as(_fp)


def iptr(a):
    return a.ctypes.data_as(_ip)


def compose_plan(faces, dirty=None):
    '''mpt_compose_plan (no context, no GPU): per-object face counts and dirty flags (None: all) -> (first faces [nobj + 1],
    [(first workgroup, workgroups), ...] of the launch); ValueError for counts that name no layout'''
    f = np.ascontiguousarray(faces, np.int32).reshape(-1)
    d = None if dirty is None else np.ascontiguousarray(dirty, np.int32).reshape(-1)
    if d is not None and d.shape != f.shape:
        raise ValueError('%d dirty flags for %d objects' % (d.size, f.size))
    n = int(f.size)
    first, begin, count = np.zeros(n + 1, np.int64), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
    p64 = C.POINTER(C.c_int64)
    nr = load_library().mpt_compose_plan(iptr(f), None if d is None else iptr(d), n, first.ctypes.data_as(p64), begin.ctypes.data_as(p64),
                                         count.ctypes.data_as(p64), n)
    if nr < 0:
        raise ValueError('face counts name no layout (negative, or more than 2^31 / 3 faces)')
    return first, [(int(begin[r]), int(count[r])) for r in range(nr)]


DEFORM_CHUNK, DEFORM_MAX_JOINTS, DEFORM_MAX_TARGETS = 1024, 256, 64      # csrc/mpt_types.h MPT_DEFORM_*


def _run_plan(symbol, counts, dirty, rows, what):
    '''the run table of a launch (csrc/run_table.h) through the door `symbol`; `rows` and `what` name the table's rows in the refusals'''
    k = np.ascontiguousarray(counts, np.int32).reshape(-1)
    d = None if dirty is None else np.ascontiguousarray(dirty, np.int32).reshape(-1)
    if d is not None and d.shape != k.shape:
        raise ValueError('%d dirty flags for %d %s' % (d.size, k.size, rows))
    n = int(k.size)
    item, block, blocks = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64), C.c_int64(0)
    nr = getattr(load_library(), symbol)(iptr(k), None if d is None else iptr(d), n, iptr(item), block.ctypes.data_as(C.POINTER(C.c_int64)), n,
                                         C.byref(blocks))
    if nr < 0:
        raise ValueError('%s counts name no launch (negative, or more than 2^31 - 1 blocks)' % what)
    return [(int(item[r]), int(block[r])) for r in range(nr)], int(blocks.value)


def deform_plan(corners, dirty=None):
    '''mpt_deform_plan (no context, no GPU): per-object corner counts and dirty flags (None: all) -> ([(object, first block), ...] of
    the launch, its blocks); ValueError for counts that name no launch'''
    return _run_plan('mpt_deform_plan', corners, dirty, 'objects', 'corner')


def skin_check(joints, weights, njoints):
    '''mpt_skin_check (no context, no GPU): (verdict, words) for joints [m,4] uint16 and weights [m,4] f32 over njoints joints;
    verdict 0 accepts'''
    j, w = np.ascontiguousarray(joints, np.uint16), np.ascontiguousarray(weights, np.float32)
    if j.ndim != 2 or j.shape[1] != 4 or w.shape != j.shape:
        raise ValueError('joints and weights must be [m,4], got %s and %s' % (j.shape, w.shape))
    why = C.create_string_buffer(200)
    rc = load_library().mpt_skin_check(j.ctypes.data_as(C.POINTER(C.c_uint16)), fptr(w), j.shape[0], int(njoints), why, len(why))
    return rc, why.value.decode()


ANIM_PATHS = ('T', 'R', 'S', 'W')                                        # csrc/mpt_types.h MPT_ANIM_T .. _W
ANIM_INTERPOLATIONS = ('STEP', 'LINEAR', 'CUBICSPLINE')                  # ... MPT_ANIM_STEP .. _CUBICSPLINE


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _clip_arrays(spec, times, values):
    spec = np.ascontiguousarray(spec, np.int32).reshape(-1, 4)
    return spec, np.ascontiguousarray(times, np.float32).reshape(-1), np.ascontiguousarray(values, np.float32).reshape(-1)


def clip_check(njoints, ntargets, spec, times, values):
    '''mpt_clip_check (no context, no GPU): (verdict, words) for a clip's packed arrays (tools.anim.pack_clip: spec [n,4] of target,
    path, interpolation, nkeys; the tracks' times and values back to back) on a mesh of njoints joints and ntargets morph targets;
    verdict 0 accepts'''
    spec, times, values = _clip_arrays(spec, times, values)
    why = C.create_string_buffer(200)
    rc = load_library().mpt_clip_check(int(njoints), int(ntargets), spec.shape[0], iptr(spec), fptr(times), times.size, fptr(values), values.size,
                                       why, len(why))
    return rc, why.value.decode()


def anim_rule(parents, rest, inverse_bind, ntargets, spec, times, values, offset, speed, loop, t):
    '''mpt_anim_rule (no context, no GPU): the pose (weights [ntargets], palette [nj,3,4]) of one object at scene time t -- skeleton
    parents [nj], rest [nj,10] (translation3 rotation4 xyzw scale3), inverse_bind [nj,3,4] (nj 0: no skeleton), the clip's packed
    arrays and the binding; ValueError with the verdict for arrays the rule refuses'''
    parents = np.ascontiguousarray(parents, np.int32).reshape(-1)
    nj = int(parents.size)
    rest = np.ascontiguousarray(rest, np.float64).reshape(nj, 10)
    inverse_bind = np.ascontiguousarray(inverse_bind, np.float64).reshape(nj, 12)
    spec, times, values = _clip_arrays(spec, times, values)
    pose = np.zeros(int(ntargets) + 12 * nj, np.float64)
    rc = load_library().mpt_anim_rule(nj, int(ntargets), iptr(parents), _dptr(rest), _dptr(inverse_bind), spec.shape[0], iptr(spec), fptr(times), times.size,
                                      fptr(values), values.size, float(offset), float(speed), int(bool(loop)), float(t), _dptr(pose))
    if rc:
        raise ValueError('mpt_anim_rule refuses its arrays: verdict %d' % rc)
    return pose[:int(ntargets)].copy(), pose[int(ntargets):].reshape(nj, 3, 4).copy()


def blend_weights(weight, fade):
    '''(w0, w1, fade_start, fade_duration) of a second binding: `weight` a number or (w0, w1), `fade` (start, duration) or None -- the
    weight is then w1 from the first'''
    w0, w1 = (float(weight), float(weight)) if np.ndim(weight) == 0 else (float(weight[0]), float(weight[1]))
    start, duration = (0.0, 0.0) if fade is None else (float(fade[0]), float(fade[1]))
    return w0, w1, start, duration


def anim_blend_rule(parents, rest, inverse_bind, ntargets, clip_a, binding_a, clip_b, binding_b, fade, t):
    '''mpt_anim_blend_rule (no context, no GPU): the pose (weights [ntargets], palette [nj,3,4]) at scene time t of one object with two
    bindings -- clip_a and clip_b packed clips (tools.anim.pack_clip), binding_a and binding_b (offset, speed, loop), fade (w0, w1,
    fade_start, fade_duration); ValueError with the verdict for what the rule refuses'''
    parents = np.ascontiguousarray(parents, np.int32).reshape(-1)
    nj = int(parents.size)
    rest = np.ascontiguousarray(rest, np.float64).reshape(nj, 10)
    inverse_bind = np.ascontiguousarray(inverse_bind, np.float64).reshape(nj, 12)
    sa, ta, va = _clip_arrays(*clip_a)
    sb, tb, vb = _clip_arrays(*clip_b)
    pose = np.zeros(int(ntargets) + 12 * nj, np.float64)
    rc = load_library().mpt_anim_blend_rule(nj, int(ntargets), iptr(parents), _dptr(rest), _dptr(inverse_bind),
                                            sa.shape[0], iptr(sa), fptr(ta), ta.size, fptr(va), va.size, float(binding_a[0]), float(binding_a[1]), int(bool(binding_a[2])),
                                            sb.shape[0], iptr(sb), fptr(tb), tb.size, fptr(vb), vb.size, float(binding_b[0]), float(binding_b[1]), int(bool(binding_b[2])),
                                            *[float(x) for x in fade], float(t), _dptr(pose))
    if rc:
        raise ValueError('mpt_anim_blend_rule refuses its arguments: verdict %d' % rc)
    return pose[:int(ntargets)].copy(), pose[int(ntargets):].reshape(nj, 3, 4).copy()


def motion_rule(clip, binding, rest, base, t):
    '''mpt_motion_rule (no context, no GPU): the world matrix [4,4] at scene time t of an object bound to the packed object clip `clip`
    by binding (offset, speed, loop), rest [10] or None and base [4,4] or None; ValueError with the verdict for what the rule refuses'''
    spec, times, values = _clip_arrays(*clip)
    rest = None if rest is None else np.ascontiguousarray(rest, np.float64).reshape(10)
    base = None if base is None else np.ascontiguousarray(base, np.float64).reshape(16)
    world = np.zeros(16, np.float64)
    rc = load_library().mpt_motion_rule(spec.shape[0], iptr(spec), fptr(times), times.size, fptr(values), values.size, float(binding[0]), float(binding[1]),
                                        int(bool(binding[2])), None if rest is None else _dptr(rest), None if base is None else _dptr(base), float(t),
                                        _dptr(world))
    if rc:
        raise ValueError('mpt_motion_rule refuses its arguments: verdict %d' % rc)
    return world.reshape(4, 4)


HIER_MAX_DEPTH, HIER_ONE_GROUP = 64, 1024                                # csrc/mpt_types.h MPT_HIER_*
PARENT_REFUSALS = ('ok', 'unknown', 'cycle', 'instance', 'no skin', 'joint', 'depth')     # csrc/anim_rule.h MptParentVerdict


def parent_check(parents, instance, njoints, obj, parent, joint=None):
    '''mpt_parent_check (no context, no GPU): (verdict, words) for binding object obj to (parent, joint) in a table whose bindings stand
    as parents [n] (-1: a root), with instance [n] (true: an instance of a scatter) and njoints [n] (of each object's mesh's skin);
    verdict 0 accepts, the others index PARENT_REFUSALS'''
    parents = np.ascontiguousarray(parents, np.int32).reshape(-1)
    instance = np.ascontiguousarray(np.asarray(instance) != 0, np.int32).reshape(-1)
    njoints = np.ascontiguousarray(njoints, np.int32).reshape(-1)
    if not parents.size == instance.size == njoints.size:
        raise ValueError('parents, instance and njoints must have one length')
    why = C.create_string_buffer(200)
    rc = load_library().mpt_parent_check(int(parents.size), iptr(parents), iptr(instance), iptr(njoints), int(obj), -1 if parent is None else int(parent),
                                         -1 if joint is None else int(joint), why, len(why))
    return rc, why.value.decode()


def hierarchy_rule(chain, t):
    '''mpt_hierarchy_rule (no context, no GPU): the world matrix [4,4] at scene time t of the last link of `chain`, a list of links
    from the root down; a link is a dict of local [4,4] (its local matrix) or motion=(packed object clip, (offset, speed, loop), rest
    [10] or None, base [4,4] or None), and, below the root, pal [3,4] or None: the palette entry it follows.  ValueError with the
    verdict for what the rule refuses'''
    n = len(chain)
    locals_, ntracks, joints = np.zeros((n, 16)), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    bindings, rests, palette = np.zeros((n, 3)), np.tile(np.float64([0, 0, 0, 0, 0, 0, 1, 1, 1, 1]), (n, 1)), np.zeros((n, 12))
    ntimes, nvalues = np.zeros(n, np.int64), np.zeros(n, np.int64)
    specs, times, values = [np.zeros((0, 4), np.int32)], [np.zeros(0, np.float32)], [np.zeros(0, np.float32)]
    for k, ln in enumerate(chain):
        if ln.get('motion') is not None:
            clip, binding, rest, base = ln['motion']
            sp, ti, va = _clip_arrays(*clip)
            specs.append(sp), times.append(ti), values.append(va)
            ntracks[k], ntimes[k], nvalues[k] = sp.shape[0], ti.size, va.size
            bindings[k] = float(binding[0]), float(binding[1]), float(bool(binding[2]))
            if rest is not None:
                rests[k] = np.asarray(rest, np.float64).reshape(10)
            locals_[k] = np.eye(4).reshape(16) if base is None else np.asarray(base, np.float64).reshape(16)
        else:
            locals_[k] = np.asarray(ln['local'], np.float64).reshape(16)
        if ln.get('pal') is not None:
            joints[k], palette[k] = 0, np.asarray(ln['pal'], np.float64).reshape(12)
    spec, ti, va = np.ascontiguousarray(np.concatenate(specs)), np.ascontiguousarray(np.concatenate(times)), np.ascontiguousarray(np.concatenate(values))
    world = np.zeros(16, np.float64)
    i64 = C.POINTER(C.c_int64)
    rc = load_library().mpt_hierarchy_rule(n, _dptr(locals_), iptr(ntracks), iptr(spec), fptr(ti), ntimes.ctypes.data_as(i64), fptr(va),
                                           nvalues.ctypes.data_as(i64), _dptr(bindings), _dptr(rests), iptr(joints), _dptr(palette), float(t), _dptr(world))
    if rc:
        raise ValueError('mpt_hierarchy_rule refuses its arguments: verdict %d' % rc)
    return world.reshape(4, 4)


SUBDIV_CHUNK, SUBDIV_MAX_LEVELS = 256, 5                                # csrc/mpt_types.h MPT_SUBDIV_*


def subdiv_plan(items, dirty=None):
    '''mpt_subdiv_plan (no context, no GPU): per-job item counts of one launch and dirty flags (None: all) -> ([(job, first block),
    ...], its blocks); ValueError for counts that name no launch'''
    return _run_plan('mpt_subdiv_plan', items, dirty, 'jobs', 'item')


SUBDIV_VARIANTS = ('plain', 'blend_crease', 'blend_corner', 'fixed')      # csrc/mpt_types.h MPT_SUBDIV_PLAIN .. _FIXED (on an edge, 1 is MPT_SUBDIV_BLEND_EDGE)
SUBDIV_CC, SUBDIV_MAX_CORNERS = 4, 64                                    # csrc/mpt_types.h MPT_SUBDIV_CC (a bit of the variant), MPT_SUBDIV_MAX_CORNERS
SUBDIV_SCHEMES = ('loop', 'catmull-clark')


def _subdiv_records(rec):
    rec = np.ascontiguousarray(rec, np.float32)
    if rec.ndim != 2 or rec.shape[1] != 8 or rec.shape[0] % 3:
        raise ValueError('records must be [3k,8], got %s' % (rec.shape,))
    return rec


def _subdiv_call(entry, args, levels, noffsets):
    '''a topology entry point (args: what it takes in front of counts), called twice: for the number of words, then for the words.
    (verdict, the words of the refusal), else (0, (counts [levels+1,3], offsets [noffsets], the block))'''
    call = getattr(load_library(), entry)
    why = C.create_string_buffer(240)
    counts, off, need = np.zeros((max(levels, 0) + 1, 3), np.int64), np.zeros(noffsets, np.int32), C.c_int64(0)
    cp = counts.ctypes.data_as(C.POINTER(C.c_int64))
    rc = call(*args, cp, iptr(off), None, 0, C.byref(need), why, len(why))
    if rc:
        return rc, why.value.decode()
    w = np.zeros(max(int(need.value), 1), np.int32)
    rc = call(*args, cp, iptr(off), iptr(w), int(need.value), C.byref(need), why, len(why))
    assert rc == 0
    return 0, (counts, off, w[:int(need.value)])


def _subdiv_decode(counts, off, w, levels):
    '''the tables of a block of words w (csrc/subdiv_rule.h documents it): a rule is (kind, variant, [ids], parameter)'''
    def rule(h, r):
        kind, variant, n = h & 3, h >> 28 & 7, h >> 2 & (1 << 26) - 1
        cc, blend = variant & SUBDIV_CC, variant & 3
        nids = n
        if kind == 0:                                                   # an interior vertex: n face point ids, p q
            nids += (n if cc else 0) + (2 if blend == 1 else 0)
        blends = (kind == 0 and blend in (1, 2)) or (kind == 2 and blend == 1)
        return kind, variant, w[r:r + nids].tolist(), float(w[r + nids:r + nids + 2].view(np.float64)[0]) if blends else None

    def rules(at, n):
        return [rule(int(h), int(r)) for h, r in zip(w[at:at + 2 * n:2], w[at + 1:at + 2 * n:2])]
    t = dict(counts=counts, first_corner=w[:int(counts[0, 0])].copy(), rules={l: rules(int(off[l]), int(counts[l, 0])) for l in range(1, levels + 1)},
             rings=[(kind, ids) for kind, _, ids, _ in rules(int(off[6]), int(counts[levels, 0]))], faces=w[int(off[7]):int(off[8])].reshape(-1, 3).copy(),
             offsets=off.copy())
    if len(off) > 9:                                                    # the last level's records
        nrec = int(off[10])
        t['records'] = [(v, kind, ids) for v, (kind, ids) in enumerate(t['rings'])]
        if off[9]:
            vert = w[int(off[9]) + 2 * nrec:int(off[9]) + 3 * nrec].tolist()
            t['records'] = [(v, kind, ids) for v, (kind, _, ids, _) in zip(vert, rules(int(off[9]), nrec))]
    if len(off) > 11:                                                   # the table of level-1 quads
        nq1 = int(counts[1, 2])
        t['quads1'] = w[int(off[11]):int(off[11]) + 2 * nq1].reshape(nq1, 2).copy()
    return t


def subdiv_topology(rec, levels):
    '''mpt_subdiv_topology (no context, no GPU) of the records rec [3k,8] f32: (verdict, words, tables).  verdict 0 accepts, and
    tables is then a dict: counts [levels+1,3] (vertices, edges, faces), first_corner [V_0], rules[l] for l = 1..levels -- a list
    of (kind, [ids of level l-1]) per vertex of level l --, rings -- the same for the last level's vertices --, faces [F_L,3]'''
    rec, levels = _subdiv_records(rec), int(levels)
    rc, got = _subdiv_call('mpt_subdiv_topology', (fptr(rec), rec.shape[0] // 3, levels), levels, 9)
    if rc:
        return rc, got, None
    t = _subdiv_decode(*got, levels)
    return 0, '', dict(counts=t['counts'], first_corner=t['first_corner'], rules={l: [(kind, ids) for kind, _, ids, _ in r] for l, r in t['rules'].items()},
                       rings=t['rings'], faces=t['faces'])


def subdiv_topology_creased(rec, levels, creases=None, corners=None):
    '''mpt_subdiv_topology_creased (no context, no GPU) of the records rec [3k,8] f32, the sharpnesses creases [k,3] and the flags
    corners [k,3] (either None): (verdict, words, tables) -- a refusal's verdict with the words of the refusal and None, else 0 with
    the block of 32-bit words and the tables decoded from it.  A rule is (kind, variant, [ids], parameter) -- the
    parameter the f64 f or s of a blending variant, else None; rules[l] and rings as subdiv_topology has them; records -- per record
    of the last level (vertex, kind, [ids]) --; faces [F_L,3] of record ids; words: the whole block'''
    rec, levels = _subdiv_records(rec), int(levels)
    k = rec.shape[0] // 3
    cr = None if creases is None else np.ascontiguousarray(creases, np.float32).reshape(k, 3)
    co = None if corners is None else np.ascontiguousarray(np.asarray(corners) != 0, np.uint8).reshape(k, 3)
    args = (fptr(rec), k, levels, None if cr is None else fptr(cr), None if co is None else co.ctypes.data_as(C.POINTER(C.c_uint8)))
    rc, got = _subdiv_call('mpt_subdiv_topology_creased', args, levels, 11)
    if rc:
        return rc, got, None
    return 0, got[2].copy(), _subdiv_decode(*got, levels)


def subdiv_topology_cc(rec, levels, polys=None, creases=None, corners=None):
    '''mpt_subdiv_topology_cc (no context, no GPU) of the records rec [3k,8] f32 -- the fans of the polygons polys [m] (None: every
    triangle a polygon) --, the sharpnesses creases and the flags corners, flat over the polygons' corners (either None):
    (verdict, words, tables) as subdiv_topology_creased.  counts [levels+1,3] are vertices, edges and faces (polygons at level 0,
    quads from level 1); rules[l] holds the vertices', the edges' and then the faces' rules of level l - 1 as (kind, variant, [ids],
    parameter), a Catmull-Clark rule with SUBDIV_CC in its variant: a face point's ids are its corners, an interior edge's a b and
    two face point ids, an interior vertex's its n neighbours, n face point ids and, blending between two creases, p q; quads1
    [Q_1,2] is the table of level-1 quads (first triangle of the polygon, n | i << 8); faces [2 Q_L,3] of record ids'''
    rec, levels = _subdiv_records(rec), int(levels)
    k = rec.shape[0] // 3
    po = None if polys is None else np.ascontiguousarray(polys, np.int32).reshape(-1)
    m = k if po is None else int(po.size)
    ncorners = 3 * k if po is None else int(np.clip(po, 0, None).sum())
    cr = None if creases is None else np.ascontiguousarray(creases, np.float32).reshape(-1)
    co = None if corners is None else np.ascontiguousarray(np.asarray(corners).reshape(-1) != 0, np.uint8)
    for name, a in (('creases', cr), ('corners', co)):
        if a is not None and a.size != ncorners:
            raise ValueError('%s must hold %d values, one per polygon corner, got %d' % (name, ncorners, a.size))
    args = (fptr(rec), k, levels, None if po is None else iptr(po), m, None if cr is None else fptr(cr),
            None if co is None else co.ctypes.data_as(C.POINTER(C.c_uint8)))
    rc, got = _subdiv_call('mpt_subdiv_topology_cc', args, levels, 12)
    if rc:
        return rc, got, None
    return 0, got[2].copy(), _subdiv_decode(*got, levels)


DISPLACE_MODES = ('normal', 'vector')                                   # include/miptina.h MPT_DISPLACE_NORMAL, _VECTOR
DISPLACE_CHANNELS = ('r', 'g', 'b', 'a', 'mean')                         # ... MPT_DISPLACE_R .. MPT_DISPLACE_MEAN
DISPLACE_MAX_UV = 2.0 ** 20                                              # csrc/displace_rule.h MPT_DISPLACE_MAX_UV


def displace_corners(faces, nverts):
    '''mpt_displace_corners (no context, no GPU): (verdict, corner [nverts]) of faces [F,3] -- per vertex the lowest index 3 g + c
    with faces[g][c] the vertex; verdict 0 accepts, 2 names an id out of range, 3 a vertex no face touches'''
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    corner = np.zeros(max(int(nverts), 1), np.int32)
    rc = load_library().mpt_displace_corners(iptr(f), f.shape[0], int(nverts), iptr(corner))
    return rc, corner[:max(int(nverts), 0)]


SCATTER_ALIGNS = ('normal', 'up')                                        # include/miptina.h MPT_SCATTER_ALIGN_NORMAL, _UP
# mpt_scatter_point (include/miptina.h): the sticky record of an instance, 48 bytes
SCATTER_POINT_DTYPE = np.dtype([('face', np.int32), ('pad', np.int32), ('b1', np.float64), ('b2', np.float64), ('scale', np.float64),
                                ('cy', np.float64), ('sy', np.float64)])


def scatter_params(scale=(1, 1), align='normal', up=(0, 1, 0), random_yaw=True, density=None, channel='mean'):
    '''mpt_scatter_params from ModelPool.add_scatter's keywords: the words are checked here, the numbers by the library'''
    if align not in SCATTER_ALIGNS:
        raise ValueError('align %r: one of %s' % (align, ', '.join(SCATTER_ALIGNS)))
    if channel not in DISPLACE_CHANNELS:
        raise ValueError('channel %r: one of %s' % (channel, ', '.join(DISPLACE_CHANNELS)))
    smin, smax = (float(scale), float(scale)) if np.ndim(scale) == 0 else (float(scale[0]), float(scale[1]))
    up = np.asarray(up, np.float64).reshape(-1)
    if up.size != 3:
        raise ValueError('up must have 3 components, got %d' % up.size)
    image = -1 if density is None else int(getattr(density, 'id', density))  # (an image.Image, or its id)
    if density is not None and image < 0:
        raise ValueError('density image id %d is negative' % image)
    return ScatterParams(smin, smax, (C.c_double * 3)(*up.tolist()), SCATTER_ALIGNS.index(align), int(bool(random_yaw)), image,
                         DISPLACE_CHANNELS.index(channel))


def scatter_rule(corners, q, seed, count, first=0, **params):
    '''mpt_scatter_rule (no context, no GPU): (verdict, records [count] of SCATTER_POINT_DTYPE, matrices [count,4,4]) of instances
    first .. first + count - 1 over world corners [F,3,3] with shares q [F]; the keywords of scatter_params'''
    p = scatter_params(**params)
    corners = np.ascontiguousarray(corners, np.float64).reshape(-1, 3, 3)
    q = np.ascontiguousarray(q, np.uint32).reshape(-1)
    if q.size != corners.shape[0]:
        raise ValueError('%d shares for %d faces' % (q.size, corners.shape[0]))
    points, worlds = np.zeros(max(int(count), 0), SCATTER_POINT_DTYPE), np.zeros((max(int(count), 0), 4, 4), np.float64)
    rc = load_library().mpt_scatter_rule(corners.ctypes.data_as(C.POINTER(C.c_double)), q.ctypes.data_as(C.POINTER(C.c_uint32)), corners.shape[0],
                                         C.byref(p), int(seed) & (2 ** 64 - 1), int(first), int(count), points.ctypes.data_as(C.c_void_p),
                                         worlds.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, points, worlds


SPACE_MAX_CANDIDATES = 1 << 24                                           # csrc/scatter_rule.h MPT_SPACE_MAX_CANDIDATES


def scatter_spacing(count, min_distance=0.0, candidates=None):
    '''(min_distance, candidates) of ModelPool.add_scatter's keywords as mpt_scatter_set_spacing takes them; candidates=None: 4 * count'''
    r = float(min_distance)
    if not np.isfinite(r) or r < 0:
        raise ValueError('the minimum distance %r is negative or not finite' % (min_distance,))
    m = 4 * int(count) if candidates is None else int(candidates)
    if r > 0 and not int(count) <= m <= SPACE_MAX_CANDIDATES:
        raise ValueError('%d candidates outside [%d, %d], the count and 2^24' % (m, count, SPACE_MAX_CANDIDATES))
    return r, m


def scatter_space_rule(points, r):
    '''mpt_scatter_space_rule (no context, no GPU): (verdict, kept [n] uint8, rounds of the synchronous form) of the elimination of
    points [n,3] at the minimum distance r'''
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    kept, rounds = np.zeros(points.shape[0], np.uint8), C.c_int32(0)
    rc = load_library().mpt_scatter_space_rule(points.ctypes.data_as(C.POINTER(C.c_double)), points.shape[0], float(r),
                                               kept.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(rounds))
    return rc, kept, rounds.value


def scatter_space_points(context, points, r):
    '''mpt_scatter_space_points, the test door: (kept [n] uint8, rounds) as the device's grid and round kernels make them'''
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    kept, rounds = np.zeros(points.shape[0], np.uint8), C.c_int32(0)
    context.call('mpt_scatter_space_points', points.ctypes.data_as(C.POINTER(C.c_double)), points.shape[0], float(r),
                 kept.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(rounds))
    return kept, rounds.value


def devices_isolated():
    '''True when the launcher shows each rank its own GPU(s) only (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES /
    CUDA_VISIBLE_DEVICES set per task, SLURM --gpus-per-task): LOCAL_RANK then does not index the visible devices'''
    return any(os.environ.get(k) for k in ('HIP_VISIBLE_DEVICES', 'ROCR_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES'))


def rank_device(ndev):
    '''the device of this rank: MIPTINA_DEVICE if given; LOCAL_RANK when the node's GPUs are all visible (a rank
    whose LOCAL_RANK has no device then fails in mpt_create -- "device out of range" -- instead of piling onto
    somebody else's GPU); device 0 when the launcher isolated ONE GPU per rank'''
    if os.environ.get('MIPTINA_DEVICE'):
        return int(os.environ['MIPTINA_DEVICE'])
    lr = int(os.environ.get('LOCAL_RANK', '0'))
    if ndev == 1 and lr > 0 and devices_isolated():
        return 0
    return lr


class Context:
    '''one device context = the reference's set of singletons (things.py:20-28)'''

    def __init__(self, device=None, **caps):
        lib = load_library()
        c = Caps(max_faces=2**21, max_texels=2**22, max_materials=2**6, max_textures=2**6,
                 max_lights=2**6, max_filmsize=2**21, max_filmpasses=3)
        for k, v in caps.items():
            setattr(c, k, int(v))
        self.caps = c
        if device is None:
            device = rank_device(lib.mpt_device_count())
        self.device = device
        self.lib = lib
        h = lib.mpt_create(C.byref(c), device)
        if not h:
            raise RuntimeError(last_error())
        self.h = C.c_void_p(h)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.mpt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def call(self, name, *args):
        check(getattr(self.lib, name)(self.h, *args))

    def set_option(self, key, value):
        self.call('mpt_set_option', key.encode(), int(value))

    def get_option(self, key):
        v = C.c_int(0)
        self.call('mpt_get_option', key.encode(), C.byref(v))
        return v.value

    def shade_variant(self):
        '''(feature mask, lean) of the SHADE stage the last render launch ran (mpt_get_shade_variant); (-1, -1) before the first'''
        feat, lean = C.c_int(0), C.c_int(0)
        self.call('mpt_get_shade_variant', C.byref(feat), C.byref(lean))
        return feat.value, lean.value

    def unit_eval(self, name, rows):
        '''test door (mpt_unit_eval): one device function of the hot path on rows of inputs, by the build the
        context's mode selects; rows f32 (i32 for the hash kinds), returns [n, out_cols] of the same type'''
        kind, nin, nout = UNIT_KINDS[name]
        dt = np.int32 if name.startswith('wanghash') else np.float32
        a = np.ascontiguousarray(np.asarray(rows, dt).reshape(-1, nin))
        out = np.zeros((a.shape[0], nout), dt)
        self.call('mpt_unit_eval', kind, a.ctypes.data_as(C.c_void_p), nin, out.ctypes.data_as(C.c_void_p), nout, a.shape[0])
        return out

    def display_eval(self, raw, nx, ny, **kw):
        '''test door (mpt_display_eval): get_display's metering and conversion kernels on the accumulators raw [nx*ny][4]; the
        keywords of display_params; returns (uint8 [nx, ny, 4] or, for layout='display', [ny, nx, 4]; the exposure used)'''
        p = display_params(**kw)
        a = np.ascontiguousarray(np.asarray(raw, np.float32).reshape(-1, 4))
        if a.shape[0] != int(nx) * int(ny):
            raise ValueError('raw holds %d accumulators, the film %dx%d' % (a.shape[0], nx, ny))
        out = np.zeros((ny, nx, 4) if p.layout == LAYOUTS['display'] else (nx, ny, 4), np.uint8)
        used = C.c_float(0)
        self.call('mpt_display_eval', C.byref(p), fptr(a), int(nx), int(ny), out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(used))
        return out, np.float32(used.value)

    def set_denoise_variance(self, variance):
        '''sigma_variance of the denoised read-backs that follow (mpt_denoise_set_variance): None or 0 = the fixed filter.
        FilmTable.get_denoised and get_display(denoised=True) set it before every call, so their callers never see the state'''
        self.call('mpt_denoise_set_variance', 0.0 if variance is None else float(variance))

    def get_denoise_variance(self):
        v = C.c_float(0)
        self.call('mpt_denoise_get_variance', C.byref(v))
        return v.value

    def denoise_eval(self, f0, f1, f2, mark, nx, ny, variance=None, var=False, **denoise_kw):
        '''test door (mpt_denoise_eval): get_denoised's launches on the accumulators f0, f1, f2 and -- guided, variance > 0 --
        mark [nx*ny][4]; the keywords of denoise_params.  Returns the image [nx, ny, 4], or with var=True (image, v_final [nx, ny])'''
        acc = [None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 4)) for a in (f0, f1, f2, mark)]
        if any(a is not None and a.shape[0] != int(nx) * int(ny) for a in acc):
            raise ValueError('the accumulators do not hold the %d pixels of the film %dx%d' % (int(nx) * int(ny), nx, ny))
        out = np.empty((nx, ny, 4), np.float32)
        v = np.empty((nx, ny), np.float32) if var else None
        self.call('mpt_denoise_eval', C.byref(denoise_params(who='denoise_eval', **denoise_kw)), 0.0 if variance is None else float(variance),
                  *(None if a is None else fptr(a) for a in acc), int(nx), int(ny), fptr(out), None if v is None else fptr(v))
        return (out, v) if var else out

    def noise_eval(self, film_raw, mark_raw, nx, ny, threshold, map=True, remark=True):
        '''test door (mpt_noise_eval): get_noise's kernels on the accumulators film_raw and mark_raw [nx*ny][4]; returns
        (NoiseResult with the map [nx, ny] or None, the mark the re-mark mode leaves [nx*ny, 4] or None)'''
        f = np.ascontiguousarray(np.asarray(film_raw, np.float32).reshape(-1, 4))
        m = np.ascontiguousarray(np.asarray(mark_raw, np.float32).reshape(-1, 4))
        if f.shape[0] != int(nx) * int(ny) or m.shape != f.shape:
            raise ValueError('film and mark hold %d and %d accumulators, the film %dx%d' % (f.shape[0], m.shape[0], nx, ny))
        e = np.empty((nx, ny), np.float32) if map else None
        new = np.empty_like(f) if remark else None
        st = NoiseStats()
        self.call('mpt_noise_eval', float(threshold), fptr(f), fptr(m), int(nx), int(ny), None if e is None else fptr(e),
                  None if new is None else fptr(new), C.byref(st))
        return NoiseResult(st, e), new

    def adapt_eval(self, film_raw, mark_raw, nx, ny, threshold, dilate=1):
        '''test door (mpt_adapt_eval): FilmTable.select's kernels on the accumulators film_raw and mark_raw [nx*ny][4]; returns
        (NoiseResult, the list int32[count])'''
        f = np.ascontiguousarray(np.asarray(film_raw, np.float32).reshape(-1, 4))
        m = np.ascontiguousarray(np.asarray(mark_raw, np.float32).reshape(-1, 4))
        if f.shape[0] != int(nx) * int(ny) or m.shape != f.shape:
            raise ValueError('film and mark hold %d and %d accumulators, the film %dx%d' % (f.shape[0], m.shape[0], nx, ny))
        out = np.empty(f.shape[0], np.int32)
        st, n = NoiseStats(), C.c_int(-1)
        self.call('mpt_adapt_eval', float(threshold), int(dilate), fptr(f), fptr(m), int(nx), int(ny), iptr(out), out.size, C.byref(n), C.byref(st))
        return NoiseResult(st), out[:n.value].copy()

    def history_eval(self, f_old, face, id, depth, motion, nx, ny, max_history=32.0, depth_tol=0.02):
        '''test door (mpt_history_eval): FilmTable.reproject's resample launch on the accumulators f_old [nx*ny][4], a kept
        G-buffer face, id (int32) and depth (f32) [nx*ny] and the motion records (MOTION_DTYPE [nx*ny]), the whole film as the
        share; returns (the new accumulators [nx*ny, 4], HistoryResult)'''
        n = int(nx) * int(ny)
        f = np.ascontiguousarray(np.asarray(f_old, np.float32).reshape(-1, 4))
        fa, ob = (np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1)) for a in (face, id))
        de = np.ascontiguousarray(np.asarray(depth, np.float32).reshape(-1))
        mo = np.ascontiguousarray(np.asarray(motion, MOTION_DTYPE).reshape(-1))
        if not (f.shape[0] == fa.size == ob.size == de.size == mo.size == n):
            raise ValueError('the arrays do not hold the %d pixels of the film %dx%d' % (n, nx, ny))
        out, st = np.empty_like(f), HistoryStats()
        self.call('mpt_history_eval', C.byref(history_params(max_history, depth_tol)), fptr(f), iptr(fa), iptr(ob), fptr(de),
                  mo.ctypes.data_as(C.c_void_p), int(nx), int(ny), fptr(out), C.byref(st))
        return out, HistoryResult(st)

    def counters(self):
        cnt = Counters()
        self.call('mpt_get_counters', C.byref(cnt))
        return cnt.asdict()

    def timer(self, symbol, segments=1):
        '''read out and reset one of the library's launch timers (mpt_*_kernel_time): (ms, launches) -- HIP-event time of the
        kernels of the launches since the last read-out -- or, for a timer of several segments, (ms0, ms1, ..., launches)'''
        ms, n = [C.c_double(0) for _ in range(segments)], C.c_int(0)
        self.call(symbol, *map(C.byref, ms), C.byref(n))
        return (*(m.value for m in ms), n.value)

    def kernel_time(self):
        return self.timer('mpt_kernel_time')


_ctx = None


def get_context(**caps):
    '''the process-wide context; created on first use (init_things passes capacities)'''
    global _ctx
    if _ctx is None:
        _ctx = Context(**caps)
    return _ctx


def have_context():
    return _ctx is not None


def drop_context():
    global _ctx
    if _ctx is not None:
        _ctx.close()
        _ctx = None

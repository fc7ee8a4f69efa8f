"""ctypes binding of the ptk C-ABI (include/ptk.h) — the MI355X render path.

There is NO CPU fallback here: if libptk.so (HIP kernels for gfx950 + host side) is missing or no
GPU is visible, loading / creating a context raises.  Scenes are dicts of numpy arrays in the
boundary's flat layout (see include/ptk.h `ptk_scene_desc`).
"""
from __future__ import annotations

import ctypes as C
import threading
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product loads the in-tree library, nothing else.  Only tools/*.sh (A/B of two builds inside one GPU-box call) point the
# binding at another build, and they have to say so twice: PTK_DEV_TOOLS=1 and PTK_LIB_PATH=<a libptk_*.so beside libptk.so>.
LIB_PATH = os.path.join(_HERE, "libptk.so")
if os.environ.get("PTK_DEV_TOOLS") == "1" and os.environ.get("PTK_LIB_PATH", "").startswith(os.path.join(_HERE, "libptk_")):
    LIB_PATH = os.environ["PTK_LIB_PATH"]

PTK_OK = 0
PTK_TILE = 16
PTK_MAX_BVH_DEPTH = 32

MATERIAL_DTYPE = np.dtype([
    ("type", np.int32), ("diffuse", np.float32, 3), ("specular", np.float32, 3),
    ("emissive", np.float32, 3), ("emissive_intensity", np.float32), ("roughness", np.float32),
    ("reflectiveness", np.float32), ("translucency", np.float32), ("ior", np.float32),
    ("tex", np.int32, 6)], align=False)
TEXTURE_DTYPE = np.dtype([("width", np.int32), ("height", np.int32), ("offset", np.int64)])
assert MATERIAL_DTYPE.itemsize == 84 and TEXTURE_DTYPE.itemsize == 16


class SceneDesc(C.Structure):
    _fields_ = [
        ("num_triangles", C.c_int32), ("verts", C.c_void_p), ("normals", C.c_void_p),
        ("uvs", C.c_void_p), ("tbn", C.c_void_p), ("smoothing", C.c_void_p), ("material", C.c_void_p),
        ("num_materials", C.c_int32), ("materials", C.c_void_p),
        ("num_textures", C.c_int32), ("textures", C.c_void_p), ("texels", C.c_void_p),
        ("texel_bytes", C.c_int64),
        ("num_lights", C.c_int32), ("lights", C.c_void_p),
    ]


class Stats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in
                ("samples", "rays", "shadow_rays", "node_visits", "tri_tests", "hits_shaded", "tex_fetches",
                 "walk_wave_iters", "walk_lane_iters", "shade_wave_execs", "shade_lanes", "gen_wave_execs", "gen_lanes",
                 "tri_wave_execs", "tri_lanes", "max_walk_nodes", "paths_started")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class AdaptiveResult(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("max_count", C.c_uint32), ("pixel_samples", C.c_uint64), ("active_pixels", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RaysAdaptiveResult(C.Structure):
    """ptk_rays_adaptive_result"""
    _fields_ = [("rounds", C.c_uint32), ("max_count", C.c_uint32), ("ray_samples", C.c_uint64), ("active_rays", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class DenoiseParams(C.Structure):
    """ptk_denoise_params"""
    _fields_ = [("iterations", C.c_int32), ("normal_squarings", C.c_int32), ("sigma_z", C.c_float), ("sigma_l", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class View(C.Structure):
    """ptk_view: pixel (column j, top-down row i) has the image point top_left + right*(delta_x*j) - up*(delta_y*i)"""
    _fields_ = [("pos", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("top_left", C.c_float * 3),
                ("delta_x", C.c_float), ("delta_y", C.c_float)]

    def as_dict(self):
        """float32 arrays and scalars, the struct's own bits"""
        d = {k: np.array(list(getattr(self, k)), np.float32) for k in ("pos", "right", "up", "top_left")}
        d.update(delta_x=np.float32(self.delta_x), delta_y=np.float32(self.delta_y))
        return d


class TemporalParams(C.Structure):
    """ptk_temporal_params"""
    _fields_ = [("max_plane_dist", C.c_float), ("min_normal_dot", C.c_float), ("max_history", C.c_float), ("match_id", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VarianceParams(C.Structure):
    """ptk_variance_params"""
    _fields_ = [("radius", C.c_int32), ("prefilter", C.c_int32), ("min_frames", C.c_float), ("max_plane_dist", C.c_float),
                ("min_normal_dot", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class UpsampleParams(C.Structure):
    """ptk_upsample_params"""
    _fields_ = [("max_plane_dist", C.c_float), ("min_normal_dot", C.c_float), ("wide", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DisplayParams(C.Structure):
    """ptk_display_params"""
    _fields_ = [("mode", C.c_int32), ("exposure", C.c_float), ("key", C.c_float), ("min_lum", C.c_float), ("max_lum", C.c_float),
                ("low_permille", C.c_int32), ("high_permille", C.c_int32), ("min_exposure", C.c_float), ("max_exposure", C.c_float),
                ("adapt", C.c_float), ("op", C.c_int32), ("white", C.c_float), ("transfer", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DisplayState(C.Structure):
    """ptk_exposure_state: the exposure state of the display transform as it lies in device memory"""
    _fields_ = [("exposure", C.c_float), ("target", C.c_float), ("lavg", C.c_float), ("has_prev", C.c_uint32),
                ("counted", C.c_uint64), ("kept", C.c_uint64)]

    def as_dict(self):
        """float32 scalars and ints, the struct's own bits"""
        d = {k: np.float32(getattr(self, k)) for k in ("exposure", "target", "lavg")}
        d.update({k: int(getattr(self, k)) for k in ("has_prev", "counted", "kept")})
        return d


class ReprojectDesc(C.Structure):
    """ptk_reproject_desc"""
    _fields_ = ([("width", C.c_int32), ("height", C.c_int32), ("hist_view", C.POINTER(View))]
                + [(k, C.c_void_p) for k in ("color", "count", "id", "position", "normal", "prev_position", "prev_normal", "albedo",
                                             "hist_color", "hist_count", "hist_id", "hist_position", "hist_normal", "hist_moments",
                                             "out_color", "out_count", "out_moments")])


class SurfaceAttrs(C.Structure):
    """ptk_surface_attrs: one pointer per attribute in id order, null = not computed"""
    _fields_ = [(k, C.c_void_p) for k in ("material", "uv", "position", "normal_geom", "normal", "albedo", "emission", "gloss", "opacity")]


class PtkError(RuntimeError):
    pass


_lib = None

# every symbol include/ptk.h declares
SYMBOLS = [
    "ptk_create", "ptk_destroy", "ptk_upload_scene", "ptk_update_materials", "ptk_set_camera", "ptk_set_frame", "ptk_set_tile",
    "ptk_reset", "ptk_render", "ptk_resolve_rgb8", "ptk_read_accum", "ptk_write_accum", "ptk_samples",
    "ptk_request_exit", "ptk_synchronize", "ptk_last_error", "ptk_accum_device_ptr", "ptk_rgb8_device_ptr",
    "ptk_bind_accum", "ptk_set_stream", "ptk_gather_accum", "ptk_set_option", "ptk_last_render_ms",
    "ptk_last_kernel_ms", "ptk_collect_stats",
    "ptk_bvh_info", "ptk_bvh_layout", "ptk_upload_timing", "ptk_download_bvh", "ptk_probe_hits", "ptk_probe_primary_dirs", "ptk_probe_math", "ptk_probe_direct", "ptk_host_alloc", "ptk_host_free",
    "ptk_packed_floats", "ptk_packed_layout", "ptk_comm_unique_id", "ptk_comm_init", "ptk_comm_destroy",
    "ptk_gather_wait", "ptk_read_gathered", "ptk_gathered_device_ptr", "ptk_probe_pack", "ptk_probe_unpack",
    "ptk_bind_out_image", "ptk_bind_out_device", "ptk_bind_gl_buffer", "ptk_comm_info", "ptk_kernel_log", "ptk_kernel_log_read",
    "ptk_debug_stall_exchange", "ptk_render_adaptive", "ptk_read_sample_counts", "ptk_read_moments",
    "ptk_trace_variant", "ptk_scene_is_plain", "ptk_scene_is_lambert", "ptk_trace_is_lambert", "ptk_trace_unit",
    "ptk_flat_zero_class", "ptk_flat_zero_mask", "ptk_flat_classes", "ptk_flat_rect_pair", "ptk_flat_rect_pairs",
    "ptk_feature_info", "ptk_render_features", "ptk_read_feature", "ptk_feature_device_ptr", "ptk_pick",
    "ptk_update_geometry", "ptk_update_geometry_device", "ptk_geometry_info", "ptk_geometry_timing",
    "ptk_trace_rays", "ptk_trace_rays_device", "ptk_last_rays_ms",
    "ptk_intersect_rays", "ptk_intersect_rays_device", "ptk_occluded_rays", "ptk_occluded_rays_device", "ptk_last_hits_ms",
    "ptk_closest_points", "ptk_closest_points_device", "ptk_last_closest_ms", "ptk_closest_stats",
    "ptk_crossings_rays", "ptk_crossings_rays_device", "ptk_contains_points", "ptk_contains_points_device",
    "ptk_inside_default_dirs", "ptk_signed_distance", "ptk_signed_distance_device", "ptk_last_crossings_ms",
    "ptk_multihit_rays", "ptk_multihit_rays_device", "ptk_last_multihit_ms",
    "ptk_overlap_boxes", "ptk_overlap_boxes_device", "ptk_overlap_spheres", "ptk_overlap_spheres_device", "ptk_last_overlap_ms",
    "ptk_overlap_stats",
    "ptk_nearest_triangles", "ptk_nearest_triangles_device", "ptk_last_nearest_ms", "ptk_nearest_stats",
    "ptk_surface_weights", "ptk_surface_weights_device", "ptk_sample_surface", "ptk_sample_surface_device", "ptk_surface_info",
    "ptk_last_surface_ms", "ptk_probe_surface_table", "ptk_probe_scan_u64",
    "ptk_attribute_info", "ptk_surface_attributes", "ptk_surface_attributes_device", "ptk_last_attributes_ms",
    "ptk_denoise_planes", "ptk_denoise_planes_device", "ptk_denoise_frame", "ptk_read_denoised", "ptk_denoised_device_ptr",
    "ptk_resolve_denoised_rgb8", "ptk_last_denoise_ms",
    "ptk_get_view", "ptk_reproject_planes", "ptk_reproject_planes_device", "ptk_temporal_frame", "ptk_read_temporal",
    "ptk_temporal_device_ptr", "ptk_last_temporal_ms",
    "ptk_geometry_snapshot", "ptk_render_motion", "ptk_read_motion", "ptk_motion_device_ptr", "ptk_reproject_planes_moving",
    "ptk_reproject_planes_moving_device", "ptk_temporal_frame_moving", "ptk_last_motion_ms",
    "ptk_reproject_moments", "ptk_reproject_moments_device", "ptk_temporal_frame_moments", "ptk_variance_planes",
    "ptk_variance_planes_device", "ptk_temporal_variance", "ptk_read_temporal_variance", "ptk_temporal_variance_device_ptr",
    "ptk_denoise_temporal", "ptk_last_variance_ms",
    "ptk_display_planes", "ptk_display_planes_device", "ptk_display_frame", "ptk_read_display", "ptk_display_device_ptr",
    "ptk_display_state", "ptk_display_reset", "ptk_display_srgb_table", "ptk_display_check_params", "ptk_last_display_ms",
    "ptk_render_guides", "ptk_read_guide", "ptk_guide_device_ptr", "ptk_guide_view", "ptk_upsample_planes",
    "ptk_upsample_planes_device", "ptk_upsample_frame", "ptk_read_upsampled", "ptk_upsampled_device_ptr", "ptk_last_upsample_ms",
    "ptk_bake_coverage", "ptk_bake_lightmap", "ptk_bake_lightmap_device", "ptk_lightmap_dilate", "ptk_lightmap_dilate_device",
    "ptk_last_bake_ms",
    "ptk_trace_rays_adaptive", "ptk_trace_rays_adaptive_device", "ptk_bake_lightmap_adaptive", "ptk_bake_lightmap_adaptive_device",
    "ptk_last_rays_adaptive_ms",
    "ptk_bake_probes", "ptk_bake_probes_device", "ptk_probes_irradiance", "ptk_probes_irradiance_device", "ptk_last_probes_ms",
    "ptk_bake_probe_visibility", "ptk_bake_probe_visibility_device", "ptk_probes_irradiance_visible",
    "ptk_probes_irradiance_visible_device", "ptk_last_probe_visibility_ms",
]


_load_lock = threading.Lock()


def load() -> C.CDLL:
    """Load libptk.so; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is not None:
        return _lib
    with _load_lock:                 # (two threads' first calls: ONE library object gets the prototypes, everybody uses that one)
        return _load_locked()


def _load_locked() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PtkError(f"{LIB_PATH} not found: the HIP extension is not built (run __graft_entry__.build()); "
                       "there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, u64, f32 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_float
    fp = C.POINTER(C.c_float)
    L.ptk_create.argtypes = [C.POINTER(vp), i32]
    L.ptk_destroy.argtypes = [vp]; L.ptk_destroy.restype = None
    L.ptk_upload_scene.argtypes = [vp, C.POINTER(SceneDesc)]
    L.ptk_update_materials.argtypes = [vp, i32, vp]
    L.ptk_set_camera.argtypes = [vp, fp, fp, fp, f32, f32, f32, f32]
    L.ptk_set_frame.argtypes = [vp, i32, i32, i32]
    L.ptk_set_tile.argtypes = [vp, i32, i32]
    L.ptk_reset.argtypes = [vp]
    L.ptk_render.argtypes = [vp, u32, u32, u64]
    L.ptk_resolve_rgb8.argtypes = [vp, vp]
    L.ptk_read_accum.argtypes = [vp, vp]
    L.ptk_host_alloc.restype = vp; L.ptk_host_alloc.argtypes = [C.c_size_t]
    L.ptk_host_free.restype = None; L.ptk_host_free.argtypes = [vp]
    L.ptk_write_accum.argtypes = [vp, vp, i32]
    L.ptk_samples.argtypes = [vp]
    L.ptk_request_exit.argtypes = [vp]
    L.ptk_synchronize.argtypes = [vp]
    L.ptk_last_error.argtypes = [vp]; L.ptk_last_error.restype = C.c_char_p
    L.ptk_accum_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.ptk_rgb8_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.ptk_bind_accum.argtypes = [vp, vp]
    L.ptk_set_stream.argtypes = [vp, vp]
    L.ptk_gather_accum.argtypes = [vp, vp, i32]
    L.ptk_packed_floats.argtypes = [i32, i32, i32, i32]; L.ptk_packed_floats.restype = C.c_int64
    L.ptk_packed_layout.argtypes = [i32, i32, i32, i32, vp]
    L.ptk_comm_unique_id.argtypes = [vp]
    L.ptk_comm_init.argtypes = [vp, vp, i32, i32]
    L.ptk_comm_destroy.argtypes = [vp]
    L.ptk_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.ptk_bind_out_image.argtypes = [vp, vp]
    L.ptk_bind_out_device.argtypes = [vp, vp]
    L.ptk_bind_gl_buffer.argtypes = [vp, C.c_uint]
    L.ptk_gather_wait.argtypes = [vp]
    L.ptk_read_gathered.argtypes = [vp, vp]
    L.ptk_gathered_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.ptk_probe_pack.argtypes = [vp, i32, i32, vp]
    L.ptk_probe_unpack.argtypes = [vp, i32, vp, vp]
    L.ptk_last_render_ms.argtypes = [vp, fp, C.POINTER(i32)]
    L.ptk_last_kernel_ms.argtypes = [vp, fp, fp]
    L.ptk_set_option.argtypes = [vp, C.c_char_p, C.c_double]
    L.ptk_collect_stats.argtypes = [vp, u32, u32, u64, C.POINTER(Stats)]
    L.ptk_render_adaptive.argtypes = [vp, f32, u32, u32, u32, u64, C.POINTER(AdaptiveResult)]
    L.ptk_read_sample_counts.argtypes = [vp, vp]
    L.ptk_read_moments.argtypes = [vp, vp]
    try:
        L.ptk_kernel_log.argtypes = [vp, i32]
        L.ptk_kernel_log_read.argtypes = [vp, C.POINTER(C.c_float), i32, C.POINTER(C.c_int)]
        L.ptk_debug_stall_exchange.argtypes = [vp, i32]
        L.ptk_trace_variant.argtypes = [vp, C.POINTER(C.c_int)]
        L.ptk_scene_is_plain.argtypes = [C.POINTER(SceneDesc)]
        for fn in (L.ptk_trace_rays, L.ptk_trace_rays_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, i32, u32, u32, u64, u32, u32, vp]
        L.ptk_last_rays_ms.argtypes = [vp, fp, fp]
        L.ptk_bake_coverage.argtypes = [vp, i32, i32, vp, vp, vp, vp]
        for fn in (L.ptk_bake_lightmap, L.ptk_bake_lightmap_device):
            fn.argtypes = [vp, i32, i32, vp, f32, i32, u32, u32, u64, u32, u32, vp, vp]
        for fn in (L.ptk_lightmap_dilate, L.ptk_lightmap_dilate_device):
            fn.argtypes = [vp, i32, i32, i32, vp, vp]
        L.ptk_last_bake_ms.argtypes = [vp, fp, fp, fp, fp]
        for fn in (L.ptk_bake_probes, L.ptk_bake_probes_device):
            fn.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, i32, u32, u32, u64, u32, u32, f32, vp, vp]
        for fn in (L.ptk_probes_irradiance, L.ptk_probes_irradiance_device):
            fn.argtypes = [vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp]
        L.ptk_last_probes_ms.argtypes = [vp, fp, fp, fp]
        for fn in (L.ptk_bake_probe_visibility, L.ptk_bake_probe_visibility_device):
            fn.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, i32, f32, u32, u64, u32, vp, vp]
        for fn in (L.ptk_probes_irradiance_visible, L.ptk_probes_irradiance_visible_device):
            fn.argtypes = [vp, vp, vp, vp, vp, i32, vp, f32, C.c_int32, vp, vp, vp]
        L.ptk_last_probe_visibility_ms.argtypes = [vp, fp, fp, fp]
        for fn in (L.ptk_trace_rays_adaptive, L.ptk_trace_rays_adaptive_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, i32, f32, u32, u32, u32, u64, u32, u32, vp, vp, vp, C.POINTER(RaysAdaptiveResult)]
        for fn in (L.ptk_bake_lightmap_adaptive, L.ptk_bake_lightmap_adaptive_device):
            fn.argtypes = [vp, i32, i32, vp, f32, i32, f32, u32, u32, u32, u64, u32, u32, vp, vp, vp, C.POINTER(RaysAdaptiveResult)]
        L.ptk_last_rays_adaptive_ms.argtypes = [vp, fp, fp, fp]
        for fn in (L.ptk_intersect_rays, L.ptk_intersect_rays_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, u32, u64, u32, vp, vp, vp, vp]
        for fn in (L.ptk_occluded_rays, L.ptk_occluded_rays_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, vp, u32, u64, u32, vp]
        L.ptk_last_hits_ms.argtypes = [vp, fp]
        for fn in (L.ptk_closest_points, L.ptk_closest_points_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp]
        L.ptk_last_closest_ms.argtypes = [vp, fp]
        L.ptk_closest_stats.argtypes = [vp, C.c_int32, vp, vp, C.POINTER(u64), C.POINTER(u64)]
        for fn in (L.ptk_crossings_rays, L.ptk_crossings_rays_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp]
        for fn in (L.ptk_contains_points, L.ptk_contains_points_device):
            fn.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, C.c_int32, vp, vp]
        L.ptk_inside_default_dirs.argtypes = [vp]
        for fn in (L.ptk_signed_distance, L.ptk_signed_distance_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, vp]
        L.ptk_last_crossings_ms.argtypes = [vp, fp]
        for fn in (L.ptk_multihit_rays, L.ptk_multihit_rays_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
        L.ptk_last_multihit_ms.argtypes = [vp, fp]
        for fn in (L.ptk_overlap_boxes, L.ptk_overlap_boxes_device, L.ptk_overlap_spheres, L.ptk_overlap_spheres_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp]
        L.ptk_last_overlap_ms.argtypes = [vp, fp]
        L.ptk_overlap_stats.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, C.POINTER(u64)]
        for fn in (L.ptk_nearest_triangles, L.ptk_nearest_triangles_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
        L.ptk_last_nearest_ms.argtypes = [vp, fp]
        L.ptk_nearest_stats.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, C.POINTER(u64), C.POINTER(u64)]
        for fn in (L.ptk_surface_weights, L.ptk_surface_weights_device):
            fn.argtypes = [vp, vp]
        for fn in (L.ptk_sample_surface, L.ptk_sample_surface_device):
            fn.argtypes = [vp, C.c_int32, u32, u32, u64, vp, vp, vp, vp, vp]
        L.ptk_surface_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), fp]
        L.ptk_last_surface_ms.argtypes = [vp, fp, fp]
        L.ptk_probe_surface_table.argtypes = [vp, vp]
        L.ptk_probe_scan_u64.argtypes = [vp, C.c_int32, vp, vp, C.c_int32]
        L.ptk_attribute_info.argtypes = [i32, C.POINTER(i32), C.POINTER(i32)]
        for fn in (L.ptk_surface_attributes, L.ptk_surface_attributes_device):
            fn.argtypes = [vp, C.c_int32, vp, vp, vp, C.POINTER(SurfaceAttrs)]
        L.ptk_last_attributes_ms.argtypes = [vp, fp]
        for fn in (L.ptk_denoise_planes, L.ptk_denoise_planes_device):
            fn.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(DenoiseParams), vp, vp]
        L.ptk_denoise_frame.argtypes = [vp, C.POINTER(DenoiseParams), u32]
        L.ptk_read_denoised.argtypes = [vp, vp]
        L.ptk_denoised_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.ptk_resolve_denoised_rgb8.argtypes = [vp, vp]
        L.ptk_last_denoise_ms.argtypes = [vp, fp, fp, fp]
        L.ptk_get_view.argtypes = [vp, C.POINTER(View)]
        for fn in (L.ptk_reproject_planes, L.ptk_reproject_planes_device):
            fn.argtypes = [vp, i32, i32, C.POINTER(View)] + [vp] * 10 + [C.POINTER(TemporalParams), vp, vp]
        L.ptk_temporal_frame.argtypes = [vp, C.POINTER(TemporalParams), u32]
        L.ptk_read_temporal.argtypes = [vp, vp, vp]
        L.ptk_temporal_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.ptk_last_temporal_ms.argtypes = [vp, fp, fp]
        L.ptk_geometry_snapshot.argtypes = [vp]
        L.ptk_render_motion.argtypes = [vp, C.POINTER(View)]
        L.ptk_read_motion.argtypes = [vp, vp, vp, vp]
        L.ptk_motion_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]
        for fn in (L.ptk_reproject_planes_moving, L.ptk_reproject_planes_moving_device):
            fn.argtypes = [vp, i32, i32, C.POINTER(View)] + [vp] * 12 + [C.POINTER(TemporalParams), vp, vp]
        L.ptk_temporal_frame_moving.argtypes = [vp, C.POINTER(TemporalParams), u32]
        L.ptk_last_motion_ms.argtypes = [vp, fp, fp]
        for fn in (L.ptk_reproject_moments, L.ptk_reproject_moments_device):
            fn.argtypes = [vp, C.POINTER(ReprojectDesc), C.POINTER(TemporalParams)]
        L.ptk_temporal_frame_moments.argtypes = [vp, C.POINTER(TemporalParams), u32]
        for fn in (L.ptk_variance_planes, L.ptk_variance_planes_device):
            fn.argtypes = [vp, i32, i32] + [vp] * 6 + [C.POINTER(VarianceParams), vp]
        L.ptk_temporal_variance.argtypes = [vp, C.POINTER(VarianceParams)]
        L.ptk_read_temporal_variance.argtypes = [vp, vp, vp]
        L.ptk_temporal_variance_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.ptk_denoise_temporal.argtypes = [vp, C.POINTER(DenoiseParams), u32]
        L.ptk_last_variance_ms.argtypes = [vp, fp, fp]
        for fn in (L.ptk_display_planes, L.ptk_display_planes_device):
            fn.argtypes = [vp, i32, i32, vp, C.POINTER(DisplayParams), vp, vp]
        L.ptk_display_frame.argtypes = [vp, i32, C.POINTER(DisplayParams)]
        L.ptk_read_display.argtypes = [vp, vp]
        L.ptk_display_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.ptk_display_state.argtypes = [vp, C.POINTER(DisplayState)]
        L.ptk_display_reset.argtypes = [vp]
        L.ptk_display_srgb_table.argtypes = [vp]
        L.ptk_display_check_params.argtypes = [C.POINTER(DisplayParams)]
        L.ptk_last_display_ms.argtypes = [vp, fp, fp, fp]
        L.ptk_render_guides.argtypes = [vp, i32, i32, u32, u64, u32]
        L.ptk_read_guide.argtypes = [vp, i32, vp]
        L.ptk_guide_device_ptr.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.ptk_guide_view.argtypes = [vp, C.POINTER(View)]
        for fn in (L.ptk_upsample_planes, L.ptk_upsample_planes_device):
            fn.argtypes = [vp, i32, i32] + [vp] * 5 + [i32, i32] + [vp] * 4 + [C.POINTER(UpsampleParams), vp, vp]
        L.ptk_upsample_frame.argtypes = [vp, i32, C.POINTER(UpsampleParams)]
        L.ptk_read_upsampled.argtypes = [vp, vp, vp]
        L.ptk_upsampled_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ptk_last_upsample_ms.argtypes = [vp, fp, fp]
        L.ptk_scene_is_lambert.argtypes = [C.POINTER(SceneDesc)]
        L.ptk_trace_is_lambert.argtypes = [vp, C.POINTER(C.c_int)]
        L.ptk_trace_unit.argtypes = [vp, C.POINTER(C.c_int)]
        L.ptk_flat_zero_class.argtypes = [C.POINTER(C.c_float)]
        L.ptk_flat_zero_mask.argtypes = [C.c_int]
        L.ptk_flat_classes.argtypes = [vp, C.POINTER(i32)]
        L.ptk_flat_rect_pair.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.ptk_flat_rect_pairs.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    except AttributeError:
        if LIB_PATH.endswith("libptk.so"):      # (an older build loaded through PTK_DEV_TOOLS for an A/B may lack the newest entry points)
            raise
    L.ptk_feature_info.argtypes = [i32, C.POINTER(i32), C.POINTER(i32)]
    L.ptk_render_features.argtypes = [vp, u32, u64, u32]
    L.ptk_read_feature.argtypes = [vp, i32, vp]
    L.ptk_feature_device_ptr.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.ptk_pick.argtypes = [vp, i32, i32, u64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    L.ptk_update_geometry.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.ptk_update_geometry_device.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.ptk_geometry_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ptk_geometry_timing.argtypes = [vp, C.POINTER(C.c_float)]
    L.ptk_bvh_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ptk_bvh_layout.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ptk_download_bvh.argtypes = [vp, vp, vp]
    L.ptk_upload_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.ptk_probe_hits.argtypes = [vp, i32, vp, vp, vp, vp]
    L.ptk_probe_math.argtypes = [vp, i32, i32, vp, vp]
    L.ptk_probe_direct.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.ptk_probe_primary_dirs.argtypes = [vp, vp]
    _lib = L
    return L


TRACE_NONE, TRACE_BVH, TRACE_FLAT, TRACE_FLAT_PLAIN = 0, 1, 2, 3      # ptk_trace_variant
UNIT_NONE, UNIT_PLAIN, UNIT_RECT, UNIT_CYCLE = 0, 1, 2, 3              # ptk_trace_unit
RAYS_ACCUMULATE, RAYS_LENS_DRAWS = 1, 2                               # ptk_trace_rays flags
BAKE_ACCUMULATE, BAKE_BACK = 1, 2                                     # ptk_bake_lightmap flags
PROBES_ACCUMULATE = 1                                                 # ptk_bake_probes flags
DENOISE_VARIANCE = 1                                                  # ptk_denoise_frame flags
INSIDE_WINDING, INSIDE_PARITY = 0, 1                                  # ptk_contains_points / ptk_signed_distance modes
OVERLAP_MAX_K = 16                                                    # PTK_OVERLAP_MAX_K: the most indices an overlap query lists per call
OVERLAP_BOX, OVERLAP_SPHERE = 0, 1                                    # PTK_OVERLAP_BOX, PTK_OVERLAP_SPHERE (ptk_overlap_stats' shape)
NEAREST_MAX_K = 16                                                    # PTK_NEAREST_MAX_K: the most triangles ptk_nearest_triangles keeps per point
MULTIHIT_MAX = 16                                                 # PTK_MULTIHIT_MAX: the most entries ptk_multihit_rays keeps per ray
SURFACE_SCAN_ITEMS = 4096                                             # PTK_SURFACE_SCAN_ITEMS: items per workgroup of the table's prefix sum
INSIDE_MODES = {"winding": INSIDE_WINDING, "parity": INSIDE_PARITY}


def inside_default_dirs() -> np.ndarray:
    """[3, 3] float32: the built-in direction set of ptk_contains_points (ptk_inside_default_dirs; no device needed)."""
    out = np.zeros((3, 3), np.float32)
    if load().ptk_inside_default_dirs(out.ctypes.data) != PTK_OK:
        raise PtkError("ptk_inside_default_dirs failed")
    return out


def inside_mode(mode) -> int:
    """PTK_INSIDE_* of a mode given by name ("winding", "parity") or by value; raises PtkError for an unknown one."""
    m = INSIDE_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if m not in (INSIDE_WINDING, INSIDE_PARITY):
        raise PtkError(f"unknown inside mode {mode!r}")
    return int(m)


def denoise_defaults(extent: float, variance: bool = False, iterations: int = 5) -> DenoiseParams:
    """The documented default parameters of the denoiser for a scene whose bounding box has the diagonal `extent`
    (world units): 5 iterations (a 61-pixel footprint), normal weight max(0, dot)^32, sigma_z = extent / 64, and sigma_l = 0.25 in
    luminance of the demodulated image - or, for the variance-guided mode, 2 standard deviations of the pixel's value."""
    return DenoiseParams(int(iterations), 5, float(extent) / 64.0, 2.0 if variance else 0.25)


def _denoise_params(params) -> DenoiseParams:
    if isinstance(params, DenoiseParams):
        return params
    return DenoiseParams(int(params["iterations"]), int(params["normal_squarings"]), float(params["sigma_z"]), float(params["sigma_l"]))


EXPOSURE_MANUAL, EXPOSURE_METERED = 0, 1                              # ptk_display_params.mode
DISPLAY_LINEAR, DISPLAY_REINHARD, DISPLAY_ACES = 0, 1, 2              # ... .op
TRANSFER_LINEAR, TRANSFER_SRGB = 0, 1                                 # ... .transfer
DISPLAY_ACCUM, DISPLAY_DENOISED, DISPLAY_TEMPORAL = 0, 1, 2           # ptk_display_frame source
_DISPLAY_FIELDS = tuple(k for k, _ in DisplayParams._fields_)


def display_defaults(**overrides) -> DisplayParams:
    """The documented default parameters of the display transform: metered exposure that brings the average of
    the histogram's ranks 100 .. 950 permille to the key 0.18, luminances 2^-20 .. 2^20 counted, the exposure held in
    2^-10 .. 2^10, adapt 1 (no lag), the ACES curve and the sRGB transfer; manual exposure 1 and white 4 for the modes that use
    them.  Keyword arguments replace fields."""
    p = DisplayParams(EXPOSURE_METERED, 1.0, 0.18, 2.0 ** -20, 2.0 ** 20, 100, 950, 2.0 ** -10, 2.0 ** 10, 1.0, DISPLAY_ACES, 4.0,
                      TRANSFER_SRGB)
    for k, v in overrides.items():
        assert k in _DISPLAY_FIELDS, k
        setattr(p, k, v)
    return p


def _display_params(params) -> DisplayParams:
    if isinstance(params, DisplayParams):
        return params
    if params is None:
        return display_defaults()
    return DisplayParams(*(params[k] for k in _DISPLAY_FIELDS))


def display_srgb_table() -> np.ndarray:
    """ptk_display_srgb_table: the 256 float32 thresholds that define the SRGB transfer; needs no device."""
    out = np.empty(256, np.float32)
    rc = load().ptk_display_srgb_table(out.ctypes.data)
    if rc != PTK_OK:
        raise PtkError(f"ptk_display_srgb_table failed ({rc})")
    return out


def display_check_params(params) -> int:
    """ptk_display_check_params: PTK_OK or the code the display entries refuse `params` with; needs no device."""
    return int(load().ptk_display_check_params(C.byref(_display_params(params))))


UPSAMPLE_ACCUM, UPSAMPLE_DENOISED, UPSAMPLE_TEMPORAL = 0, 1, 2        # ptk_upsample_frame source
UPSAMPLE_GUIDES = (1 << 2) | (1 << 4) | (1 << 6) | (1 << 7)           # MATERIAL, POSITION, NORMAL, ALBEDO: what upsample_frame needs


def upsample_defaults(extent: float) -> UpsampleParams:
    """The documented default parameters of guided upsampling for a scene whose bounding box has the diagonal
    `extent` (world units): a low-resolution tap counts within 1 % of the extent of the pixel's tangent plane and with a normal
    within about 26 degrees (dot >= 0.9), as temporal_defaults has them; ring 1 is on."""
    return UpsampleParams(float(extent) / 100.0, 0.9, 1)


def _upsample_params(params) -> UpsampleParams:
    if isinstance(params, UpsampleParams):
        return params
    return UpsampleParams(float(params["max_plane_dist"]), float(params["min_normal_dot"]), int(params["wide"]))


TEMPORAL_RESET = 1                                                    # ptk_temporal_frame flags
TEMPORAL_MOVING = 2                                                   # ... and ptk_temporal_frame_moments' own


def temporal_defaults(extent: float) -> TemporalParams:
    """The documented default parameters of temporal reprojection for a scene whose bounding box has the diagonal
    `extent` (world units): a history tap counts within 1 % of the extent of the pixel's tangent plane and with a normal within
    about 26 degrees (dot >= 0.9), carrying the same id; the history weighs at most 64 samples."""
    return TemporalParams(float(extent) / 100.0, 0.9, 64.0, 1)


def _temporal_params(params) -> TemporalParams:
    if isinstance(params, TemporalParams):
        return params
    return TemporalParams(float(params["max_plane_dist"]), float(params["min_normal_dot"]), float(params["max_history"]), int(params["match_id"]))


def variance_defaults(extent: float) -> VarianceParams:
    """The documented default parameters of the temporal variance for a scene whose bounding box has the diagonal
    `extent`: a 7x7 window for the spatial estimate, the 3x3 prefilter, the spatial estimate below 4 frames of history, and the
    plane and normal thresholds of temporal_defaults."""
    return VarianceParams(3, 1, 4.0, float(extent) / 100.0, 0.9)


def _variance_params(params) -> VarianceParams:
    if isinstance(params, VarianceParams):
        return params
    return VarianceParams(int(params["radius"]), int(params["prefilter"]), float(params["min_frames"]), float(params["max_plane_dist"]),
                          float(params["min_normal_dot"]))


def _view(view) -> View:
    """a View, or a dict of its fields (tests/temporal_rule.py view_of)"""
    if isinstance(view, View):
        return view
    f3 = C.c_float * 3
    return View(f3(*map(float, view["pos"])), f3(*map(float, view["right"])), f3(*map(float, view["up"])), f3(*map(float, view["top_left"])),
                float(view["delta_x"]), float(view["delta_y"]))


# first-hit feature planes (ptk_render_features): ids, and their names in id order
(FEAT_DEPTH, FEAT_TRIANGLE, FEAT_MATERIAL, FEAT_BARY, FEAT_POSITION, FEAT_NORMAL_GEOM, FEAT_NORMAL, FEAT_ALBEDO, FEAT_EMISSION,
 FEAT_GLOSS) = range(10)
FEAT_NAMES = ("depth", "triangle", "material", "bary", "position", "normal_geom", "normal", "albedo", "emission", "gloss")
FEAT_ALL = (1 << len(FEAT_NAMES)) - 1


def feature_info(feature: int):
    """(channels, is_int) of a feature plane (ptk_feature_info; no device needed); raises for an unknown id."""
    ch = C.c_int(0); isint = C.c_int(0)
    if load().ptk_feature_info(int(feature), C.byref(ch), C.byref(isint)) != PTK_OK:
        raise PtkError(f"ptk_feature_info: unknown feature {feature}")
    return ch.value, bool(isint.value)


def feature_array(feature: int, width: int, height: int) -> np.ndarray:
    """An empty host array of a feature plane's shape and type: [H, W] or [H, W, c], float32 or int32."""
    ch, isint = feature_info(feature)
    return np.empty((height, width) if ch == 1 else (height, width, ch), np.int32 if isint else np.float32)


# surface attributes (ptk_surface_attributes): ids, and their names in id order
(ATTR_MATERIAL, ATTR_UV, ATTR_POSITION, ATTR_NORMAL_GEOM, ATTR_NORMAL, ATTR_ALBEDO, ATTR_EMISSION, ATTR_GLOSS, ATTR_OPACITY) = range(9)
ATTR_NAMES = ("material", "uv", "position", "normal_geom", "normal", "albedo", "emission", "gloss", "opacity")
ATTR_ALL = (1 << len(ATTR_NAMES)) - 1


def attribute_info(attr: int):
    """(channels, is_int) of a surface attribute (ptk_attribute_info; no device needed); raises for an unknown id."""
    ch = C.c_int(0); isint = C.c_int(0)
    if load().ptk_attribute_info(int(attr), C.byref(ch), C.byref(isint)) != PTK_OK:
        raise PtkError(f"ptk_attribute_info: unknown attribute {attr}")
    return ch.value, bool(isint.value)


def attribute_array(attr: int, n: int) -> np.ndarray:
    """An empty host array of a surface attribute's shape and type for n queries: [n] or [n, c], float32 or int32."""
    ch, isint = attribute_info(attr)
    return np.empty((n,) if ch == 1 else (n, ch), np.int32 if isint else np.float32)


def scene_is_plain(arrays: dict) -> bool:
    """ptk_scene_is_plain on a scene's arrays: the table half of the PLAIN-kernel predicate (no device needed)."""
    a = normalise_arrays(arrays)
    d = scene_desc(a)
    return bool(load().ptk_scene_is_plain(C.byref(d)))


def scene_is_lambert(arrays: dict) -> bool:
    """ptk_scene_is_lambert on a scene's arrays: plain, and no material has reflectiveness > 0 (no device needed)."""
    a = normalise_arrays(arrays)
    d = scene_desc(a)
    return bool(load().ptk_scene_is_lambert(C.byref(d)))


def flat_zero_class(v1, v2, v3) -> int:
    """ptk_flat_zero_class of the record the packers store for a triangle: edges v2 - v1, v3 - v1 in float32 (no device needed)."""
    v1, v2, v3 = (np.asarray(v, np.float32) for v in (v1, v2, v3))
    e = np.concatenate([v2 - v1, v3 - v1]).astype(np.float32)
    return int(load().ptk_flat_zero_class((C.c_float * 6)(*e.tolist())))


def flat_rect_pair(tri_a, tri_b) -> int:
    """ptk_flat_rect_pair of the records the packers store for two triangles (each three vertices): 1..6, or 0 for no pair (no device needed)."""
    recs = []
    for t in (tri_a, tri_b):
        v1, v2, v3 = (np.asarray(v, np.float32) for v in t)
        recs.append(np.concatenate([v1, v2 - v1, v3 - v1]).astype(np.float32))
    return int(load().ptk_flat_rect_pair((C.c_float * 9)(*recs[0].tolist()), (C.c_float * 9)(*recs[1].tolist())))


def flat_rect_prefix(verts) -> list:
    """The kinds of the pair prefix of a flat list ([n, 9] vertices in triangle order) by the rule the device applies
    (classify_flat_kernel): pairs of records 2k, 2k + 1 from the front for as long as ptk_flat_rect_pair holds (no device needed)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3, 3)
    kinds = []
    for k in range(0, min(len(v), 16) - 1, 2):
        kind = flat_rect_pair(v[k], v[k + 1])
        if kind == 0:
            break
        kinds.append(kind)
    return kinds


def flat_zero_mask(zero_class: int) -> int:
    """The 6-bit mask over (e1.x e1.y e1.z e2.x e2.y e2.z) a class stands for; -1 outside 0..15."""
    return int(load().ptk_flat_zero_mask(int(zero_class)))


def normalise_arrays(a: dict) -> dict:
    n = len(a["verts"])
    return {
        "verts": np.ascontiguousarray(a["verts"], dtype=np.float32).reshape(n, 9),
        "normals": np.ascontiguousarray(a["normals"], dtype=np.float32).reshape(n, 9),
        "uvs": np.ascontiguousarray(a["uvs"], dtype=np.float32).reshape(n, 6),
        "tbn": np.ascontiguousarray(a["tbn"], dtype=np.float32).reshape(n, 9),
        "smoothing": np.ascontiguousarray(a["smoothing"], dtype=np.uint8).reshape(n),
        "material": np.ascontiguousarray(a["material"], dtype=np.int32).reshape(n),
        "materials": np.ascontiguousarray(a["materials"], dtype=MATERIAL_DTYPE),
        "textures": np.ascontiguousarray(a.get("textures", np.zeros(0, TEXTURE_DTYPE)), dtype=TEXTURE_DTYPE),
        "texels": np.ascontiguousarray(a.get("texels", np.zeros(0, np.uint8)), dtype=np.uint8),
        "lights": np.ascontiguousarray(a["lights"], dtype=np.int32),
    }


def scene_desc(a: dict) -> SceneDesc:
    d = SceneDesc()
    d.num_triangles = len(a["verts"])
    for k in ("verts", "normals", "uvs", "tbn", "smoothing", "material", "materials", "textures", "texels", "lights"):
        setattr(d, k, a[k].ctypes.data if a[k].size else None)
    d.num_materials = len(a["materials"])
    d.num_textures = len(a["textures"])
    d.texel_bytes = a["texels"].size
    d.num_lights = len(a["lights"])
    return d


class Context:
    """One GPU, one HIP stream (ptk_ctx)."""

    def __init__(self, device: int = 0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.ptk_create(C.byref(h), device)
        if rc != PTK_OK:
            raise PtkError(f"ptk_create(device={device}) failed with {rc}: no usable MI355X / HIP device")
        self.h = h
        self.width = self.height = 0
        self._keep = None

    def _chk(self, rc: int, what: str):
        if rc != PTK_OK:
            raise PtkError(f"{what} failed ({rc}): {self.L.ptk_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.L.ptk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- scene / camera / frame ------------------------------------------------------------
    def upload_scene(self, arrays: dict):
        a = normalise_arrays(arrays)
        d = scene_desc(a)
        self._chk(self.L.ptk_upload_scene(self.h, C.byref(d)), "ptk_upload_scene")

    def num_triangles(self) -> int:
        """triangles of the uploaded scene (ptk_bvh_info: every triangle has one record in the leaf order)"""
        return self.bvh_info()[2]

    def update_materials(self, materials: np.ndarray):
        m = np.ascontiguousarray(materials, dtype=MATERIAL_DTYPE)
        self._chk(self.L.ptk_update_materials(self.h, len(m), m.ctypes.data), "ptk_update_materials")

    def update_geometry(self, first: int, verts, normals=None, tbn=None, num_tris: Optional[int] = None):
        """ptk_update_geometry: move triangles [first, first + n) of the uploaded scene and refit the BVH.  verts / normals / tbn
        are [n, 9] float32: numpy arrays (host call), or - for ptk_update_geometry_device - torch tensors on the context's GPU
        or integer device addresses (then num_tris says how many triangles).  normals and tbn go together or are both None."""
        def dev_ptr(a):
            if a is None:
                return None
            if isinstance(a, int):
                return C.c_void_p(a)
            assert a.is_cuda and a.is_contiguous() and str(a.dtype) == "torch.float32", "float32 contiguous device tensor"
            return C.c_void_p(a.data_ptr())
        if isinstance(verts, int) or hasattr(verts, "data_ptr"):
            n = int(num_tris) if num_tris is not None else verts.numel() // 9
            dev = self.device_ordinal()
            for t in (verts, normals, tbn):                   # tensors: on THIS context's GPU, and n x 9 floats each
                if t is not None and not isinstance(t, int):
                    assert t.device.index == dev, f"tensor on cuda:{t.device.index}, context on device {dev}"
                    assert t.numel() == n * 9, f"{t.numel()} elements where {n} triangles need {n * 9}"
            self._chk(self.L.ptk_update_geometry_device(self.h, int(first), n, dev_ptr(verts), dev_ptr(normals), dev_ptr(tbn)),
                      "ptk_update_geometry_device")
            return
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
        nn = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(len(v), 9)
        tb = None if tbn is None else np.ascontiguousarray(tbn, dtype=np.float32).reshape(len(v), 9)
        self._chk(self.L.ptk_update_geometry(self.h, int(first), len(v), v.ctypes.data if len(v) else None,
                                             None if nn is None else nn.ctypes.data, None if tb is None else tb.ctypes.data),
                  "ptk_update_geometry")

    def device_ordinal(self) -> int:
        """the HIP ordinal of this context's GPU"""
        d = C.c_int32(-1)
        self.L.ptk_comm_info(self.h, None, None, None, C.byref(d))       # (the ordinal is written even where there is no communicator)
        return d.value

    def geometry_info(self) -> dict:
        """ptk_geometry_info: updates since the upload, whether the tree is a refitted one, its SAH cost as built and now."""
        u = C.c_uint32(0); r = C.c_int(0); b = C.c_double(0); n = C.c_double(0)
        self._chk(self.L.ptk_geometry_info(self.h, C.byref(u), C.byref(r), C.byref(b), C.byref(n)), "ptk_geometry_info")
        return {"updates": u.value, "refitted": bool(r.value), "sah_built": b.value, "sah_now": n.value}

    def geometry_timing(self) -> dict:
        """HIP-event times (ms) of the last update_geometry: staging copies + bounds, record repack, refit."""
        t = (C.c_float * 3)()
        self._chk(self.L.ptk_geometry_timing(self.h, t), "ptk_geometry_timing")
        return {"copy_ms": t[0], "repack_ms": t[1], "refit_ms": t[2]}

    def set_camera(self, pos, dir, up, focal, fovy, focal_dist, aperture):
        f3 = C.c_float * 3
        self._chk(self.L.ptk_set_camera(self.h, f3(*map(float, pos)), f3(*map(float, dir)), f3(*map(float, up)),
                                        float(focal), float(fovy), float(focal_dist), float(aperture)), "ptk_set_camera")

    def set_frame(self, width: int, height: int, max_depth: int):
        self._chk(self.L.ptk_set_frame(self.h, width, height, max_depth), "ptk_set_frame")
        self.width, self.height = width, height

    def set_tile(self, rank: int, world: int):
        self._chk(self.L.ptk_set_tile(self.h, rank, world), "ptk_set_tile")

    def reset(self):
        self._chk(self.L.ptk_reset(self.h), "ptk_reset")

    # ---- render ----------------------------------------------------------------------------
    def render(self, first_sample: int, spp: int, seed: int):
        self._chk(self.L.ptk_render(self.h, first_sample, spp, seed), "ptk_render")

    def render_adaptive(self, threshold: float, min_spp: int, step: int, max_spp: int, seed: int) -> dict:
        """Adaptive render (include/ptk.h ptk_render_adaptive): resets the accumulator, renders rounds of `step` samples until
        every pixel meets `threshold` or has max_spp; synchronous.  Returns rounds, max_count, pixel_samples, active_pixels."""
        r = AdaptiveResult()
        self._chk(self.L.ptk_render_adaptive(self.h, float(threshold), int(min_spp), int(step), int(max_spp), int(seed),
                                             C.byref(r)), "ptk_render_adaptive")
        return r.as_dict()

    def render_features(self, mask: int, sample: int = 0, seed: int = 0):
        """ptk_render_features: the first-hit planes of `mask` (bit k = FEAT_*) for sample `sample` of `seed`; asynchronous."""
        self._chk(self.L.ptk_render_features(self.h, int(sample), int(seed), int(mask)), "ptk_render_features")

    def read_feature(self, feature: int) -> np.ndarray:
        """One plane of the last render_features: [H, W] or [H, W, c], float32 or int32, rows bottom-up like read_accum."""
        out = feature_array(feature, self.width, self.height)
        self._chk(self.L.ptk_read_feature(self.h, int(feature), out.ctypes.data), "ptk_read_feature")
        return out

    def feature_device_ptr(self, feature: int):
        p = C.c_void_p(); b = C.c_size_t()
        self._chk(self.L.ptk_feature_device_ptr(self.h, int(feature), C.byref(p), C.byref(b)), "ptk_feature_device_ptr")
        return p.value, b.value

    def pick(self, x: int, y: int, seed: int = 0):
        """ptk_pick: (triangle, material, t) of what pixel (x, y) sees, y from the top row; (-1, -1, inf) for nothing."""
        tri = C.c_int32(-1); mat = C.c_int32(-1); t = C.c_float(0)
        self._chk(self.L.ptk_pick(self.h, int(x), int(y), int(seed), C.byref(tri), C.byref(mat), C.byref(t)), "ptk_pick")
        return tri.value, mat.value, t.value

    def trace_rays(self, origins, dirs, max_depth: int, first_sample: int, spp: int, seed: int, key_base: int = 0, out=None,
                   lens_draws: bool = False):
        """ptk_trace_rays: radiance along the rays (origins[i], dirs[i]) - [n, 3] float32, unit directions - summed in float32 over
        samples [first_sample, first_sample + spp) in sample order, on the streams of (seed, RNG pixel key_base + i, sample).
        numpy arrays go through the host entry (synchronous) and give a numpy [n, 3] float32 array.  torch tensors on the context's
        GPU go through ptk_trace_rays_device with no host copy and give a torch tensor, written on the context's stream: after
        set_stream(the tensors' stream) everything is ordered on that stream, otherwise synchronise around the call.
        out: an array / tensor of the same kind that already holds sums of earlier samples; the new ones are added to it in place
        (PTK_RAYS_ACCUMULATE) and it is returned.  lens_draws: PTK_RAYS_LENS_DRAWS (include/ptk.h)."""
        flags = (RAYS_ACCUMULATE if out is not None else 0) | (RAYS_LENS_DRAWS if lens_draws else 0)
        args = (int(max_depth), int(first_sample), int(spp), int(seed), int(key_base) & 0xffffffff, flags)
        if hasattr(origins, "data_ptr"):
            import torch
            dev = self.device_ordinal()
            n = origins.numel() // 3
            if out is None:
                out = torch.empty((n, 3), dtype=torch.float32, device=origins.device)
            for t in (origins, dirs, out):
                assert t.is_cuda and t.device.index == dev, f"tensor on {t.device}, context on device {dev}"
                assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n * 3, "[n, 3] float32 contiguous tensors"
            ptr = (lambda t: C.c_void_p(t.data_ptr()) if n else None)
            self._chk(self.L.ptk_trace_rays_device(self.h, n, ptr(origins), ptr(dirs), *args, ptr(out)), "ptk_trace_rays_device")
            return out
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n, "as many directions as origins"
        if out is None:
            out = np.empty((n, 3), np.float32)
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.size == n * 3, \
            "out: a C-contiguous float32 array of n x 3"
        ptr = (lambda a: a.ctypes.data if n else None)
        self._chk(self.L.ptk_trace_rays(self.h, n, ptr(o), ptr(d), *args, ptr(out)), "ptk_trace_rays")
        return out

    def last_rays_ms(self):
        """(trace_ms, fold_ms): HIP-event times of the last trace_rays call's kernels, summed over its passes; waits for it."""
        t = C.c_float(0); f = C.c_float(0)
        self._chk(self.L.ptk_last_rays_ms(self.h, C.byref(t), C.byref(f)), "ptk_last_rays_ms")
        return t.value, f.value

    # ---- closest-hit and occlusion queries --------------------------------------------------
    def _ray_tensors(self, tensors, n, widths):
        import torch
        dev = self.device_ordinal()
        for t, (dtype, k) in zip(tensors, widths):
            assert t.is_cuda and t.device.index == dev, f"tensor on {t.device}, context on device {dev}"
            assert t.dtype == dtype and t.is_contiguous() and t.numel() == n * k, f"contiguous {dtype} tensors of n x {k}"

    def intersect_rays(self, origins, dirs, sample: int = 0, seed: int = 0, key_base: int = 0):
        """ptk_intersect_rays: the closest accepted hit of the rays (origins[i], dirs[i]) - [n, 3] float32, directions used as
        given - with the stochastic-opacity draws of sample `sample` of (seed, RNG pixel key_base + i).  Returns (tri [n] int32, -1
        on a miss; t [n] float32 in units of |dir|, inf on a miss; bary [n, 2] float32 = u, v; material [n] int32, -1 on a miss).
        numpy arrays go through the host entry (synchronous) and give numpy arrays; torch tensors on the context's GPU go through
        ptk_intersect_rays_device with no host copy and give torch tensors written on the context's stream (see trace_rays)."""
        args = (int(sample), int(seed), int(key_base) & 0xffffffff)
        if hasattr(origins, "data_ptr"):
            import torch
            n = origins.numel() // 3
            mk = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=origins.device)
            out = (mk((n,), torch.int32), mk((n,), torch.float32), mk((n, 2), torch.float32), mk((n,), torch.int32))
            self._ray_tensors((origins, dirs), n, ((torch.float32, 3),) * 2)
            if n:
                self._chk(self.L.ptk_intersect_rays_device(self.h, n, C.c_void_p(origins.data_ptr()), C.c_void_p(dirs.data_ptr()), *args,
                                                           *(C.c_void_p(t.data_ptr()) for t in out)), "ptk_intersect_rays_device")
            return out
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n, "as many directions as origins"
        out = (np.empty(n, np.int32), np.empty(n, np.float32), np.empty((n, 2), np.float32), np.empty(n, np.int32))
        if n:
            self._chk(self.L.ptk_intersect_rays(self.h, n, o.ctypes.data, d.ctypes.data, *args, *(a.ctypes.data for a in out)),
                      "ptk_intersect_rays")
        return out

    def occluded_rays(self, origins, dirs, tmax=None, sample: int = 0, seed: int = 0, key_base: int = 0):
        """ptk_occluded_rays: [n] uint8, 1 where some accepted triangle lies at t < tmax[i] (strictly; t in units of |dir|) along
        ray i, under the candidate rule of intersect_rays.  tmax: [n] float32 of the rays' kind, or None for no bound.  numpy in,
        numpy out through the host entry; torch in, torch out through ptk_occluded_rays_device with no host copy."""
        args = (int(sample), int(seed), int(key_base) & 0xffffffff)
        if hasattr(origins, "data_ptr"):
            import torch
            n = origins.numel() // 3
            out = torch.empty((n,), dtype=torch.uint8, device=origins.device)
            self._ray_tensors((origins, dirs), n, ((torch.float32, 3),) * 2)
            if tmax is not None:
                self._ray_tensors((tmax,), n, ((torch.float32, 1),))
            if n:
                self._chk(self.L.ptk_occluded_rays_device(self.h, n, C.c_void_p(origins.data_ptr()), C.c_void_p(dirs.data_ptr()),
                                                          C.c_void_p(tmax.data_ptr()) if tmax is not None else None, *args,
                                                          C.c_void_p(out.data_ptr())), "ptk_occluded_rays_device")
            return out
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n, "as many directions as origins"
        tm = None
        if tmax is not None:
            tm = np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
            assert len(tm) == n, "one tmax per ray"
        out = np.empty(n, np.uint8)
        if n:
            self._chk(self.L.ptk_occluded_rays(self.h, n, o.ctypes.data, d.ctypes.data, tm.ctypes.data if tm is not None else None, *args,
                                               out.ctypes.data), "ptk_occluded_rays")
        return out

    def last_hits_ms(self) -> float:
        """HIP-event time of the last intersect_rays / occluded_rays call's kernel; waits for it."""
        t = C.c_float(0)
        self._chk(self.L.ptk_last_hits_ms(self.h, C.byref(t)), "ptk_last_hits_ms")
        return t.value

    # ---- closest-point queries --------------------------------------------------------------
    def closest_points(self, points, max_dist=None):
        """ptk_closest_points: for each of the points [n, 3] float32 the nearest point of the scene's surface, under the rule of
        include/ptk.h.  max_dist: [n] float32 of the points' kind - only surface strictly nearer counts; NaN, zero or negative finds
        nothing - or None for no bound.  Returns (tri [n] int32, -1 on a miss; dist [n] float32, inf on a miss; point [n, 3]
        float32, 0 on a miss; bary [n, 2] float32 = the weights of vertex 2 and vertex 3, 0 on a miss).  numpy arrays go through
        the host entry (synchronous) and give numpy arrays; torch tensors on the context's GPU go through
        ptk_closest_points_device with no host copy and give torch tensors written on the context's stream (see trace_rays)."""
        if hasattr(points, "data_ptr"):
            import torch
            n = points.numel() // 3
            mk = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=points.device)
            out = (mk((n,), torch.int32), mk((n,), torch.float32), mk((n, 3), torch.float32), mk((n, 2), torch.float32))
            self._ray_tensors((points,), n, ((torch.float32, 3),))
            if max_dist is not None:
                self._ray_tensors((max_dist,), n, ((torch.float32, 1),))
            if n:
                self._chk(self.L.ptk_closest_points_device(self.h, n, C.c_void_p(points.data_ptr()),
                                                           C.c_void_p(max_dist.data_ptr()) if max_dist is not None else None,
                                                           *(C.c_void_p(t.data_ptr()) for t in out)), "ptk_closest_points_device")
            return out
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        md = None
        if max_dist is not None:
            md = np.ascontiguousarray(max_dist, dtype=np.float32).reshape(-1)
            assert len(md) == n, "one max_dist per point"
        out = (np.empty(n, np.int32), np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 2), np.float32))
        if n:
            self._chk(self.L.ptk_closest_points(self.h, n, p.ctypes.data, md.ctypes.data if md is not None else None,
                                                *(a.ctypes.data for a in out)), "ptk_closest_points")
        return out

    def last_closest_ms(self) -> float:
        """HIP-event time of the last closest_points call's kernel; waits for it."""
        t = C.c_float(0)
        self._chk(self.L.ptk_last_closest_ms(self.h, C.byref(t)), "ptk_last_closest_ms")
        return t.value

    def closest_stats(self, points, max_dist=None):
        """ptk_closest_stats (measurement hook): (interior nodes fetched, triangle records tested) by a closest_points query of
        these torch tensors on the context's GPU, summed over the points; synchronous, writes no outputs."""
        import torch
        n = points.numel() // 3
        self._ray_tensors((points,), n, ((torch.float32, 3),))
        if max_dist is not None:
            self._ray_tensors((max_dist,), n, ((torch.float32, 1),))
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.L.ptk_closest_stats(self.h, n, C.c_void_p(points.data_ptr()) if n else None,
                                           C.c_void_p(max_dist.data_ptr()) if max_dist is not None else None, C.byref(a), C.byref(b)),
                  "ptk_closest_stats")
        return a.value, b.value

    # ---- crossing counts, containment, signed distance ---------------------------------------
    def crossings_rays(self, origins, dirs, tmax=None):
        """ptk_crossings_rays: (front [n] int32, back [n] int32), the number of triangles ray i = (origins[i], dirs[i]) crosses at
        1e-5 < t < tmax[i] (t in units of |dir|) from the side they wind counter-clockwise on / from the other side, under the rule
        of include/ptk.h - geometry only, every crossing counts.  tmax: [n] float32 of the rays' kind, or None for no bound.  numpy
        in, numpy out through the host entry; torch in, torch out through ptk_crossings_rays_device with no host copy."""
        if hasattr(origins, "data_ptr"):
            import torch
            n = origins.numel() // 3
            out = (torch.empty((n,), dtype=torch.int32, device=origins.device), torch.empty((n,), dtype=torch.int32, device=origins.device))
            self._ray_tensors((origins, dirs), n, ((torch.float32, 3),) * 2)
            if tmax is not None:
                self._ray_tensors((tmax,), n, ((torch.float32, 1),))
            if n:
                self._chk(self.L.ptk_crossings_rays_device(self.h, n, C.c_void_p(origins.data_ptr()), C.c_void_p(dirs.data_ptr()),
                                                           C.c_void_p(tmax.data_ptr()) if tmax is not None else None,
                                                           *(C.c_void_p(t.data_ptr()) for t in out)), "ptk_crossings_rays_device")
            return out
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n, "as many directions as origins"
        tm = None
        if tmax is not None:
            tm = np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
            assert len(tm) == n, "one tmax per ray"
        out = (np.empty(n, np.int32), np.empty(n, np.int32))
        if n:
            self._chk(self.L.ptk_crossings_rays(self.h, n, o.ctypes.data, d.ctypes.data, tm.ctypes.data if tm is not None else None,
                                                *(a.ctypes.data for a in out)), "ptk_crossings_rays")
        return out

    def _inside_dirs(self, dirs, torch_device=None):
        """(D, the direction array to keep alive or None for the built-in set, its pointer or None)"""
        if dirs is None:
            return 3, None, None
        if torch_device is not None and hasattr(dirs, "data_ptr"):
            import torch
            D = dirs.numel() // 3
            self._ray_tensors((dirs,), D, ((torch.float32, 3),))
            return D, dirs, C.c_void_p(dirs.data_ptr())
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        if torch_device is not None:
            import torch
            t = torch.from_numpy(d).to(torch_device)
            return len(d), t, C.c_void_p(t.data_ptr())
        return len(d), d, d.ctypes.data

    def contains_points(self, points, dirs=None, mode=INSIDE_WINDING, want_winding: bool = False):
        """ptk_contains_points: inside [n] uint8, 1 where the majority of the rays from points[i] along the D directions votes
        inside - under "winding" (the default) a ray votes when it crosses unequal numbers of back and front faces, under "parity"
        when it crosses an odd number of faces.  dirs: [D, 3] float32, D odd and in 1 .. 31, or None for the built-in three
        (inside_default_dirs()).  With want_winding also winding [n, D] int32 = back - front per direction: (inside, winding).
        numpy in, numpy out through the host entry; torch in, torch out through ptk_contains_points_device (a numpy dirs is copied
        to the points' device first)."""
        m = inside_mode(mode)
        if hasattr(points, "data_ptr"):
            import torch
            n = points.numel() // 3
            self._ray_tensors((points,), n, ((torch.float32, 3),))
            D, keep, dptr = self._inside_dirs(dirs, points.device)
            inside = torch.empty((n,), dtype=torch.uint8, device=points.device)
            winding = torch.empty((n, D), dtype=torch.int32, device=points.device) if want_winding else None
            if n:
                self._chk(self.L.ptk_contains_points_device(self.h, n, C.c_void_p(points.data_ptr()), D, dptr, m, C.c_void_p(inside.data_ptr()),
                                                            C.c_void_p(winding.data_ptr()) if want_winding else None), "ptk_contains_points_device")
                if keep is not None and keep is not dirs:
                    self.synchronize()                      # (the copy of dirs made here must outlive the kernel)
            return (inside, winding) if want_winding else inside
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        D, keep, dptr = self._inside_dirs(dirs)
        inside = np.empty(n, np.uint8)
        winding = np.empty((n, D), np.int32) if want_winding else None
        if n:
            self._chk(self.L.ptk_contains_points(self.h, n, p.ctypes.data, D, dptr, m, inside.ctypes.data,
                                                 winding.ctypes.data if want_winding else None), "ptk_contains_points")
        elif D < 1 or D > 31 or D % 2 == 0:
            raise PtkError("ptk_contains_points: num_dirs must be odd and in 1 .. 31")
        return (inside, winding) if want_winding else inside

    def signed_distance(self, points, max_dist=None, dirs=None, mode=INSIDE_WINDING):
        """ptk_signed_distance: closest_points(points, max_dist) - (tri, dist, point, bary), bit for bit - with the sign bit of dist
        set where contains_points(points, dirs, mode) says inside: negative inside, -inf inside and beyond max_dist.  numpy in,
        numpy out through the host entry; torch in, torch out through ptk_signed_distance_device."""
        m = inside_mode(mode)
        if hasattr(points, "data_ptr"):
            import torch
            n = points.numel() // 3
            mk = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=points.device)
            out = (mk((n,), torch.int32), mk((n,), torch.float32), mk((n, 3), torch.float32), mk((n, 2), torch.float32))
            self._ray_tensors((points,), n, ((torch.float32, 3),))
            if max_dist is not None:
                self._ray_tensors((max_dist,), n, ((torch.float32, 1),))
            D, keep, dptr = self._inside_dirs(dirs, points.device)
            if n:
                self._chk(self.L.ptk_signed_distance_device(self.h, n, C.c_void_p(points.data_ptr()),
                                                            C.c_void_p(max_dist.data_ptr()) if max_dist is not None else None, D, dptr, m,
                                                            *(C.c_void_p(t.data_ptr()) for t in out)), "ptk_signed_distance_device")
                if keep is not None and keep is not dirs:
                    self.synchronize()
            return out
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        md = None
        if max_dist is not None:
            md = np.ascontiguousarray(max_dist, dtype=np.float32).reshape(-1)
            assert len(md) == n, "one max_dist per point"
        D, keep, dptr = self._inside_dirs(dirs)
        out = (np.empty(n, np.int32), np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 2), np.float32))
        if n:
            self._chk(self.L.ptk_signed_distance(self.h, n, p.ctypes.data, md.ctypes.data if md is not None else None, D, dptr, m,
                                                 *(a.ctypes.data for a in out)), "ptk_signed_distance")
        elif D < 1 or D > 31 or D % 2 == 0:
            raise PtkError("ptk_signed_distance: num_dirs must be odd and in 1 .. 31")
        return out

    def last_crossings_ms(self) -> float:
        """HIP-event time of the last crossings_rays / contains_points / signed_distance call's kernels; waits for it."""
        t = C.c_float(0)
        self._chk(self.L.ptk_last_crossings_ms(self.h, C.byref(t)), "ptk_last_crossings_ms")
        return t.value

    # ---- ordered multi-hit queries ------------------------------------------------------------
    def multihit_rays(self, origins, dirs, max_hits, tmax=None):
        """ptk_multihit_rays: (count [n] int32, tri [n, K] int32, t [n, K] float32, bary [n, K, 2] float32, side [n, K] int8) for
        K = max_hits in 1 .. MULTIHIT_MAX - the first K triangles ray i = (origins[i], dirs[i]) crosses at 1e-5 < t < tmax[i],
        ascending by (t, triangle index) under the rule of include/ptk.h; geometry only, coincident triangles each appear.  Behind
        count[i]: tri -1, t +inf, bary 0, side 0.  side is +1 where the ray meets the triangle's counter-clockwise side, -1 on the
        other.  tmax: [n] float32 of the rays' kind, or None for no bound.  numpy in, numpy out through the host entry; torch in,
        torch out through ptk_multihit_rays_device with no host copy."""
        K = int(max_hits)
        if K < 1 or K > MULTIHIT_MAX:
            raise PtkError(f"ptk_multihit_rays: max_hits must be in 1 .. {MULTIHIT_MAX}")
        if hasattr(origins, "data_ptr"):
            import torch
            n = origins.numel() // 3
            mk = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=origins.device)
            out = (mk((n,), torch.int32), mk((n, K), torch.int32), mk((n, K), torch.float32), mk((n, K, 2), torch.float32), mk((n, K), torch.int8))
            self._ray_tensors((origins, dirs), n, ((torch.float32, 3),) * 2)
            if tmax is not None:
                self._ray_tensors((tmax,), n, ((torch.float32, 1),))
            if n:
                self._chk(self.L.ptk_multihit_rays_device(self.h, n, C.c_void_p(origins.data_ptr()), C.c_void_p(dirs.data_ptr()),
                                                          C.c_void_p(tmax.data_ptr()) if tmax is not None else None, K,
                                                          *(C.c_void_p(t.data_ptr()) for t in out)), "ptk_multihit_rays_device")
            return out
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n, "as many directions as origins"
        tm = None
        if tmax is not None:
            tm = np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
            assert len(tm) == n, "one tmax per ray"
        out = (np.empty(n, np.int32), np.empty((n, K), np.int32), np.empty((n, K), np.float32), np.empty((n, K, 2), np.float32),
               np.empty((n, K), np.int8))
        if n:
            self._chk(self.L.ptk_multihit_rays(self.h, n, o.ctypes.data, d.ctypes.data, tm.ctypes.data if tm is not None else None, K,
                                               *(a.ctypes.data for a in out)), "ptk_multihit_rays")
        return out

    def last_multihit_ms(self) -> float:
        """HIP-event time of the last multihit_rays call's kernel (0 where it launched none); waits for it."""
        t = C.c_float(0)
        self._chk(self.L.ptk_last_multihit_ms(self.h, C.byref(t)), "ptk_last_multihit_ms")
        return t.value

    # ---- K-nearest triangle queries -------------------------------------------------------------
    def nearest_triangles(self, points, k, max_dist=None):
        """ptk_nearest_triangles: (count [n] int32, tri [n, K] int32, dist [n, K] float32, point [n, K, 3] float32, bary [n, K, 2]
        float32) for K = k in 1 .. NEAREST_MAX_K - the K triangles nearest to each of the points [n, 3] float32, ascending by
        (distance, triangle index) under closest_points' rule (include/ptk.h); coincident triangles each appear, column 0 is
        closest_points' answer.  max_dist: [n] float32 of the points' kind - only surface strictly nearer counts; NaN, zero or
        negative finds nothing - or None for no bound.  Behind count[i]: tri -1, dist +inf, point 0, bary 0.  numpy in, numpy out
        through the host entry; torch in, torch out through ptk_nearest_triangles_device with no host copy."""
        K = int(k)
        if K < 1 or K > NEAREST_MAX_K:
            raise PtkError(f"ptk_nearest_triangles: k must be in 1 .. {NEAREST_MAX_K}")
        if hasattr(points, "data_ptr"):
            import torch
            n = points.numel() // 3
            mk = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=points.device)
            out = (mk((n,), torch.int32), mk((n, K), torch.int32), mk((n, K), torch.float32), mk((n, K, 3), torch.float32),
                   mk((n, K, 2), torch.float32))
            self._ray_tensors((points,), n, ((torch.float32, 3),))
            if max_dist is not None:
                self._ray_tensors((max_dist,), n, ((torch.float32, 1),))
            if n:
                self._chk(self.L.ptk_nearest_triangles_device(self.h, n, C.c_void_p(points.data_ptr()),
                                                              C.c_void_p(max_dist.data_ptr()) if max_dist is not None else None, K,
                                                              *(C.c_void_p(t.data_ptr()) for t in out)), "ptk_nearest_triangles_device")
            return out
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        md = None
        if max_dist is not None:
            md = np.ascontiguousarray(max_dist, dtype=np.float32).reshape(-1)
            assert len(md) == n, "one max_dist per point"
        out = (np.empty(n, np.int32), np.empty((n, K), np.int32), np.empty((n, K), np.float32), np.empty((n, K, 3), np.float32),
               np.empty((n, K, 2), np.float32))
        if n:
            self._chk(self.L.ptk_nearest_triangles(self.h, n, p.ctypes.data, md.ctypes.data if md is not None else None, K,
                                                   *(a.ctypes.data for a in out)), "ptk_nearest_triangles")
        return out

    def last_nearest_ms(self) -> float:
        """HIP-event time of the last nearest_triangles call's kernel (0 where it launched none); waits for it."""
        t = C.c_float(0)
        self._chk(self.L.ptk_last_nearest_ms(self.h, C.byref(t)), "ptk_last_nearest_ms")
        return t.value

    def nearest_stats(self, points, k, max_dist=None):
        """ptk_nearest_stats (measurement hook): (interior nodes fetched, triangle records tested) by a nearest_triangles query for
        this k of these torch tensors on the context's GPU, summed over the points; synchronous, writes no outputs."""
        import torch
        n = points.numel() // 3
        self._ray_tensors((points,), n, ((torch.float32, 3),))
        if max_dist is not None:
            self._ray_tensors((max_dist,), n, ((torch.float32, 1),))
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.L.ptk_nearest_stats(self.h, n, C.c_void_p(points.data_ptr()) if n else None,
                                           C.c_void_p(max_dist.data_ptr()) if max_dist is not None else None, int(k), C.byref(a), C.byref(b)),
                  "ptk_nearest_stats")
        return a.value, b.value

    # ---- overlap queries ----------------------------------------------------------------------
    def _overlap(self, name, a, b, width_b, k, tri_from):
        """the entry `name` (host: numpy) or `name`_device (torch) over queries a [n, 3], b [n, width_b]: (count [n], tris [n, k])"""
        K = int(k)
        if K < 0 or K > OVERLAP_MAX_K:
            raise PtkError(f"{name}: k must be in 0 .. {OVERLAP_MAX_K}")
        if hasattr(a, "data_ptr"):
            import torch
            n = a.numel() // 3
            out = (torch.empty((n,), dtype=torch.int32, device=a.device), torch.empty((n, K), dtype=torch.int32, device=a.device))
            self._ray_tensors((a, b), n, ((torch.float32, 3), (torch.float32, width_b)))
            if tri_from is not None:
                self._ray_tensors((tri_from,), n, ((torch.int32, 1),))
            if n:
                self._chk(getattr(self.L, name + "_device")(self.h, n, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                                                            C.c_void_p(tri_from.data_ptr()) if tri_from is not None else None, K,
                                                            C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()) if K else None),
                          name + "_device")
            return out
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        n = len(a)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        assert len(b) == n * width_b, "one box corner or radius per query"
        tf = None
        if tri_from is not None:
            tf = np.ascontiguousarray(tri_from, dtype=np.int32).reshape(-1)
            assert len(tf) == n, "one tri_from per query"
        out = (np.empty(n, np.int32), np.empty((n, K), np.int32))
        if n:
            self._chk(getattr(self.L, name)(self.h, n, a.ctypes.data, b.ctypes.data, tf.ctypes.data if tf is not None else None, K,
                                            out[0].ctypes.data, out[1].ctypes.data if K else None), name)
        return out

    def overlap_boxes(self, lo, hi, k: int = 0, tri_from=None):
        """ptk_overlap_boxes: (count [n] int32, tris [n, k] int32) for the closed boxes [lo[i], hi[i]] ([n, 3] float32 each) under
        the 13-axis rule of include/ptk.h: count = how many triangles of index >= tri_from[i] (None: 0) meet the box - k does not
        cap it -, tris = the k smallest of their indices ascending, -1 behind the last; 0 <= k <= OVERLAP_MAX_K.  A box with
        !(lo <= hi) on some axis meets nothing.  Page through a long list with tri_from = last listed + 1 (overlap.all_in_boxes).
        numpy in, numpy out through the host entry; torch in, torch out through ptk_overlap_boxes_device with no host copy."""
        return self._overlap("ptk_overlap_boxes", lo, hi, 3, k, tri_from)

    def overlap_spheres(self, centers, radius, k: int = 0, tri_from=None):
        """ptk_overlap_spheres: overlap_boxes' answer for the spheres (centers[i], radius[i]) - [n, 3] and [n] float32: a triangle
        is met when closest_points' squared distance from the centre is finite and strictly below radius^2; a NaN, zero or
        negative radius meets nothing."""
        return self._overlap("ptk_overlap_spheres", centers, radius, 1, k, tri_from)

    def last_overlap_ms(self) -> float:
        """HIP-event time of the last overlap_boxes / overlap_spheres call's kernel (0 where it launched none); waits for it."""
        t = C.c_float(0)
        self._chk(self.L.ptk_last_overlap_ms(self.h, C.byref(t)), "ptk_last_overlap_ms")
        return t.value

    def overlap_stats(self, shape, a, b, tri_from=None):
        """ptk_overlap_stats (measurement hook): (interior nodes fetched, triangle records tested, triangles accepted, records the
        three box axes did not separate - boxes only) by an overlap query of these torch tensors on the context's GPU (shape
        OVERLAP_BOX: lo, hi; OVERLAP_SPHERE: centers, radius), summed over the queries; synchronous, writes no outputs."""
        import torch
        n = a.numel() // 3
        self._ray_tensors((a, b), n, ((torch.float32, 3), (torch.float32, 3 if shape == OVERLAP_BOX else 1)))
        if tri_from is not None:
            self._ray_tensors((tri_from,), n, ((torch.int32, 1),))
        got = (C.c_uint64 * 4)()
        self._chk(self.L.ptk_overlap_stats(self.h, int(shape), n, C.c_void_p(a.data_ptr()) if n else None, C.c_void_p(b.data_ptr()) if n else None,
                                           C.c_void_p(tri_from.data_ptr()) if tri_from is not None else None, got), "ptk_overlap_stats")
        return tuple(int(v) for v in got)

    # ---- surface sampling ---------------------------------------------------------------------
    def set_surface_weights(self, weights=None):
        """ptk_surface_weights: per-triangle weights [triangles] float32, finite and >= 0, multiplied onto the areas - or None for
        the areas alone.  A numpy array goes through the host entry, a torch tensor on the context's GPU through
        ptk_surface_weights_device.  The table is rebuilt by the next call that needs it."""
        if weights is None:
            self._chk(self.L.ptk_surface_weights(self.h, None), "ptk_surface_weights")
        elif hasattr(weights, "data_ptr"):
            import torch
            self._ray_tensors((weights,), self.num_triangles(), ((torch.float32, 1),))
            self._chk(self.L.ptk_surface_weights_device(self.h, C.c_void_p(weights.data_ptr())), "ptk_surface_weights_device")
        else:
            w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
            assert len(w) == self.num_triangles(), "one weight per triangle"
            self._chk(self.L.ptk_surface_weights(self.h, w.ctypes.data), "ptk_surface_weights")

    def sample_surface(self, n, seed=0, key_base=0, sample=0, device=False, want=(True, True, True, True, True)):
        """ptk_sample_surface: (tri [n] int32, bary [n, 2], position [n, 3], normal [n, 3] float32, material [n] int32) - n points of
        the scene's surface, a triangle drawn in proportion to its area (times its weight, set_surface_weights), the point uniform
        on it, under the rule of include/ptk.h; sample j is a function of (seed, key_base + j, sample) and the scene alone.
        device=False: numpy arrays through the host entry; device=True: torch tensors on the context's GPU through
        ptk_sample_surface_device, no host copy.  want: which of the five outputs to compute (None stands for the others)."""
        n = int(n)
        shapes = (((n,), "int32"), ((n, 2), "float32"), ((n, 3), "float32"), ((n, 3), "float32"), ((n,), "int32"))
        args = (n, int(key_base) & 0xffffffff, int(sample) & 0xffffffff, int(seed) & 0xffffffffffffffff)
        if device:
            import torch
            dev = torch.device("cuda", self.device_ordinal())
            out = tuple(torch.empty(shape, dtype=getattr(torch, dt), device=dev) if w else None for (shape, dt), w in zip(shapes, want))
            self._chk(self.L.ptk_sample_surface_device(self.h, *args, *(C.c_void_p(t.data_ptr()) if t is not None else None for t in out)),
                      "ptk_sample_surface_device")
            return out
        out = tuple(np.empty(shape, dt) if w else None for (shape, dt), w in zip(shapes, want))
        self._chk(self.L.ptk_sample_surface(self.h, *args, *(a.ctypes.data if a is not None else None for a in out)), "ptk_sample_surface")
        return out

    def surface_info(self):
        """ptk_surface_info: (total, exponent E, drawable triangles, largest weight) of the sampling table in force, built where
        it is missing or stale"""
        total, e, dr, m = C.c_uint64(0), C.c_int32(0), C.c_int32(0), C.c_float(0)
        self._chk(self.L.ptk_surface_info(self.h, C.byref(total), C.byref(e), C.byref(dr), C.byref(m)), "ptk_surface_info")
        return total.value, e.value, dr.value, np.float32(m.value)

    def last_surface_ms(self):
        """(table_ms, sample_ms): HIP-event times of the last sample_surface call's table build (0: it built none) and kernel"""
        a, b = C.c_float(0), C.c_float(0)
        self._chk(self.L.ptk_last_surface_ms(self.h, C.byref(a), C.byref(b)), "ptk_last_surface_ms")
        return a.value, b.value

    def probe_surface_table(self):
        """ptk_probe_surface_table: the inclusive sums [triangles] uint64 ptk_sample_surface would search now"""
        incl = np.empty(self.num_triangles(), np.uint64)
        self._chk(self.L.ptk_probe_surface_table(self.h, incl.ctypes.data), "ptk_probe_surface_table")
        return incl

    def probe_scan_u64(self, values, items_per_workgroup=0):
        """ptk_probe_scan_u64: the table's prefix sum on these uint64 values (0 items: the table's own workgroup size)"""
        v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
        out = np.empty_like(v)
        self._chk(self.L.ptk_probe_scan_u64(self.h, len(v), v.ctypes.data, out.ctypes.data, int(items_per_workgroup)), "ptk_probe_scan_u64")
        return out

    # ---- surface attributes -------------------------------------------------------------------
    def surface_attributes(self, tri, bary, dirs=None, want=ATTR_ALL):
        """ptk_surface_attributes: dict name (ATTR_NAMES) -> array of what is AT the surface points (tri[i], bary[i] = u, v) - tri
        [n] int32, bary [n, 2] float32, as intersect_rays, closest_points, sample_surface, bake_coverage ... return them - under the
        rule of include/ptk.h: material [n] int32; uv, gloss [n, 2]; position, normal_geom, normal, albedo, emission [n, 3]; opacity
        [n] float32.  A triangle index outside the scene (a missed ray's -1) gives material -1 and zeros.  dirs [n, 3] float32 or
        None: the direction each point is seen along, against which the shading normal is flipped.  want: bit k = attribute k; only
        those are computed and returned.  numpy in, numpy out through the host entry; torch tensors on the context's GPU in, torch
        out through ptk_surface_attributes_device with no host copy, written on the context's stream."""
        want = int(want) & ATTR_ALL
        if not want:
            raise PtkError("ptk_surface_attributes: no output array")
        ids = [k for k in range(len(ATTR_NAMES)) if want >> k & 1]
        if hasattr(tri, "data_ptr"):
            import torch
            n = tri.numel()
            self._ray_tensors((tri, bary), n, ((torch.int32, 1), (torch.float32, 2)))
            if dirs is not None:
                self._ray_tensors((dirs,), n, ((torch.float32, 3),))
            out = {}
            for k in ids:
                ch, isint = attribute_info(k)
                out[ATTR_NAMES[k]] = torch.empty((n,) if ch == 1 else (n, ch), dtype=torch.int32 if isint else torch.float32, device=tri.device)
            if n:
                block = SurfaceAttrs(**{nm: t.data_ptr() for nm, t in out.items()})
                self._chk(self.L.ptk_surface_attributes_device(self.h, n, C.c_void_p(tri.data_ptr()), C.c_void_p(bary.data_ptr()),
                                                               C.c_void_p(dirs.data_ptr()) if dirs is not None else None, C.byref(block)),
                          "ptk_surface_attributes_device")
            return out
        t = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1)
        n = len(t)
        b = np.ascontiguousarray(bary, dtype=np.float32).reshape(-1, 2)
        assert len(b) == n, "one (u, v) per triangle index"
        d = None
        if dirs is not None:
            d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
            assert len(d) == n, "one direction per query"
        out = {ATTR_NAMES[k]: attribute_array(k, n) for k in ids}
        if n:
            block = SurfaceAttrs(**{nm: a.ctypes.data for nm, a in out.items()})
            self._chk(self.L.ptk_surface_attributes(self.h, n, t.ctypes.data, b.ctypes.data, d.ctypes.data if d is not None else None,
                                                    C.byref(block)), "ptk_surface_attributes")
        return out

    def last_attributes_ms(self) -> float:
        """HIP-event time of the last surface_attributes call's kernel; waits for it."""
        t = C.c_float(0)
        self._chk(self.L.ptk_last_attributes_ms(self.h, C.byref(t)), "ptk_last_attributes_ms")
        return t.value

    # ---- a-trous denoiser --------------------------------------------------------------------
    def denoise_planes(self, color, mask, normal, position, params, albedo=None, variance=None, want_variance: bool = False):
        """ptk_denoise_planes: the a-trous filter of include/ptk.h over the image color [H, W, 3] float32, guided by normal and
        position [H, W, 3] float32 over the pixels with mask [H, W] int32 >= 0; albedo [H, W, 3] demodulates, variance [H, W]
        switches the luminance weight to standard deviations.  params: DenoiseParams (denoise_defaults) or a dict of its fields.
        Returns the filtered image, or (image, variance) with want_variance.  numpy arrays go through the host entry (synchronous)
        and give numpy arrays; torch tensors on the context's GPU go through ptk_denoise_planes_device with no host copy and give
        torch tensors written on the context's stream (see trace_rays)."""
        prm = _denoise_params(params)
        assert variance is not None or not want_variance, "out_variance needs a variance plane"
        H, W = int(color.shape[0]), int(color.shape[1])
        px = H * W
        if hasattr(color, "data_ptr"):
            import torch
            planes = [(color, torch.float32, 3), (mask, torch.int32, 1), (normal, torch.float32, 3), (position, torch.float32, 3)]
            planes += [(t, torch.float32, k) for t, k in ((albedo, 3), (variance, 1)) if t is not None]
            self._ray_tensors([t for t, _, _ in planes], px, [(d, k) for _, d, k in planes])
            out = torch.empty((H, W, 3), dtype=torch.float32, device=color.device)
            out_var = torch.empty((H, W), dtype=torch.float32, device=color.device) if want_variance else None
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and px else None
            self._chk(self.L.ptk_denoise_planes_device(self.h, W, H, ptr(color), ptr(mask), ptr(normal), ptr(position), ptr(albedo),
                                                       ptr(variance), C.byref(prm), ptr(out), ptr(out_var)), "ptk_denoise_planes_device")
            return (out, out_var) if want_variance else out
        f = lambda a, shape: None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(shape)
        color, normal, position, albedo = (f(a, (H, W, 3)) for a in (color, normal, position, albedo))
        variance = f(variance, (H, W))
        mask = np.ascontiguousarray(mask, dtype=np.int32).reshape(H, W)
        out = np.empty((H, W, 3), np.float32)
        out_var = np.empty((H, W), np.float32) if want_variance else None
        ptr = lambda a: a.ctypes.data if a is not None and px else None
        self._chk(self.L.ptk_denoise_planes(self.h, W, H, ptr(color), ptr(mask), ptr(normal), ptr(position), ptr(albedo), ptr(variance),
                                            C.byref(prm), ptr(out), ptr(out_var)), "ptk_denoise_planes")
        return (out, out_var) if want_variance else out

    def denoise_frame(self, params, variance: bool = False, render_features: bool = True, seed: int = 0):
        """ptk_denoise_frame: filters the frame in the accumulator into the context's denoised plane (read_denoised); asynchronous.
        variance: the variance-guided mode, legal after render_adaptive.  render_features: render the five guide planes first
        (sample 0 of `seed`, which replaces the planes of an earlier render_features); False uses the caller's snapshot as it is."""
        if render_features:
            self.render_features((1 << FEAT_TRIANGLE) | (1 << FEAT_POSITION) | (1 << FEAT_NORMAL) | (1 << FEAT_ALBEDO) | (1 << FEAT_EMISSION),
                                 0, seed)
        prm = _denoise_params(params)
        self._chk(self.L.ptk_denoise_frame(self.h, C.byref(prm), DENOISE_VARIANCE if variance else 0), "ptk_denoise_frame")

    def read_denoised(self) -> np.ndarray:
        """[H][W][3] float32, the last denoise_frame's result, rows bottom-up like read_accum; waits for the stream."""
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        self._chk(self.L.ptk_read_denoised(self.h, out.ctypes.data), "ptk_read_denoised")
        return out

    def denoised_device_ptr(self):
        p = C.c_void_p(); b = C.c_size_t()
        self._chk(self.L.ptk_denoised_device_ptr(self.h, C.byref(p), C.byref(b)), "ptk_denoised_device_ptr")
        return p.value, b.value

    def resolve_denoised_rgb8(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The 8-bit resolve of the denoised frame, in resolve_rgb8's layout."""
        if out is None:
            out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        self._chk(self.L.ptk_resolve_denoised_rgb8(self.h, out.ctypes.data), "ptk_resolve_denoised_rgb8")
        return out

    def last_denoise_ms(self) -> dict:
        """HIP-event times of the last denoise call: pack kernel, filter launches, unpack kernel; waits for it."""
        t = [C.c_float(0) for _ in range(3)]
        self._chk(self.L.ptk_last_denoise_ms(self.h, *(C.byref(x) for x in t)), "ptk_last_denoise_ms")
        return dict(zip(("pack_ms", "filter_ms", "unpack_ms"), (x.value for x in t)))

    # ---- display transform -------------------------------------------------------------------
    def display_planes(self, color, params=None, want_state: bool = False):
        """ptk_display_planes: exposure, tone curve and transfer function of include/ptk.h over the image color [H, W, 3] float32
        into [H, W, 3] uint8, rows as given.  params: DisplayParams (display_defaults) or a dict of its fields.  A metered call
        reads and updates the context's exposure state on the device.  Returns the bytes, or (bytes, state) with want_state: a
        dict for numpy input, a [8] int32 tensor holding ptk_exposure_state's 32 bytes for tensors.  numpy arrays go through the
        host entry (synchronous); torch tensors on the context's GPU go through ptk_display_planes_device with no host copy and
        give torch tensors written on the context's stream (see trace_rays)."""
        prm = _display_params(params)
        H, W = int(color.shape[0]), int(color.shape[1])
        px = H * W
        if hasattr(color, "data_ptr"):
            import torch
            self._ray_tensors([color], px, [(torch.float32, 3)])
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=color.device)
            state = torch.zeros(8, dtype=torch.int32, device=color.device) if want_state else None
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and px else None
            self._chk(self.L.ptk_display_planes_device(self.h, W, H, ptr(color), C.byref(prm), ptr(out), ptr(state)),
                      "ptk_display_planes_device")
            return (out, state) if want_state else out
        color = np.ascontiguousarray(color, dtype=np.float32).reshape(H, W, 3)
        out = np.empty((H, W, 3), np.uint8)
        st = DisplayState()
        self._chk(self.L.ptk_display_planes(self.h, W, H, color.ctypes.data if px else None, C.byref(prm), out.ctypes.data if px else None,
                                            C.byref(st) if want_state and px else None), "ptk_display_planes")
        if want_state and not px:
            return out, self.display_state()
        return (out, st.as_dict()) if want_state else out

    def display_frame(self, source: int = DISPLAY_ACCUM, params=None):
        """ptk_display_frame: the display transform over the context's frame - source DISPLAY_ACCUM (S1 / n), DISPLAY_DENOISED or
        DISPLAY_TEMPORAL - into the context's display image (read_display); asynchronous."""
        prm = _display_params(params)
        self._chk(self.L.ptk_display_frame(self.h, int(source), C.byref(prm)), "ptk_display_frame")

    def read_display(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """[H][W][3] uint8, the last display_frame's result, in resolve_rgb8's layout; waits for the stream."""
        if out is None:
            out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        self._chk(self.L.ptk_read_display(self.h, out.ctypes.data), "ptk_read_display")
        return out

    def display_device_ptr(self):
        p = C.c_void_p(); b = C.c_size_t()
        self._chk(self.L.ptk_display_device_ptr(self.h, C.byref(p), C.byref(b)), "ptk_display_device_ptr")
        return p.value, b.value

    def display_state(self) -> dict:
        """ptk_display_state: the exposure state behind the last display call (exposure, target, lavg as float32; has_prev,
        counted, kept); waits for the stream."""
        st = DisplayState()
        self._chk(self.L.ptk_display_state(self.h, C.byref(st)), "ptk_display_state")
        return st.as_dict()

    def display_reset(self):
        """ptk_display_reset: forgets the exposure state; asynchronous."""
        self._chk(self.L.ptk_display_reset(self.h), "ptk_display_reset")

    def last_display_ms(self) -> dict:
        """HIP-event times of the last display call: meter kernel, exposure step, apply kernel; waits for it."""
        t = [C.c_float(0) for _ in range(3)]
        self._chk(self.L.ptk_last_display_ms(self.h, *(C.byref(x) for x in t)), "ptk_last_display_ms")
        return dict(zip(("meter_ms", "exposure_ms", "apply_ms"), (x.value for x in t)))

    # ---- guided upsampling -------------------------------------------------------------------
    def render_guides(self, width: int, height: int, mask: int = UPSAMPLE_GUIDES, sample: int = 0, seed: int = 0):
        """ptk_render_guides: the first-hit planes of `mask` (bit k = FEAT_*) for the current scene and camera at width x height -
        a resolution of their own, whatever the frame's is - for sample `sample` of `seed`; asynchronous.  The frame is not
        touched.  The default mask is what upsample_frame needs."""
        self._chk(self.L.ptk_render_guides(self.h, int(width), int(height), int(sample), int(seed), int(mask)), "ptk_render_guides")
        if int(width) > 0 and int(height) > 0:
            self.guide_width, self.guide_height = int(width), int(height)

    def read_guide(self, feature: int) -> np.ndarray:
        """One plane of the last render_guides: [H, W] or [H, W, c] at the guides' size, typed and laid out like read_feature's."""
        out = feature_array(feature, getattr(self, "guide_width", 0), getattr(self, "guide_height", 0))
        self._chk(self.L.ptk_read_guide(self.h, int(feature), out.ctypes.data if out.size else None), "ptk_read_guide")
        return out

    def guide_device_ptr(self, feature: int):
        p = C.c_void_p(); b = C.c_size_t()
        self._chk(self.L.ptk_guide_device_ptr(self.h, int(feature), C.byref(p), C.byref(b)), "ptk_guide_device_ptr")
        return p.value, b.value

    def guide_view(self) -> View:
        """ptk_guide_view: the image-plane set-up the last render_guides used (get_view's arithmetic at the guides' size)."""
        v = View()
        self._chk(self.L.ptk_guide_view(self.h, C.byref(v)), "ptk_guide_view")
        return v

    def upsample_planes(self, low, high, params):
        """ptk_upsample_planes: the low image carried to the high guides' resolution by the rule of include/ptk.h.  low: (color
        [h, w, 3] float32, id [h, w] int32, position [h, w, 3], normal [h, w, 3], albedo [h, w, 3] or None); high: (id [H, W],
        position, normal, albedo or None); rows bottom-up; the two albedo planes go together.  params: UpsampleParams
        (upsample_defaults) or a dict of its fields.  Returns (color [H, W, 3] float32, class [H, W] int32: 0 bilinear, 1 ring 1,
        2 a hole).  numpy arrays go through the host entry (synchronous) and give numpy arrays; torch tensors on the context's GPU
        go through ptk_upsample_planes_device with no host copy and give torch tensors written on the context's stream (see
        trace_rays)."""
        prm = _upsample_params(params)
        low, high = list(low), list(high)
        assert len(low) == 5 and len(high) == 4, "five low planes and four high planes (albedo may be None)"
        h, w = int(low[0].shape[0]), int(low[0].shape[1])
        H, W = int(high[0].shape[0]), int(high[0].shape[1])
        px, PX = h * w, H * W
        live = px > 0 and PX > 0
        if hasattr(low[0], "data_ptr"):
            import torch
            f3, i1 = (torch.float32, 3), (torch.int32, 1)
            have = [t for t in low + high if t is not None]
            kinds = [k for t, k in zip(low + high, [f3, i1, f3, f3, f3, i1, f3, f3, f3]) if t is not None]
            sizes = [n for t, n in zip(low + high, [px] * 5 + [PX] * 4) if t is not None]
            for t, k, n in zip(have, kinds, sizes):
                self._ray_tensors([t], n, [k])
            out = torch.empty((H, W, 3), dtype=torch.float32, device=low[0].device)
            cls = torch.empty((H, W), dtype=torch.int32, device=low[0].device)
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and live else None
            self._chk(self.L.ptk_upsample_planes_device(self.h, w, h, *(ptr(t) for t in low), W, H, *(ptr(t) for t in high), C.byref(prm),
                                                        ptr(out), ptr(cls)), "ptk_upsample_planes_device")
            return out, cls
        lo_kinds = [(np.float32, (h, w, 3)), (np.int32, (h, w)), (np.float32, (h, w, 3)), (np.float32, (h, w, 3)), (np.float32, (h, w, 3))]
        hi_kinds = [(np.int32, (H, W)), (np.float32, (H, W, 3)), (np.float32, (H, W, 3)), (np.float32, (H, W, 3))]
        low = [None if a is None else np.ascontiguousarray(a, dtype=d).reshape(sh) for a, (d, sh) in zip(low, lo_kinds)]
        high = [None if a is None else np.ascontiguousarray(a, dtype=d).reshape(sh) for a, (d, sh) in zip(high, hi_kinds)]
        out = np.empty((H, W, 3), np.float32); cls = np.empty((H, W), np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and live else None
        self._chk(self.L.ptk_upsample_planes(self.h, w, h, *(ptr(a) for a in low), W, H, *(ptr(a) for a in high), C.byref(prm), ptr(out),
                                             ptr(cls)), "ptk_upsample_planes")
        return out, cls

    def upsample_frame(self, source: int = UPSAMPLE_ACCUM, params=None):
        """ptk_upsample_frame: the context's frame - source UPSAMPLE_ACCUM (S1 / n), UPSAMPLE_DENOISED or UPSAMPLE_TEMPORAL - up to
        the resolution of the last render_guides, guided by the feature planes and the guide planes MATERIAL, POSITION, NORMAL and
        ALBEDO (read_upsampled); asynchronous.  params: UpsampleParams (upsample_defaults) or a dict of its fields."""
        prm = _upsample_params(params)
        self._chk(self.L.ptk_upsample_frame(self.h, int(source), C.byref(prm)), "ptk_upsample_frame")

    def upsampled_device_ptr(self):
        """(color pointer, class pointer, width, height): the last upsample_frame's result in device memory"""
        a = C.c_void_p(); b = C.c_void_p(); w = C.c_int(0); h = C.c_int(0)
        self._chk(self.L.ptk_upsampled_device_ptr(self.h, C.byref(a), C.byref(b), C.byref(w), C.byref(h)), "ptk_upsampled_device_ptr")
        return a.value, b.value, w.value, h.value

    def read_upsampled(self):
        """(color [H][W][3] float32, class [H][W] int32) of the last upsample_frame, rows bottom-up; waits for the stream."""
        _, _, w, h = self.upsampled_device_ptr()
        color = np.empty((h, w, 3), dtype=np.float32)
        cls = np.empty((h, w), dtype=np.int32)
        self._chk(self.L.ptk_read_upsampled(self.h, color.ctypes.data, cls.ctypes.data), "ptk_read_upsampled")
        return color, cls

    def last_upsample_ms(self) -> dict:
        """HIP-event times of the last upsample call: pack kernel, upsample kernel; waits for it."""
        t = [C.c_float(0) for _ in range(2)]
        self._chk(self.L.ptk_last_upsample_ms(self.h, *(C.byref(x) for x in t)), "ptk_last_upsample_ms")
        return dict(zip(("pack_ms", "kernel_ms"), (x.value for x in t)))

    # ---- temporal reprojection ---------------------------------------------------------------
    def get_view(self) -> View:
        """ptk_get_view: the image-plane set-up of the current camera and frame (a pending set_camera included); host arithmetic."""
        v = View()
        self._chk(self.L.ptk_get_view(self.h, C.byref(v)), "ptk_get_view")
        return v

    def reproject_planes(self, hist_view, current, history, params):
        """ptk_reproject_planes: the history - planes rendered under hist_view (a View or a dict of its fields) - carried into the
        current frame and blended with it, by the rule of include/ptk.h.  current and history: sequences (color [H, W, 3] float32,
        count [H, W] float32, id [H, W] int32, position [H, W, 3] float32, normal [H, W, 3] float32), rows bottom-up.  params:
        TemporalParams (temporal_defaults) or a dict of its fields.  Returns (color [H, W, 3], count [H, W]).  numpy arrays go
        through the host entry (synchronous) and give numpy arrays; torch tensors on the context's GPU go through
        ptk_reproject_planes_device with no host copy and give torch tensors written on the context's stream (see trace_rays)."""
        prm = _temporal_params(params)
        view = _view(hist_view)
        planes = list(current) + list(history)
        assert len(planes) == 10, "five current and five history planes"
        H, W = int(planes[0].shape[0]), int(planes[0].shape[1])
        px = H * W
        if hasattr(planes[0], "data_ptr"):
            import torch
            kinds = [(torch.float32, 3), (torch.float32, 1), (torch.int32, 1), (torch.float32, 3), (torch.float32, 3)] * 2
            self._ray_tensors(planes, px, kinds)
            out = torch.empty((H, W, 3), dtype=torch.float32, device=planes[0].device)
            out_n = torch.empty((H, W), dtype=torch.float32, device=planes[0].device)
            ptr = lambda t: C.c_void_p(t.data_ptr()) if px else None
            self._chk(self.L.ptk_reproject_planes_device(self.h, W, H, C.byref(view), *(ptr(t) for t in planes), C.byref(prm), ptr(out),
                                                         ptr(out_n)), "ptk_reproject_planes_device")
            return out, out_n
        shapes = [(np.float32, (H, W, 3)), (np.float32, (H, W)), (np.int32, (H, W)), (np.float32, (H, W, 3)), (np.float32, (H, W, 3))] * 2
        planes = [np.ascontiguousarray(a, dtype=d).reshape(sh) for a, (d, sh) in zip(planes, shapes)]
        out = np.empty((H, W, 3), np.float32); out_n = np.empty((H, W), np.float32)
        ptr = lambda a: a.ctypes.data if px else None
        self._chk(self.L.ptk_reproject_planes(self.h, W, H, C.byref(view), *(ptr(a) for a in planes), C.byref(prm), ptr(out), ptr(out_n)),
                  "ptk_reproject_planes")
        return out, out_n

    def temporal_frame(self, params, reset: bool = False, render_features: bool = True, seed: int = 0, moving: bool = False,
                       moments: bool = False):
        """ptk_temporal_frame: carries the previous call's result into the frame in the accumulator and blends the two by sample
        counts (read_temporal); asynchronous.  reset: drop the history.  render_features: render the guide planes MATERIAL,
        POSITION and NORMAL first (sample 0 of `seed`, which replaces the planes of an earlier render_features); False uses the
        caller's snapshot as it is.  moving: ptk_temporal_frame_moving - the history follows the triangles that
        update_geometry moved since snapshot_geometry (read_motion gives where they were); its guide planes are those three
        with TRIANGLE and BARY.  moments: ptk_temporal_frame_moments - the moments of demodulated luminance ride along
        (temporal_variance, read_temporal_variance, denoise_temporal); its guide planes are those of the entry with ALBEDO, and
        the render_features of this call adds TRIANGLE and EMISSION, which denoise_temporal needs."""
        mask = (1 << FEAT_MATERIAL) | (1 << FEAT_POSITION) | (1 << FEAT_NORMAL)
        if moving:
            mask |= (1 << FEAT_TRIANGLE) | (1 << FEAT_BARY)
        if moments:
            mask |= (1 << FEAT_ALBEDO) | (1 << FEAT_TRIANGLE) | (1 << FEAT_EMISSION)
        if render_features:
            self.render_features(mask, 0, seed)
        prm = _temporal_params(params)
        flags = TEMPORAL_RESET if reset else 0
        if moments:
            self._chk(self.L.ptk_temporal_frame_moments(self.h, C.byref(prm), flags | (TEMPORAL_MOVING if moving else 0)),
                      "ptk_temporal_frame_moments")
        elif moving:
            self._chk(self.L.ptk_temporal_frame_moving(self.h, C.byref(prm), flags), "ptk_temporal_frame_moving")
        else:
            self._chk(self.L.ptk_temporal_frame(self.h, C.byref(prm), flags), "ptk_temporal_frame")

    def read_temporal(self):
        """(color [H][W][3], count [H][W]) float32 of the last temporal_frame, rows bottom-up like read_accum; waits for the stream."""
        color = np.empty((self.height, self.width, 3), dtype=np.float32)
        count = np.empty((self.height, self.width), dtype=np.float32)
        self._chk(self.L.ptk_read_temporal(self.h, color.ctypes.data, count.ctypes.data), "ptk_read_temporal")
        return color, count

    def temporal_device_ptr(self):
        """(color pointer, count pointer, pixels): the unpacked planes of the last temporal_frame in device memory"""
        a = C.c_void_p(); b = C.c_void_p(); n = C.c_size_t()
        self._chk(self.L.ptk_temporal_device_ptr(self.h, C.byref(a), C.byref(b), C.byref(n)), "ptk_temporal_device_ptr")
        return a.value, b.value, n.value

    def last_temporal_ms(self) -> dict:
        """HIP-event times of the last reprojection call: pack kernel (0 for the frame entry), reprojection kernel; waits for it."""
        t = [C.c_float(0) for _ in range(2)]
        self._chk(self.L.ptk_last_temporal_ms(self.h, *(C.byref(x) for x in t)), "ptk_last_temporal_ms")
        return dict(zip(("pack_ms", "kernel_ms"), (x.value for x in t)))

    # ---- temporal reprojection over moving geometry ------------------------------------------
    def snapshot_geometry(self):
        """ptk_geometry_snapshot: keeps the resident vertices as they are now as the PREVIOUS geometry of render_motion and
        temporal_frame(moving=True); on the context's stream, behind every update_geometry so far and ahead of every later one."""
        self._chk(self.L.ptk_geometry_snapshot(self.h), "ptk_geometry_snapshot")

    def render_motion(self, view=None):
        """ptk_render_motion: for the feature planes TRIANGLE, BARY, POSITION and NORMAL of the last render_features, where each
        pixel's surface point was at the snapshot, its normal there, and - under `view` (a View or a dict of its fields; None: NaN
        everywhere) - its screen-space motion vector (read_motion); asynchronous."""
        v = None if view is None else _view(view)
        self._chk(self.L.ptk_render_motion(self.h, None if v is None else C.byref(v)), "ptk_render_motion")

    def read_motion(self):
        """(prev_position [H][W][3], prev_normal [H][W][3], motion [H][W][2]) float32 of the last render_motion or
        temporal_frame(moving=True), rows bottom-up; motion = (columns, top-down rows) from the pixel to where its point was, NaN
        on a miss and behind the view.  Waits for the stream."""
        pp = np.empty((self.height, self.width, 3), dtype=np.float32)
        pn = np.empty((self.height, self.width, 3), dtype=np.float32)
        mv = np.empty((self.height, self.width, 2), dtype=np.float32)
        self._chk(self.L.ptk_read_motion(self.h, pp.ctypes.data, pn.ctypes.data, mv.ctypes.data), "ptk_read_motion")
        return pp, pn, mv

    def motion_device_ptr(self):
        """(prev_position, prev_normal, motion pointers, pixels): the planes of read_motion in device memory"""
        a = C.c_void_p(); b = C.c_void_p(); m = C.c_void_p(); n = C.c_size_t()
        self._chk(self.L.ptk_motion_device_ptr(self.h, C.byref(a), C.byref(b), C.byref(m), C.byref(n)), "ptk_motion_device_ptr")
        return a.value, b.value, m.value, n.value

    def reproject_planes_moving(self, hist_view, current, prev_position, prev_normal, history, params):
        """ptk_reproject_planes_moving: reproject_planes in moving mode - prev_position and prev_normal [H, W, 3] say where the
        current frame's points were in the history's geometry and what their normals were there (read_motion).  numpy arrays or
        torch tensors, as reproject_planes."""
        prm = _temporal_params(params)
        view = _view(hist_view)
        planes = list(current) + [prev_position, prev_normal] + list(history)
        assert len(planes) == 12, "five current, two previous-geometry and five history planes"
        H, W = int(planes[0].shape[0]), int(planes[0].shape[1])
        px = H * W
        if hasattr(planes[0], "data_ptr"):
            import torch
            five = [(torch.float32, 3), (torch.float32, 1), (torch.int32, 1), (torch.float32, 3), (torch.float32, 3)]
            self._ray_tensors(planes, px, five + [(torch.float32, 3)] * 2 + five)
            out = torch.empty((H, W, 3), dtype=torch.float32, device=planes[0].device)
            out_n = torch.empty((H, W), dtype=torch.float32, device=planes[0].device)
            ptr = lambda t: C.c_void_p(t.data_ptr()) if px else None
            self._chk(self.L.ptk_reproject_planes_moving_device(self.h, W, H, C.byref(view), *(ptr(t) for t in planes), C.byref(prm),
                                                                ptr(out), ptr(out_n)), "ptk_reproject_planes_moving_device")
            return out, out_n
        five = [(np.float32, (H, W, 3)), (np.float32, (H, W)), (np.int32, (H, W)), (np.float32, (H, W, 3)), (np.float32, (H, W, 3))]
        shapes = five + [(np.float32, (H, W, 3))] * 2 + five
        planes = [np.ascontiguousarray(a, dtype=d).reshape(sh) for a, (d, sh) in zip(planes, shapes)]
        out = np.empty((H, W, 3), np.float32); out_n = np.empty((H, W), np.float32)
        ptr = lambda a: a.ctypes.data if px else None
        self._chk(self.L.ptk_reproject_planes_moving(self.h, W, H, C.byref(view), *(ptr(a) for a in planes), C.byref(prm), ptr(out),
                                                     ptr(out_n)), "ptk_reproject_planes_moving")
        return out, out_n

    def last_motion_ms(self) -> dict:
        """HIP-event times of the last render_motion or temporal_frame(moving=True): motion kernel, reprojection kernel (0 for
        render_motion); waits for it."""
        t = [C.c_float(0) for _ in range(2)]
        self._chk(self.L.ptk_last_motion_ms(self.h, *(C.byref(x) for x in t)), "ptk_last_motion_ms")
        return dict(zip(("motion_ms", "temporal_ms"), (x.value for x in t)))

    # ---- temporal moments, variance and the denoiser behind them ----------------------------
    def reproject_moments(self, hist_view, current, history, params, albedo=None, prev=None):
        """ptk_reproject_moments: reproject_planes - with prev = (prev_position, prev_normal) reproject_planes_moving - with the
        moments of demodulated luminance as one more pair of channels.  current: the five planes of reproject_planes; history:
        those five and the history's moments [H, W, 2]; albedo [H, W, 3] demodulates.  Returns (color [H, W, 3], count [H, W],
        moments [H, W, 2]).  numpy arrays or torch tensors on the context's GPU, as reproject_planes."""
        prm = _temporal_params(params)
        view = _view(hist_view)
        current = list(current); history = list(history)
        assert len(current) == 5 and len(history) == 6, "five current planes; five history planes and the history's moments"
        assert prev is None or len(prev) == 2, "prev = (prev_position, prev_normal)"
        extra = [None, None] if prev is None else list(prev)
        planes = current + extra + [albedo] + history
        H, W = int(planes[0].shape[0]), int(planes[0].shape[1])
        px = H * W
        torch_side = hasattr(planes[0], "data_ptr")
        if torch_side:
            import torch
            five = [(torch.float32, 3), (torch.float32, 1), (torch.int32, 1), (torch.float32, 3), (torch.float32, 3)]
            kinds = five + [(torch.float32, 3)] * 3 + five + [(torch.float32, 2)]
            have = [(t, k) for t, k in zip(planes, kinds) if t is not None]
            self._ray_tensors([t for t, _ in have], px, [k for _, k in have])
            mk = lambda shape: torch.empty(shape, dtype=torch.float32, device=planes[0].device)
            ptr = lambda t: t.data_ptr() if t is not None and px else None
        else:
            five = [(np.float32, (H, W, 3)), (np.float32, (H, W)), (np.int32, (H, W)), (np.float32, (H, W, 3)), (np.float32, (H, W, 3))]
            shapes = five + [(np.float32, (H, W, 3))] * 3 + five + [(np.float32, (H, W, 2))]
            planes = [None if a is None else np.ascontiguousarray(a, dtype=d).reshape(sh) for a, (d, sh) in zip(planes, shapes)]
            mk = lambda shape: np.empty(shape, np.float32)
            ptr = lambda a: a.ctypes.data if a is not None and px else None
        outs = [mk((H, W, 3)), mk((H, W)), mk((H, W, 2))]
        desc = ReprojectDesc(W, H, C.pointer(view), *(ptr(a) for a in planes + outs))
        if torch_side:
            self._chk(self.L.ptk_reproject_moments_device(self.h, C.byref(desc), C.byref(prm)), "ptk_reproject_moments_device")
        else:
            self._chk(self.L.ptk_reproject_moments(self.h, C.byref(desc), C.byref(prm)), "ptk_reproject_moments")
        return tuple(outs)

    def variance_planes(self, moments, count, frame_count, ident, position, normal, params):
        """ptk_variance_planes: the variance [H, W] of the accumulated demodulated luminance from its moments [H, W, 2], the
        blended count and the current frame's own count [H, W], by the rule of include/ptk.h; id [H, W] int32, position and normal
        [H, W, 3] guide the spatial estimate of pixels with a short history.  params: VarianceParams (variance_defaults) or a dict
        of its fields.  numpy arrays or torch tensors on the context's GPU, as reproject_planes."""
        prm = _variance_params(params)
        planes = [moments, count, frame_count, ident, position, normal]
        H, W = int(count.shape[0]), int(count.shape[1])
        px = H * W
        if hasattr(moments, "data_ptr"):
            import torch
            kinds = [(torch.float32, 2), (torch.float32, 1), (torch.float32, 1), (torch.int32, 1), (torch.float32, 3), (torch.float32, 3)]
            self._ray_tensors(planes, px, kinds)
            out = torch.empty((H, W), dtype=torch.float32, device=moments.device)
            ptr = lambda t: C.c_void_p(t.data_ptr()) if px else None
            self._chk(self.L.ptk_variance_planes_device(self.h, W, H, *(ptr(t) for t in planes), C.byref(prm), ptr(out)),
                      "ptk_variance_planes_device")
            return out
        shapes = [(np.float32, (H, W, 2)), (np.float32, (H, W)), (np.float32, (H, W)), (np.int32, (H, W)), (np.float32, (H, W, 3)),
                  (np.float32, (H, W, 3))]
        planes = [np.ascontiguousarray(a, dtype=d).reshape(sh) for a, (d, sh) in zip(planes, shapes)]
        out = np.empty((H, W), np.float32)
        ptr = lambda a: a.ctypes.data if px else None
        self._chk(self.L.ptk_variance_planes(self.h, W, H, *(ptr(a) for a in planes), C.byref(prm), ptr(out)), "ptk_variance_planes")
        return out

    def temporal_variance(self, params):
        """ptk_temporal_variance: the variance plane of the last temporal_frame(moments=True); asynchronous."""
        prm = _variance_params(params)
        self._chk(self.L.ptk_temporal_variance(self.h, C.byref(prm)), "ptk_temporal_variance")

    def read_temporal_variance(self, variance: bool = True):
        """(moments [H][W][2], variance [H][W]) float32 of the last temporal_frame(moments=True) and temporal_variance, rows
        bottom-up; variance=False: (moments, None), legal before temporal_variance.  Waits for the stream."""
        mom = np.empty((self.height, self.width, 2), dtype=np.float32)
        var = np.empty((self.height, self.width), dtype=np.float32) if variance else None
        self._chk(self.L.ptk_read_temporal_variance(self.h, mom.ctypes.data, var.ctypes.data if variance else None),
                  "ptk_read_temporal_variance")
        return mom, var

    def temporal_variance_device_ptr(self, variance: bool = True):
        """(moments pointer, variance pointer or None, pixels): the planes of read_temporal_variance in device memory"""
        a = C.c_void_p(); b = C.c_void_p(); n = C.c_size_t()
        self._chk(self.L.ptk_temporal_variance_device_ptr(self.h, C.byref(a), C.byref(b) if variance else None, C.byref(n)),
                  "ptk_temporal_variance_device_ptr")
        return a.value, (b.value if variance else None), n.value

    def denoise_temporal(self, params, variance: bool = True):
        """ptk_denoise_temporal: the a-trous filter over the last temporal_frame's result into the context's denoised plane
        (read_denoised), on the device; asynchronous.  variance: guided by temporal_variance's plane."""
        prm = _denoise_params(params)
        self._chk(self.L.ptk_denoise_temporal(self.h, C.byref(prm), DENOISE_VARIANCE if variance else 0), "ptk_denoise_temporal")

    def last_variance_ms(self) -> dict:
        """HIP-event times of the last variance call: variance kernel, prefilter (0 without one); waits for it."""
        t = [C.c_float(0) for _ in range(2)]
        self._chk(self.L.ptk_last_variance_ms(self.h, *(C.byref(x) for x in t)), "ptk_last_variance_ms")
        return dict(zip(("variance_ms", "prefilter_ms"), (x.value for x in t)))

    # ---- lightmap baking -------------------------------------------------------------------
    def _bake_uvs(self, uvs, torch_side: bool):
        if uvs is None:
            return None, None
        if torch_side:
            assert hasattr(uvs, "data_ptr") and uvs.is_cuda and uvs.is_contiguous() and str(uvs.dtype) == "torch.float32", \
                "uvs: a float32 contiguous tensor on the context's GPU, like out"
            return uvs, C.c_void_p(uvs.data_ptr())
        u = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6)
        return u, u.ctypes.data

    def bake_coverage(self, width: int, height: int, uvs=None):
        """ptk_bake_coverage: (owner [H, W] int32, -1 uncovered; bary [H, W, 2] = (b2, b3); pos [H, W, 3]) of a width x height
        lightmap over the chart corners uvs [triangles, 6] (None: the scene's own uvs); rows bottom-up; no tracing."""
        u, up = self._bake_uvs(uvs, False)
        owner = np.empty((height, width), np.int32)
        bary = np.empty((height, width, 2), np.float32); pos = np.empty((height, width, 3), np.float32)
        self._chk(self.L.ptk_bake_coverage(self.h, int(width), int(height), up, owner.ctypes.data, bary.ctypes.data, pos.ctypes.data),
                  "ptk_bake_coverage")
        return owner, bary, pos

    def bake_lightmap(self, width: int, height: int, offset: float, max_depth: int, first_sample: int, spp: int, seed: int, uvs=None,
                      key_base: int = 0, out=None, back: bool = False, device: bool = False):
        """ptk_bake_lightmap: (sums [H, W, 3] float32, owner [H, W] int32) of a width x height lightmap - the float32 in-order sums
        over samples [first_sample, first_sample + spp) of the radiance along each covered texel's ray (origin = P + n * offset,
        direction -n), on the streams of (seed, RNG pixel key_base + texel index, sample); rows bottom-up.
        numpy arrays (or nothing) go through the host entry (synchronous).  With a torch tensor for uvs or out - or device=True -
        the call is ptk_bake_lightmap_device with no host copy: tensors on the context's GPU in and out, written on the context's
        stream.  out: sums of earlier samples, added to in place (PTK_BAKE_ACCUMULATE).  back: PTK_BAKE_BACK."""
        flags = (BAKE_ACCUMULATE if out is not None else 0) | (BAKE_BACK if back else 0)
        args = (float(offset), int(max_depth), int(first_sample), int(spp), int(seed), int(key_base) & 0xffffffff, flags)
        if device or hasattr(uvs, "data_ptr") or hasattr(out, "data_ptr"):
            import torch
            dev = torch.device("cuda", self.device_ordinal())
            u, up = self._bake_uvs(uvs, True)
            if out is None:
                out = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
            owner = torch.empty((height, width), dtype=torch.int32, device=dev)
            assert out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous() \
                and out.numel() == width * height * 3, "out: a [H, W, 3] float32 contiguous tensor on the context's GPU"
            self._chk(self.L.ptk_bake_lightmap_device(self.h, int(width), int(height), up, *args, C.c_void_p(out.data_ptr()),
                                                      C.c_void_p(owner.data_ptr())), "ptk_bake_lightmap_device")
            return out, owner
        u, up = self._bake_uvs(uvs, False)
        if out is None:
            out = np.empty((height, width, 3), np.float32)
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.size == width * height * 3, \
            "out: a C-contiguous float32 array of H x W x 3"
        owner = np.empty((height, width), np.int32)
        self._chk(self.L.ptk_bake_lightmap(self.h, int(width), int(height), up, *args, out.ctypes.data, owner.ctypes.data), "ptk_bake_lightmap")
        return out, owner

    def dilate_lightmap(self, image, owner, passes: int):
        """ptk_lightmap_dilate: chart padding in place, `passes` times; numpy arrays (host entry) or torch tensors on the context's
        GPU (device entry, on the context's stream).  image [H, W, 3] float32, owner [H, W] int32; returns (image, owner)."""
        h, w = owner.shape
        if hasattr(image, "data_ptr"):
            import torch
            assert image.is_cuda and owner.is_cuda and image.is_contiguous() and owner.is_contiguous()
            assert image.dtype == torch.float32 and owner.dtype == torch.int32 and image.numel() == w * h * 3
            self._chk(self.L.ptk_lightmap_dilate_device(self.h, w, h, int(passes), C.c_void_p(image.data_ptr()), C.c_void_p(owner.data_ptr())),
                      "ptk_lightmap_dilate_device")
            return image, owner
        assert image.dtype == np.float32 and image.flags["C_CONTIGUOUS"] and image.size == w * h * 3
        assert owner.dtype == np.int32 and owner.flags["C_CONTIGUOUS"]
        self._chk(self.L.ptk_lightmap_dilate(self.h, w, h, int(passes), image.ctypes.data, owner.ctypes.data), "ptk_lightmap_dilate")
        return image, owner

    def last_bake_ms(self) -> dict:
        """HIP-event times (ms) of the last bake's kernels: coverage, ray generation, trace, scatter; waits for it."""
        t = [C.c_float(0) for _ in range(4)]
        self._chk(self.L.ptk_last_bake_ms(self.h, *(C.byref(x) for x in t)), "ptk_last_bake_ms")
        return dict(zip(("coverage_ms", "raygen_ms", "trace_ms", "scatter_ms"), (x.value for x in t)))

    # ---- adaptive ray queries and lightmap bakes ---------------------------------------------
    def trace_rays_adaptive(self, origins, dirs, max_depth: int, threshold: float, min_spp: int, step: int, max_spp: int, seed: int,
                            key_base: int = 0, lens_draws: bool = False, want_sumsq: bool = True):
        """ptk_trace_rays_adaptive: rounds of `step` samples along the rays (origins[i], dirs[i]) until each ray's noise meets
        `threshold` (the rule of render_adaptive, per ray) or it has max_spp.  Returns (sum [n, 3] float32, sumsq [n, 3] float32 or
        None, counts [n] uint32, result dict: rounds, max_count, ray_samples, active_rays); sum[i] is bit for bit
        trace_rays(first_sample 0, spp counts[i]) of ray i, the mean is sum / counts.  numpy arrays go through the host entry and
        give numpy arrays; torch tensors on the context's GPU go through the device entry with no host copy and give tensors
        (counts as int32 holding the uint32 bits).  Either way the call is synchronous."""
        flags = RAYS_LENS_DRAWS if lens_draws else 0
        args = (int(max_depth), float(threshold), int(min_spp), int(step), int(max_spp), int(seed), int(key_base) & 0xffffffff, flags)
        r = RaysAdaptiveResult()
        if hasattr(origins, "data_ptr"):
            import torch
            dev = self.device_ordinal()
            n = origins.numel() // 3
            for t in (origins, dirs):
                assert t.is_cuda and t.device.index == dev, f"tensor on {t.device}, context on device {dev}"
                assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n * 3, "[n, 3] float32 contiguous tensors"
            s1 = torch.empty((n, 3), dtype=torch.float32, device=origins.device)
            s2 = torch.empty((n, 3), dtype=torch.float32, device=origins.device) if want_sumsq else None
            counts = torch.empty((n,), dtype=torch.int32, device=origins.device)
            ptr = (lambda t: C.c_void_p(t.data_ptr()) if n and t is not None else None)
            self._chk(self.L.ptk_trace_rays_adaptive_device(self.h, n, ptr(origins), ptr(dirs), *args, ptr(s1), ptr(s2), ptr(counts),
                                                            C.byref(r)), "ptk_trace_rays_adaptive_device")
            return s1, s2, counts, r.as_dict()
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n, "as many directions as origins"
        s1 = np.empty((n, 3), np.float32)
        s2 = np.empty((n, 3), np.float32) if want_sumsq else None
        counts = np.empty((n,), np.uint32)
        ptr = (lambda a: a.ctypes.data if n and a is not None else None)
        self._chk(self.L.ptk_trace_rays_adaptive(self.h, n, ptr(o), ptr(d), *args, ptr(s1), ptr(s2), ptr(counts), C.byref(r)),
                  "ptk_trace_rays_adaptive")
        return s1, s2, counts, r.as_dict()

    def bake_lightmap_adaptive(self, width: int, height: int, offset: float, max_depth: int, threshold: float, min_spp: int, step: int,
                               max_spp: int, seed: int, uvs=None, key_base: int = 0, back: bool = False, device: bool = False):
        """ptk_bake_lightmap_adaptive: (sums [H, W, 3] float32, counts [H, W] uint32, owner [H, W] int32, result dict) of a
        width x height lightmap baked in rounds of `step` samples until each covered texel's 3x3 neighbourhood meets `threshold`,
        or max_spp; rows bottom-up; uncovered texels hold 0 / 0; the mean is sums / counts.  numpy uvs (or none) go through the host
        entry; a torch tensor for uvs - or device=True - through the device entry: tensors on the context's GPU (counts as int32
        holding the uint32 bits).  Either way the call is synchronous.  back: PTK_BAKE_BACK."""
        flags = BAKE_BACK if back else 0
        args = (float(offset), int(max_depth), float(threshold), int(min_spp), int(step), int(max_spp), int(seed), int(key_base) & 0xffffffff,
                flags)
        r = RaysAdaptiveResult()
        if device or hasattr(uvs, "data_ptr"):
            import torch
            dev = torch.device("cuda", self.device_ordinal())
            u, up = self._bake_uvs(uvs, True)
            out = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
            counts = torch.empty((height, width), dtype=torch.int32, device=dev)
            owner = torch.empty((height, width), dtype=torch.int32, device=dev)
            self._chk(self.L.ptk_bake_lightmap_adaptive_device(self.h, int(width), int(height), up, *args, C.c_void_p(out.data_ptr()),
                                                               C.c_void_p(counts.data_ptr()), C.c_void_p(owner.data_ptr()), C.byref(r)),
                      "ptk_bake_lightmap_adaptive_device")
            return out, counts, owner, r.as_dict()
        u, up = self._bake_uvs(uvs, False)
        out = np.empty((height, width, 3), np.float32)
        counts = np.empty((height, width), np.uint32)
        owner = np.empty((height, width), np.int32)
        self._chk(self.L.ptk_bake_lightmap_adaptive(self.h, int(width), int(height), up, *args, out.ctypes.data, counts.ctypes.data,
                                                    owner.ctypes.data, C.byref(r)), "ptk_bake_lightmap_adaptive")
        return out, counts, owner, r.as_dict()

    def last_rays_adaptive_ms(self) -> dict:
        """Times (ms) of the last adaptive ray query or bake: the host's wall time for the round loop, the HIP-event time of its
        rays_keyed_kernel launches, that of the other kernels of its rounds."""
        t = [C.c_float(0) for _ in range(3)]
        self._chk(self.L.ptk_last_rays_adaptive_ms(self.h, *(C.byref(x) for x in t)), "ptk_last_rays_adaptive_ms")
        return dict(zip(("total_ms", "trace_ms", "other_ms"), (x.value for x in t)))

    # ---- irradiance probes -----------------------------------------------------------------
    def bake_probes(self, positions, dirs, max_depth: int, first_sample: int, spp: int, seed: int, weight: float, key_base: int = 0,
                    radiance=None, want_radiance: bool = True):
        """ptk_bake_probes: (radiance [P, D, 3], coefs [P, 9, 3]) float32 of the probes at positions [P, 3] over the directions
        dirs [D, 3] (used as given): radiance[p, j] = the float32 in-order sum over samples [first_sample, first_sample + spp) of
        the radiance along (positions[p], dirs[j]) on the streams of (seed, RNG pixel key_base + p * D + j, sample); coefs = its
        projection onto 9 real spherical harmonics times weight (probes.sh_weight for a uniform direction set).
        numpy arrays go through the host entry (synchronous); torch tensors on the context's GPU through ptk_bake_probes_device with
        no host copy, written on the context's stream.  radiance: the table of earlier samples' sums, added to in place
        (PTK_PROBES_ACCUMULATE); coefs always comes from the whole table.  want_radiance=False (without a table): the table stays in
        the context's own buffer and None is returned for it."""
        flags = PROBES_ACCUMULATE if radiance is not None else 0
        args = (int(max_depth), int(first_sample), int(spp), int(seed), int(key_base) & 0xffffffff, flags, float(weight))
        if hasattr(positions, "data_ptr"):
            import torch
            dev = self.device_ordinal()
            P, D = positions.numel() // 3, dirs.numel() // 3
            if radiance is None and want_radiance:
                radiance = torch.empty((P, D, 3), dtype=torch.float32, device=positions.device)
            coefs = torch.empty((P, 9, 3), dtype=torch.float32, device=positions.device)
            for t, n in ((positions, P * 3), (dirs, D * 3), (radiance, P * D * 3), (coefs, P * 27)):
                if t is None:
                    continue
                assert t.is_cuda and t.device.index == dev, f"tensor on {t.device}, context on device {dev}"
                assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, "float32 contiguous tensors of [P, 3], [D, 3], [P, D, 3]"
            ptr = (lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None)
            self._chk(self.L.ptk_bake_probes_device(self.h, P, ptr(positions), D, ptr(dirs), *args, ptr(radiance), ptr(coefs)),
                      "ptk_bake_probes_device")
            return radiance, coefs
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        P, D = len(pos), len(d)
        if radiance is None and want_radiance:
            radiance = np.empty((P, D, 3), np.float32)
        assert radiance is None or (isinstance(radiance, np.ndarray) and radiance.dtype == np.float32 and radiance.flags["C_CONTIGUOUS"]
                                    and radiance.size == P * D * 3), "radiance: a C-contiguous float32 array of P x D x 3"
        coefs = np.empty((P, 9, 3), np.float32)
        ptr = (lambda a: a.ctypes.data if a is not None and a.size else None)
        self._chk(self.L.ptk_bake_probes(self.h, P, ptr(pos), D, ptr(d), *args, ptr(radiance), ptr(coefs)), "ptk_bake_probes")
        return radiance, coefs

    def probes_irradiance(self, dims, origin, spacing, coefs, points, normals):
        """ptk_probes_irradiance: [n, 3] float32 Lambertian irradiance at (points[i], normals[i]) from the probe grid of dims =
        (nx, ny, nz) probes at origin + i * spacing whose coefficients coefs [nz, ny, nx, 9, 3] (bake_probes over
        probes.grid_positions) are interpolated trilinearly; no visibility weighting.  numpy arrays: the host entry; torch tensors
        (coefs, points, normals) on the context's GPU: the device entry, on the context's stream."""
        g_dims = (C.c_int32 * 3)(*(int(n) for n in dims))
        g_origin = (C.c_float * 3)(*(float(x) for x in origin))
        g_spacing = (C.c_float * 3)(*(float(x) for x in spacing))
        count = int(g_dims[0]) * int(g_dims[1]) * int(g_dims[2]) * 27
        if hasattr(points, "data_ptr"):
            import torch
            dev = self.device_ordinal()
            n = points.numel() // 3
            out = torch.empty((n, 3), dtype=torch.float32, device=points.device)
            for t, m in ((coefs, count), (points, n * 3), (normals, n * 3)):
                assert t.is_cuda and t.device.index == dev, f"tensor on {t.device}, context on device {dev}"
                assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == m, "float32 contiguous tensors of [nz, ny, nx, 9, 3], [n, 3]"
            ptr = (lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None)
            self._chk(self.L.ptk_probes_irradiance_device(self.h, g_dims, g_origin, g_spacing, ptr(coefs), n, ptr(points), ptr(normals), ptr(out)),
                      "ptk_probes_irradiance_device")
            return out
        c = np.ascontiguousarray(coefs, dtype=np.float32)
        q = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        assert c.size == count, "coefs: dims[0] * dims[1] * dims[2] probes of 9 x 3 floats"
        assert len(nrm) == len(q), "as many normals as points"
        out = np.empty((len(q), 3), np.float32)
        ptr = (lambda a: a.ctypes.data if a.size else None)
        self._chk(self.L.ptk_probes_irradiance(self.h, g_dims, g_origin, g_spacing, ptr(c), len(q), ptr(q), ptr(nrm), ptr(out)),
                  "ptk_probes_irradiance")
        return out

    def last_probes_ms(self) -> dict:
        """HIP-event times (ms) of the last probe bake's kernels: ray generation, trace, projection; waits for it."""
        t = [C.c_float(0) for _ in range(3)]
        self._chk(self.L.ptk_last_probes_ms(self.h, *(C.byref(x) for x in t)), "ptk_last_probes_ms")
        return dict(zip(("raygen_ms", "trace_ms", "project_ms"), (x.value for x in t)))

    # ---- probe visibility ------------------------------------------------------------------
    def bake_probe_visibility(self, positions, dirs, res: int, max_dist: float, sample: int = 0, seed: int = 0, key_base: int = 0,
                              want_depth: bool = True):
        """ptk_bake_probe_visibility: (depth [P, D], moments [P, res * res, 2]) float32 of the probes at positions [P, 3] over the
        directions dirs [D, 3] (used as given): depth[p, j] = the t intersect_rays gives the ray (positions[p], dirs[j]) with
        (sample, seed, key_base + p * D + j), inf on a miss; moments[p, b * res + a] = the cos^32-weighted mean of min(depth,
        max_dist) and of its square about the direction of octahedral texel (a, b) (probes.default_max_dist for a grid).
        numpy arrays go through the host entry (synchronous); torch tensors on the context's GPU through the _device entry with no
        host copy, written on the context's stream.  want_depth=False: the table stays in the context's own buffer and None is
        returned for it."""
        args = (int(res), float(max_dist), int(sample), int(seed), int(key_base) & 0xffffffff)
        texels = int(res) * int(res) if 1 <= int(res) <= 16 else 1       # (a refused res allocates no more than that)
        if hasattr(positions, "data_ptr"):
            import torch
            dev = self.device_ordinal()
            P, D = positions.numel() // 3, dirs.numel() // 3
            depth = torch.empty((P, D), dtype=torch.float32, device=positions.device) if want_depth else None
            moments = torch.empty((P, texels, 2), dtype=torch.float32, device=positions.device)
            for t, n in ((positions, P * 3), (dirs, D * 3)):
                assert t.is_cuda and t.device.index == dev, f"tensor on {t.device}, context on device {dev}"
                assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, "float32 contiguous tensors of [P, 3], [D, 3]"
            ptr = (lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None)
            self._chk(self.L.ptk_bake_probe_visibility_device(self.h, P, ptr(positions), D, ptr(dirs), *args, ptr(depth), ptr(moments)),
                      "ptk_bake_probe_visibility_device")
            return depth, moments
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        P, D = len(pos), len(d)
        depth = np.empty((P, D), np.float32) if want_depth else None
        moments = np.empty((P, texels, 2), np.float32)
        ptr = (lambda a: a.ctypes.data if a is not None and a.size else None)
        self._chk(self.L.ptk_bake_probe_visibility(self.h, P, ptr(pos), D, ptr(d), *args, ptr(depth), ptr(moments)), "ptk_bake_probe_visibility")
        return depth, moments

    def probes_irradiance_visible(self, dims, origin, spacing, coefs, res: int, moments, points, normals, normal_bias: float = 0.0):
        """ptk_probes_irradiance_visible: probes_irradiance with every corner probe weighted by its trilinear factor, a back-face
        term and the Chebyshev bound of its depth moments - moments [nz, ny, nx, res * res, 2] of bake_probe_visibility over
        probes.grid_positions - at the point pushed normal_bias along its normal: a probe behind a wall no longer lights the room in
        front of it.  numpy arrays: the host entry; torch tensors (coefs, moments, points, normals) on the context's GPU: the device
        entry, on the context's stream."""
        g_dims = (C.c_int32 * 3)(*(int(n) for n in dims))
        g_origin = (C.c_float * 3)(*(float(x) for x in origin))
        g_spacing = (C.c_float * 3)(*(float(x) for x in spacing))
        probes = int(g_dims[0]) * int(g_dims[1]) * int(g_dims[2])
        if hasattr(points, "data_ptr"):
            import torch
            dev = self.device_ordinal()
            n = points.numel() // 3
            out = torch.empty((n, 3), dtype=torch.float32, device=points.device)
            for t, m in ((coefs, probes * 27), (moments, probes * int(res) * int(res) * 2), (points, n * 3), (normals, n * 3)):
                assert t.is_cuda and t.device.index == dev, f"tensor on {t.device}, context on device {dev}"
                assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == m, \
                    "float32 contiguous tensors of [nz, ny, nx, 9, 3], [nz, ny, nx, res * res, 2], [n, 3]"
            ptr = (lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None)
            self._chk(self.L.ptk_probes_irradiance_visible_device(self.h, g_dims, g_origin, g_spacing, ptr(coefs), int(res), ptr(moments),
                                                                  float(normal_bias), n, ptr(points), ptr(normals), ptr(out)),
                      "ptk_probes_irradiance_visible_device")
            return out
        c = np.ascontiguousarray(coefs, dtype=np.float32)
        m = np.ascontiguousarray(moments, dtype=np.float32)
        q = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        assert c.size == probes * 27, "coefs: dims[0] * dims[1] * dims[2] probes of 9 x 3 floats"
        assert m.size == probes * int(res) * int(res) * 2, "moments: dims[0] * dims[1] * dims[2] probes of res x res x 2 floats"
        assert len(nrm) == len(q), "as many normals as points"
        out = np.empty((len(q), 3), np.float32)
        ptr = (lambda a: a.ctypes.data if a.size else None)
        self._chk(self.L.ptk_probes_irradiance_visible(self.h, g_dims, g_origin, g_spacing, ptr(c), int(res), ptr(m), float(normal_bias),
                                                       len(q), ptr(q), ptr(nrm), ptr(out)), "ptk_probes_irradiance_visible")
        return out

    def last_probe_visibility_ms(self) -> dict:
        """HIP-event times (ms) of the last visibility bake's kernels: ray generation, hits, moments; waits for it."""
        t = [C.c_float(0) for _ in range(3)]
        self._chk(self.L.ptk_last_probe_visibility_ms(self.h, *(C.byref(x) for x in t)), "ptk_last_probe_visibility_ms")
        return dict(zip(("raygen_ms", "hits_ms", "moments_ms"), (x.value for x in t)))

    def read_sample_counts(self) -> np.ndarray:
        """[H][W] uint32 samples per pixel, rows bottom-up like read_accum; 0 = not owned."""
        out = np.empty((self.height, self.width), dtype=np.uint32)
        self._chk(self.L.ptk_read_sample_counts(self.h, out.ctypes.data), "ptk_read_sample_counts")
        return out

    def read_moments(self) -> np.ndarray:
        """[H][W][3] float32 sums of squared samples of the last adaptive render, rows bottom-up."""
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        self._chk(self.L.ptk_read_moments(self.h, out.ctypes.data), "ptk_read_moments")
        return out

    def synchronize(self):
        self._chk(self.L.ptk_synchronize(self.h), "ptk_synchronize")

    def read_accum(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        self._chk(self.L.ptk_read_accum(self.h, out.ctypes.data), "ptk_read_accum")
        return out

    def write_accum(self, total: np.ndarray, samples: int):
        t = np.ascontiguousarray(total, dtype=np.float32)
        assert t.shape == (self.height, self.width, 3)
        self._chk(self.L.ptk_write_accum(self.h, t.ctypes.data, samples), "ptk_write_accum")

    def resolve_rgb8(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        if out is None:
            out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        self._chk(self.L.ptk_resolve_rgb8(self.h, out.ctypes.data), "ptk_resolve_rgb8")
        return out

    def samples(self) -> int:
        return self.L.ptk_samples(self.h)

    def request_exit(self):
        self._chk(self.L.ptk_request_exit(self.h), "ptk_request_exit")

    def last_render_ms(self):
        ms = C.c_float(0); n = C.c_int(0)
        self._chk(self.L.ptk_last_render_ms(self.h, C.byref(ms), C.byref(n)), "ptk_last_render_ms")
        return ms.value, n.value

    def last_kernel_ms(self):
        t = C.c_float(0); a = C.c_float(0)
        self._chk(self.L.ptk_last_kernel_ms(self.h, C.byref(t), C.byref(a)), "ptk_last_kernel_ms")
        return t.value, a.value

    def kernel_log(self, capacity: int):
        """Start (capacity > 0) or stop (0) the log of every trace launch's duration."""
        self._chk(self.L.ptk_kernel_log(self.h, int(capacity)), "ptk_kernel_log")
        self._klog_cap = int(capacity)

    def kernel_log_read(self):
        """Durations (ms) of the trace launches since the log was started / last read, in launch order."""
        cap = max(1, getattr(self, "_klog_cap", 0))
        buf = (C.c_float * cap)(); n = C.c_int(0)
        self._chk(self.L.ptk_kernel_log_read(self.h, buf, cap, C.byref(n)), "ptk_kernel_log_read")
        return [float(buf[i]) for i in range(n.value)]

    def trace_variant(self) -> int:
        """Which trace kernel the newest launch ran: TRACE_NONE / TRACE_BVH / TRACE_FLAT / TRACE_FLAT_PLAIN."""
        v = C.c_int(0)
        self._chk(self.L.ptk_trace_variant(self.h, C.byref(v)), "ptk_trace_variant")
        return v.value

    def trace_is_lambert(self) -> bool:
        """Whether the newest launch ran the LAMBERT level of the PLAIN kernel (trace_variant gives TRACE_FLAT_PLAIN for both)."""
        v = C.c_int(0)
        self._chk(self.L.ptk_trace_is_lambert(self.h, C.byref(v)), "ptk_trace_is_lambert")
        return bool(v.value)

    def trace_unit(self) -> int:
        """Which unit's kernel the newest launch ran, for the bit-exact PLAIN kernels: UNIT_PLAIN / UNIT_RECT / UNIT_CYCLE, else UNIT_NONE."""
        v = C.c_int(0)
        self._chk(self.L.ptk_trace_unit(self.h, C.byref(v)), "ptk_trace_unit")
        return v.value

    def flat_classes(self) -> list:
        """The device's zero class of every triangle of the flat list (scenes of <= 16 triangles), in triangle order."""
        out = (C.c_int32 * 16)()
        self._chk(self.L.ptk_flat_classes(self.h, out), "ptk_flat_classes")
        return [int(v) for v in out if v >= 0]

    def flat_rect_pairs(self) -> list:
        """The kinds (1..6) of the device's pair prefix of the flat list: entry k is the pair of records 2k, 2k + 1; [] when record 0, 1 are no pair."""
        out = (C.c_int32 * 8)()
        m = C.c_int32(0)
        self._chk(self.L.ptk_flat_rect_pairs(self.h, out, C.byref(m)), "ptk_flat_rect_pairs")
        return [int(out[k]) for k in range(m.value)]

    def set_option(self, name: str, value: float):
        self._chk(self.L.ptk_set_option(self.h, name.encode(), float(value)), "ptk_set_option")

    def collect_stats(self, first_sample: int, spp: int, seed: int) -> dict:
        s = Stats()
        self._chk(self.L.ptk_collect_stats(self.h, first_sample, spp, seed, C.byref(s)), "ptk_collect_stats")
        return s.as_dict()

    def bvh_info(self):
        n = C.c_int32(); d = C.c_int32(); t = C.c_int32()
        self._chk(self.L.ptk_bvh_info(self.h, C.byref(n), C.byref(d), C.byref(t)), "ptk_bvh_info")
        return n.value, d.value, t.value

    def bvh_layout(self):
        w = C.c_int32(); b = C.c_int32(); s = C.c_int32()
        self._chk(self.L.ptk_bvh_layout(self.h, C.byref(w), C.byref(b), C.byref(s)), "ptk_bvh_layout")
        return w.value, b.value, s.value

    def download_bvh(self):
        n_nodes, _, n_tris = self.bvh_info()
        nodes = np.zeros((n_nodes, 16), np.float32); order = np.zeros(n_tris, np.int32)
        self._chk(self.L.ptk_download_bvh(self.h, nodes.ctypes.data, order.ctypes.data), "ptk_download_bvh")
        return nodes, order

    def upload_timing(self):
        t = (C.c_double * 4)(); dev = C.c_int(0)
        self._chk(self.L.ptk_upload_timing(self.h, t, C.byref(dev)), "ptk_upload_timing")
        d = dict(zip(("bvh_ms", "pack_ms", "copy_ms", "total_ms"), [round(x, 2) for x in t]))
        d["built_on_device"] = bool(dev.value)
        return d

    def node_width(self) -> int:
        return self.bvh_layout()[0]

    def accum_device_ptr(self):
        p = C.c_void_p(); b = C.c_size_t()
        self._chk(self.L.ptk_accum_device_ptr(self.h, C.byref(p), C.byref(b)), "ptk_accum_device_ptr")
        return p.value, b.value

    def rgb8_device_ptr(self):
        p = C.c_void_p(); b = C.c_size_t()
        self._chk(self.L.ptk_rgb8_device_ptr(self.h, C.byref(p), C.byref(b)), "ptk_rgb8_device_ptr")
        return p.value, b.value

    def bind_accum(self, dev_ptr: int):
        self._chk(self.L.ptk_bind_accum(self.h, dev_ptr), "ptk_bind_accum")

    def set_stream(self, stream_handle: int):
        self._chk(self.L.ptk_set_stream(self.h, stream_handle), "ptk_set_stream")

    # ---- multi-GPU exchange step -------------------------------------------------------------
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == 128
        self._chk(self.L.ptk_comm_init(self.h, C.c_char_p(unique_id), rank, world), "ptk_comm_init")

    def comm_destroy(self):
        self._chk(self.L.ptk_comm_destroy(self.h), "ptk_comm_destroy")

    def comm_info(self) -> dict:
        """rank / world / device as the library's own RCCL communicator reports them, and the context's HIP ordinal."""
        r, w, d, cd = C.c_int32(-1), C.c_int32(0), C.c_int32(-1), C.c_int32(-1)
        self._chk(self.L.ptk_comm_info(self.h, C.byref(r), C.byref(w), C.byref(d), C.byref(cd)), "ptk_comm_info")
        return {"rank": r.value, "world": w.value, "comm_device": d.value, "ctx_device": cd.value}

    def bind_out_image(self, out):
        """ptk_bind_out_image: `out` = a C-contiguous uint8 [H, W, 3] array (kept alive by the caller) or None."""
        if out is None:
            self._chk(self.L.ptk_bind_out_image(self.h, None), "ptk_bind_out_image")
            return
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size == self.width * self.height * 3
        self._chk(self.L.ptk_bind_out_image(self.h, out.ctypes.data_as(C.c_void_p)), "ptk_bind_out_image")

    def bind_out_device(self, device_ptr):
        """ptk_bind_out_device: the address of W*H*3 bytes of this GPU's memory (e.g. a torch uint8 tensor's data_ptr()) or None."""
        self._chk(self.L.ptk_bind_out_device(self.h, C.c_void_p(device_ptr) if device_ptr else None), "ptk_bind_out_device")

    def bind_gl_buffer(self, gl_buffer: int):
        """ptk_bind_gl_buffer: an OpenGL buffer object of the calling thread's current context (0 unbinds)."""
        self._chk(self.L.ptk_bind_gl_buffer(self.h, int(gl_buffer)), "ptk_bind_gl_buffer")

    def gather_accum(self, root: int = 0, comm=None):
        self._chk(self.L.ptk_gather_accum(self.h, comm, root), "ptk_gather_accum")

    def debug_stall_exchange(self, milliseconds: int):
        self._chk(self.L.ptk_debug_stall_exchange(self.h, int(milliseconds)), "ptk_debug_stall_exchange")

    def gather_wait(self):
        self._chk(self.L.ptk_gather_wait(self.h), "ptk_gather_wait")

    def read_gathered(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        self._chk(self.L.ptk_read_gathered(self.h, out.ctypes.data), "ptk_read_gathered")
        return out

    def gathered_device_ptr(self):
        p = C.c_void_p(); b = C.c_size_t()
        self._chk(self.L.ptk_gathered_device_ptr(self.h, C.byref(p), C.byref(b)), "ptk_gathered_device_ptr")
        return p.value, b.value

    def probe_pack(self, rank: int, world: int) -> np.ndarray:
        out = np.zeros(packed_floats(self.width, self.height, rank, world), np.float32)
        self._chk(self.L.ptk_probe_pack(self.h, rank, world, out.ctypes.data), "ptk_probe_pack")
        return out

    def probe_unpack(self, world: int, packed_all: np.ndarray) -> np.ndarray:
        p = np.ascontiguousarray(packed_all, np.float32)
        out = np.empty((self.height, self.width, 3), np.float32)
        self._chk(self.L.ptk_probe_unpack(self.h, world, p.ctypes.data, out.ctypes.data), "ptk_probe_unpack")
        return out

    # ---- probes ----------------------------------------------------------------------------
    def probe_hits(self, ro: np.ndarray, rd: np.ndarray):
        ro = np.ascontiguousarray(ro, np.float32); rd = np.ascontiguousarray(rd, np.float32)
        n = len(ro)
        tri = np.empty(n, np.int32); tuv = np.empty((n, 3), np.float32)
        self._chk(self.L.ptk_probe_hits(self.h, n, ro.ctypes.data, rd.ctypes.data, tri.ctypes.data, tuv.ctypes.data), "ptk_probe_hits")
        return tri, tuv

    def probe_direct(self, p, n, diffuse, tape) -> np.ndarray:
        """DirectIllumimation at surface points p with normals n, its three draws per point on `tape` ([N, 3] each)."""
        a = [np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (p, n, diffuse, tape)]
        out = np.empty_like(a[0])
        self._chk(self.L.ptk_probe_direct(self.h, len(a[0]), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, out.ctypes.data),
                  "ptk_probe_direct")
        return out

    def probe_math(self, op: int, x: np.ndarray) -> np.ndarray:
        """The kernels' arithmetic helpers on an array, from the build the "contract" option selects (op 0 rcp, 1 rcp with
        special cases, 2 sqrt, 3 normalize()'s factor 1/sqrt, 4 sin and 5 cos of the polynomial on [0, 2 pi], 6 the cycle unit's sqrt from v_rsq_f32, 7 its 1/sqrt)."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        self._chk(self.L.ptk_probe_math(self.h, op, x.size, x.ctypes.data, out.ctypes.data), "ptk_probe_math")
        return out

    def primary_dirs(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 3), np.float32)
        self._chk(self.L.ptk_probe_primary_dirs(self.h, out.ctypes.data), "ptk_probe_primary_dirs")
        return out


# ---- packed exchange layout (host-only functions of the library: no GPU needed) ---------------------------------
def packed_floats(width: int, height: int, rank: int, world: int) -> int:
    n = load().ptk_packed_floats(width, height, rank, world)
    if n < 0:
        raise PtkError("ptk_packed_floats: bad arguments")
    return int(n)


def packed_layout(width: int, height: int, rank: int, world: int) -> np.ndarray:
    """For every float of rank `rank`'s packed buffer: its index in the accumulator (W*H*3, rows bottom-up), -1 = padding."""
    idx = np.empty(packed_floats(width, height, rank, world), np.int64)
    if load().ptk_packed_layout(width, height, rank, world, idx.ctypes.data) != PTK_OK:
        raise PtkError("ptk_packed_layout: bad arguments")
    return idx


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    if load().ptk_comm_unique_id(buf) != PTK_OK:
        raise PtkError("ptk_comm_unique_id (ncclGetUniqueId) failed")
    return buf.raw

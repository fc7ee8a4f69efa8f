"""Python mirror of the reference's `PathTracer` class (reference PathTracing/src/pathtracer.h:100-130),
bound to the C++ host layer in libptk.so through the C wrapper of include/ptk_host.h.

Same method names, argument meaning, call order and (silent) error behaviour as the reference, so the
tests read like calls into the reference class:

    pt = PathTracer()
    pt.LoadObject("cornell.obj", model)          # 4x4, column-major like glm
    pt.SetMaterial(0, 0, material_floats)
    pt.BuildBVH(); pt.SetResolution((w, h)); pt.SetTraceDepth(d)
    pt.SetOutImage(rgb8); pt.ResetImage()
    pt.RenderFrame()                              # one sample per pixel, on the GPU

Nothing here computes pixels on the CPU: rendering needs libptk.so and an MI355X.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional, Sequence

import numpy as np

from . import ptk as _ptk

_f = C.POINTER(C.c_float)

HOST_SYMBOLS = [
    "pth_create", "pth_destroy", "pth_load_object", "pth_set_material", "pth_set_texture", "pth_build_bvh",
    "pth_reset_image", "pth_clear_scene", "pth_get_samples", "pth_get_triangle_count", "pth_get_trace_depth",
    "pth_set_trace_depth", "pth_set_out_image", "pth_set_out_gl_buffer", "pth_set_out_device_image", "pth_set_resolution", "pth_get_resolution", "pth_num_objects",
    "pth_num_elements", "pth_name", "pth_set_camera", "pth_set_projection", "pth_set_focal_dist", "pth_set_aperture",
    "pth_render_frame", "pth_exit", "pth_set_seed", "pth_set_tile", "pth_render_frames", "pth_read_accum",
    "pth_last_error", "pth_context", "pth_staged_scene", "pth_load_scene_file", "pth_pts_roundtrip",
    "pth_trs_matrix", "pth_euler_camera", "pth_triangle_init", "pth_image_load", "pth_image_data", "pth_image_tex2d",
    "pth_export_png", "pth_render_adaptive", "pth_read_sample_counts",
    "pth_render_features", "pth_read_feature", "pth_pick", "pth_set_object_transform", "pth_trace_rays", "pth_get_camera",
    "pth_bake_lightmap", "pth_bake_coverage", "pth_lightmap_dilate", "pth_bake_probes", "pth_sample_probes",
    "pth_bake_probe_visibility", "pth_sample_probes_visible",
    "pth_trace_rays_adaptive", "pth_bake_lightmap_adaptive", "pth_intersect_rays", "pth_occluded_rays", "pth_closest_points", "pth_overlap_boxes", "pth_overlap_spheres",
    "pth_crossings_rays", "pth_contains_points", "pth_signed_distance", "pth_multihit_rays", "pth_nearest_triangles",
    "pth_sample_surface", "pth_set_surface_weights", "pth_surface_info", "pth_surface_attributes",
    "pth_denoise_frame", "pth_read_denoised", "pth_resolve_denoised", "pth_temporal_frame", "pth_read_temporal", "pth_get_view",
    "pth_track_motion", "pth_temporal_frame_moving", "pth_read_motion", "pth_temporal_frame_moments", "pth_temporal_variance",
    "pth_read_temporal_variance", "pth_denoise_temporal", "pth_get_object_transform",
    "pth_display_frame", "pth_read_display", "pth_display_state", "pth_display_reset",
    "pth_render_guides", "pth_read_guide", "pth_upsample_frame", "pth_read_upsampled",
]

_bound = False
_bind_lock = threading.Lock()


def lib() -> C.CDLL:
    L = _ptk.load()
    if _bound:
        return L
    with _bind_lock:                 # (the prototypes are complete before any thread's first call: a pointer returned through
        return _bind_locked(L)       # ctypes' default int would be cut to 32 bits)


def _bind_locked(L) -> C.CDLL:
    global _bound
    if _bound:
        return L
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.pth_create.restype = vp; L.pth_create.argtypes = [i32]
    L.pth_destroy.restype = None; L.pth_destroy.argtypes = [vp]
    L.pth_load_object.restype = None; L.pth_load_object.argtypes = [vp, C.c_char_p, _f]
    L.pth_set_object_transform.restype = None; L.pth_set_object_transform.argtypes = [vp, i32, _f]
    L.pth_set_material.restype = None; L.pth_set_material.argtypes = [vp, i32, i32, _f]
    L.pth_set_texture.restype = None; L.pth_set_texture.argtypes = [vp, i32, i32, i32, C.c_char_p]
    for n in ("pth_build_bvh", "pth_reset_image", "pth_clear_scene", "pth_render_frame", "pth_exit"):
        getattr(L, n).restype = None; getattr(L, n).argtypes = [vp]
    for n in ("pth_get_samples", "pth_get_triangle_count", "pth_get_trace_depth", "pth_num_objects"):
        getattr(L, n).restype = i32; getattr(L, n).argtypes = [vp]
    L.pth_num_elements.restype = i32; L.pth_num_elements.argtypes = [vp, i32]
    L.pth_name.restype = i32; L.pth_name.argtypes = [vp, i32, i32, C.c_char_p, i32]
    L.pth_set_trace_depth.restype = None; L.pth_set_trace_depth.argtypes = [vp, i32]
    L.pth_set_out_image.restype = None; L.pth_set_out_image.argtypes = [vp, vp]
    L.pth_set_out_gl_buffer.restype = None; L.pth_set_out_gl_buffer.argtypes = [vp, C.c_uint]
    L.pth_set_out_device_image.restype = None; L.pth_set_out_device_image.argtypes = [vp, vp]
    L.pth_set_resolution.restype = None; L.pth_set_resolution.argtypes = [vp, i32, i32]
    L.pth_get_resolution.restype = None; L.pth_get_resolution.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.pth_set_camera.restype = None; L.pth_set_camera.argtypes = [vp, _f, _f, _f]
    L.pth_set_projection.restype = None; L.pth_set_projection.argtypes = [vp, f32, f32]
    L.pth_set_focal_dist.restype = None; L.pth_set_focal_dist.argtypes = [vp, f32]
    L.pth_set_aperture.restype = None; L.pth_set_aperture.argtypes = [vp, f32]
    L.pth_set_seed.restype = None; L.pth_set_seed.argtypes = [vp, C.c_uint64]
    L.pth_set_tile.restype = None; L.pth_set_tile.argtypes = [vp, i32, i32]
    L.pth_render_frames.restype = None; L.pth_render_frames.argtypes = [vp, i32]
    L.pth_read_accum.restype = i32; L.pth_read_accum.argtypes = [vp, vp]
    L.pth_render_adaptive.restype = i32
    L.pth_render_adaptive.argtypes = [vp, f32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_ptk.AdaptiveResult)]
    L.pth_read_sample_counts.restype = i32; L.pth_read_sample_counts.argtypes = [vp, vp]
    L.pth_render_features.restype = i32; L.pth_render_features.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.pth_read_feature.restype = i32; L.pth_read_feature.argtypes = [vp, i32, vp]
    L.pth_pick.restype = i32; L.pth_pick.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    try:
        L.pth_get_camera.restype = None; L.pth_get_camera.argtypes = [vp, _f, _f, _f]
        L.pth_trace_rays.restype = i32
        L.pth_trace_rays.argtypes = [vp, i32, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp]
        L.pth_bake_lightmap.restype = i32
        L.pth_bake_lightmap.argtypes = [vp, i32, i32, vp, f32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
        L.pth_bake_coverage.restype = i32; L.pth_bake_coverage.argtypes = [vp, i32, i32, vp, vp, vp, vp]
        L.pth_lightmap_dilate.restype = i32; L.pth_lightmap_dilate.argtypes = [vp, i32, i32, i32, vp, vp]
        L.pth_bake_probes.restype = i32
        L.pth_bake_probes.argtypes = [vp, i32, vp, i32, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32, vp, vp]
        L.pth_sample_probes.restype = i32; L.pth_sample_probes.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp]
        L.pth_bake_probe_visibility.restype = i32
        L.pth_bake_probe_visibility.argtypes = [vp, i32, vp, i32, vp, i32, f32, C.c_uint32, C.c_uint32, vp, vp]
        L.pth_sample_probes_visible.restype = i32
        L.pth_sample_probes_visible.argtypes = [vp, vp, vp, vp, vp, i32, vp, f32, i32, vp, vp, vp]
        u32, res = C.c_uint32, C.POINTER(_ptk.RaysAdaptiveResult)
        L.pth_trace_rays_adaptive.restype = i32
        L.pth_trace_rays_adaptive.argtypes = [vp, i32, vp, vp, f32, u32, u32, u32, u32, u32, vp, vp, vp, res]
        L.pth_bake_lightmap_adaptive.restype = i32
        L.pth_bake_lightmap_adaptive.argtypes = [vp, i32, i32, vp, f32, f32, u32, u32, u32, u32, u32, vp, vp, vp, res]
        L.pth_intersect_rays.restype = i32; L.pth_intersect_rays.argtypes = [vp, i32, vp, vp, u32, u32, vp, vp, vp, vp]
        L.pth_occluded_rays.restype = i32; L.pth_occluded_rays.argtypes = [vp, i32, vp, vp, vp, u32, u32, vp]
        L.pth_closest_points.restype = i32; L.pth_closest_points.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
        for fn in (L.pth_overlap_boxes, L.pth_overlap_spheres):
            fn.restype = i32; fn.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp]
        L.pth_crossings_rays.restype = i32; L.pth_crossings_rays.argtypes = [vp, i32, vp, vp, vp, vp, vp]
        L.pth_multihit_rays.restype = i32; L.pth_multihit_rays.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
        L.pth_nearest_triangles.restype = i32; L.pth_nearest_triangles.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]
        L.pth_sample_surface.restype = i32; L.pth_sample_surface.argtypes = [vp, i32, u32, u32, vp, vp, vp, vp, vp]
        L.pth_surface_attributes.restype = i32; L.pth_surface_attributes.argtypes = [vp, i32] + [vp] * 12
        L.pth_set_surface_weights.restype = i32; L.pth_set_surface_weights.argtypes = [vp, vp]
        L.pth_surface_info.restype = i32; L.pth_surface_info.argtypes = [vp, vp, vp, vp, vp]
        L.pth_contains_points.restype = i32; L.pth_contains_points.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp]
        L.pth_signed_distance.restype = i32; L.pth_signed_distance.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]
        L.pth_denoise_frame.restype = i32; L.pth_denoise_frame.argtypes = [vp, C.POINTER(_ptk.DenoiseParams), i32]
        L.pth_read_denoised.restype = i32; L.pth_read_denoised.argtypes = [vp, vp]
        L.pth_resolve_denoised.restype = i32; L.pth_resolve_denoised.argtypes = [vp, vp]
        L.pth_temporal_frame.restype = i32; L.pth_temporal_frame.argtypes = [vp, C.POINTER(_ptk.TemporalParams), i32]
        L.pth_read_temporal.restype = i32; L.pth_read_temporal.argtypes = [vp, vp, vp]
        L.pth_get_view.restype = i32; L.pth_get_view.argtypes = [vp, C.POINTER(_ptk.View)]
        L.pth_get_object_transform.restype = i32; L.pth_get_object_transform.argtypes = [vp, i32, C.POINTER(C.c_float)]
        L.pth_track_motion.restype = None; L.pth_track_motion.argtypes = [vp, i32]
        L.pth_temporal_frame_moving.restype = i32; L.pth_temporal_frame_moving.argtypes = [vp, C.POINTER(_ptk.TemporalParams), i32]
        L.pth_temporal_frame_moments.restype = i32; L.pth_temporal_frame_moments.argtypes = [vp, C.POINTER(_ptk.TemporalParams), i32, i32]
        L.pth_temporal_variance.restype = i32; L.pth_temporal_variance.argtypes = [vp, C.POINTER(_ptk.VarianceParams)]
        L.pth_read_temporal_variance.restype = i32; L.pth_read_temporal_variance.argtypes = [vp, vp, vp]
        L.pth_denoise_temporal.restype = i32; L.pth_denoise_temporal.argtypes = [vp, C.POINTER(_ptk.DenoiseParams), i32]
        L.pth_display_frame.restype = i32; L.pth_display_frame.argtypes = [vp, i32, C.POINTER(_ptk.DisplayParams)]
        L.pth_read_display.restype = i32; L.pth_read_display.argtypes = [vp, vp]
        L.pth_display_state.restype = i32; L.pth_display_state.argtypes = [vp, C.POINTER(_ptk.DisplayState)]
        L.pth_display_reset.restype = i32; L.pth_display_reset.argtypes = [vp]
        L.pth_render_guides.restype = i32; L.pth_render_guides.argtypes = [vp, i32, i32]
        L.pth_read_guide.restype = i32; L.pth_read_guide.argtypes = [vp, i32, vp]
        L.pth_upsample_frame.restype = i32; L.pth_upsample_frame.argtypes = [vp, i32, C.POINTER(_ptk.UpsampleParams)]
        L.pth_read_upsampled.restype = i32; L.pth_read_upsampled.argtypes = [vp, vp, vp]
        L.pth_read_motion.restype = i32; L.pth_read_motion.argtypes = [vp, vp, vp, vp]
    except AttributeError:
        if _ptk.LIB_PATH.endswith("libptk.so"):   # (an older build loaded through PTK_DEV_TOOLS for an A/B may lack the newest entry points)
            raise
    L.pth_last_error.restype = C.c_char_p; L.pth_last_error.argtypes = [vp]
    L.pth_context.restype = vp; L.pth_context.argtypes = [vp]
    L.pth_staged_scene.restype = C.POINTER(_ptk.SceneDesc); L.pth_staged_scene.argtypes = [vp]
    L.pth_load_scene_file.restype = i32; L.pth_load_scene_file.argtypes = [vp, C.c_char_p]
    L.pth_pts_roundtrip.restype = i32; L.pth_pts_roundtrip.argtypes = [C.c_char_p, C.c_char_p]
    L.pth_trs_matrix.restype = None; L.pth_trs_matrix.argtypes = [_f, _f, _f, _f]
    L.pth_euler_camera.restype = None; L.pth_euler_camera.argtypes = [_f, _f]
    L.pth_triangle_init.restype = None; L.pth_triangle_init.argtypes = [_f, _f]
    L.pth_image_load.restype = i32; L.pth_image_load.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(i32)]
    L.pth_image_data.restype = None; L.pth_image_data.argtypes = [vp]
    L.pth_image_tex2d.restype = None; L.pth_image_tex2d.argtypes = [f32, f32, _f]
    L.pth_export_png.restype = i32; L.pth_export_png.argtypes = [C.c_char_p, vp, i32, i32]
    _bound = True
    return L


def _fp(a):
    return a.ctypes.data_as(_f)


def _f3(v):
    return np.ascontiguousarray(v, dtype=np.float32).reshape(3)


class _PinnedBuffer:
    """Owner of one ptk_host_alloc block, exposed to numpy through the array interface."""

    def __init__(self, shape):
        from . import ptk as _ptk
        self._L = _ptk.load()
        n = int(np.prod(shape))
        self._p = self._L.ptk_host_alloc(n)
        if not self._p:
            raise MemoryError("ptk_host_alloc failed (no HIP device?)")
        self.__array_interface__ = {"shape": tuple(shape), "typestr": "|u1", "data": (self._p, False), "version": 3}

    def __del__(self):
        if getattr(self, "_p", None):
            self._L.ptk_host_free(self._p)
            self._p = None


class PathTracer:
    """The reference's PathTracer API (method names kept verbatim) + the marked extensions."""

    def __init__(self, device: int = 0):
        self.L = lib()
        self.h = self.L.pth_create(device)
        if not self.h:
            raise _ptk.PtkError("pth_create failed")
        self._out = None

    def close(self):
        if getattr(self, "h", None):
            self.L.pth_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference API -------------------------------------------------------------------------
    def LoadObject(self, file: str, model=None):
        M = np.eye(4, dtype=np.float32) if model is None else np.ascontiguousarray(model, dtype=np.float32)
        self.L.pth_load_object(self.h, file.encode(), _fp(M.reshape(16)))

    def _set_tex(self, slot, objId, elementId, file):
        self.L.pth_set_texture(self.h, objId, elementId, slot, file.encode())

    def SetDiffuseTextureForElement(self, objId, elementId, file): self._set_tex(0, objId, elementId, file)
    def SetNormalTextureForElement(self, objId, elementId, file): self._set_tex(1, objId, elementId, file)
    def SetEmissTextureForElement(self, objId, elementId, file): self._set_tex(2, objId, elementId, file)
    def SetRoughnessTextureForElement(self, objId, elementId, file): self._set_tex(3, objId, elementId, file)
    def SetMetallicTextureForElement(self, objId, elementId, file): self._set_tex(4, objId, elementId, file)
    def SetOpacityTextureForElement(self, objId, elementId, file): self._set_tex(5, objId, elementId, file)

    def SetMaterial(self, objId: int, elementId: int, material):
        """material: 15 floats (type, diffuse rgb, specular rgb, emissive rgb, emissiveIntensity, roughness,
        reflectiveness, translucency, ior) or scenes.MaterialDesc."""
        m = material.as_floats() if hasattr(material, "as_floats") else np.ascontiguousarray(material, dtype=np.float32)
        self.L.pth_set_material(self.h, objId, elementId, _fp(m))

    def BuildBVH(self): self.L.pth_build_bvh(self.h)
    def ResetImage(self): self.L.pth_reset_image(self.h)
    def ClearScene(self): self.L.pth_clear_scene(self.h)
    def GetSamples(self) -> int: return self.L.pth_get_samples(self.h)
    def GetTriangleCount(self) -> int: return self.L.pth_get_triangle_count(self.h)
    def GetTraceDepth(self) -> int: return self.L.pth_get_trace_depth(self.h)
    def SetTraceDepth(self, depth: int): self.L.pth_set_trace_depth(self.h, depth)

    def SetOutImage(self, out: Optional[np.ndarray]):
        """out: caller-owned uint8 array of W*H*3 (rows bottom-up), written by every RenderFrame()."""
        if out is not None:
            assert out.dtype == np.uint8 and out.flags.c_contiguous
        self.L.pth_set_out_image(self.h, out.ctypes.data if out is not None else None)
        self._out = out                 # (after the call: the previous buffer - this may be its last reference - is unbound before it is freed)

    def SetOutGLBuffer(self, gl_buffer: int):
        """Extension: the 8-bit image goes into an OpenGL buffer object of the current context (0 switches back)."""
        self.L.pth_set_out_gl_buffer(self.h, int(gl_buffer))
        if gl_buffer:
            self._out = None

    def SetOutDeviceImage(self, device_ptr):
        """Extension: the 8-bit image goes into W*H*3 bytes of this GPU's memory (an address, e.g. a torch uint8 tensor's
        data_ptr(), kept alive by the caller); None switches back."""
        self.L.pth_set_out_device_image(self.h, C.c_void_p(device_ptr) if device_ptr else None)
        if device_ptr:
            self._out = None

    def AllocOutImage(self) -> np.ndarray:
        """A page-locked W*H*3 uint8 hand-off buffer (ptk_host_alloc) for SetOutImage: RenderFrame()'s copy into
        it is a single DMA transfer.  Freed when the returned array (and its views) are garbage-collected."""
        w, h = self.GetResolution()
        return np.asarray(_PinnedBuffer((h, w, 3)))

    def SetResolution(self, res: Sequence[int]): self.L.pth_set_resolution(self.h, int(res[0]), int(res[1]))

    def GetResolution(self):
        w = C.c_int(); h = C.c_int()
        self.L.pth_get_resolution(self.h, C.byref(w), C.byref(h))
        return w.value, h.value

    def GetNames(self, obj: int):
        """(object name, [element names]) of loaded object `obj` (PathTracerLoader::Object, pathtracer.cpp:49-62)."""
        def one(e):
            buf = C.create_string_buffer(1024)
            n = self.L.pth_name(self.h, obj, e, buf, 1024)
            return None if n < 0 else buf.value.decode("latin-1")
        return one(-1), [one(e) for e in range(self.L.pth_num_elements(self.h, obj))]

    def GetLoadedObjects(self):
        return [self.L.pth_num_elements(self.h, i) for i in range(self.L.pth_num_objects(self.h))]

    def SetCamera(self, pos, dir, up): self.L.pth_set_camera(self.h, _fp(_f3(pos)), _fp(_f3(dir)), _fp(_f3(up)))
    def SetProjection(self, f: float, fovy: float): self.L.pth_set_projection(self.h, f, fovy)
    def SetCameraFocalDist(self, dist: float): self.L.pth_set_focal_dist(self.h, dist)
    def SetCameraAperture(self, aperture: float): self.L.pth_set_aperture(self.h, aperture)
    def RenderFrame(self): self.L.pth_render_frame(self.h)
    def Exit(self): self.L.pth_exit(self.h)

    # ---- extensions ----------------------------------------------------------------------------
    def SetSeed(self, seed: int): self.L.pth_set_seed(self.h, seed)
    def SetTile(self, rank: int, world: int): self.L.pth_set_tile(self.h, rank, world)

    def SetObjectTransform(self, objId: int, model):
        """Extension: stage object `objId` again under the 4x4 `model` ([column][row], as LoadObject takes it).  After BuildBVH()
        the next render call moves its triangles on the device and refits the BVH (include/ptk.h ptk_update_geometry)."""
        M = np.ascontiguousarray(model, dtype=np.float32)
        self.L.pth_set_object_transform(self.h, int(objId), _fp(M.reshape(16)))

    def GetObjectTransform(self, objId: int) -> np.ndarray:
        """Extension: the 4x4 matrix ([column][row]) object `objId` is staged under - LoadObject's or the last SetObjectTransform's."""
        M = np.zeros(16, np.float32)
        if not self.L.pth_get_object_transform(self.h, int(objId), _fp(M)):
            raise _ptk.PtkError(f"GetObjectTransform: no object {objId}")
        return M.reshape(4, 4)

    def RenderFrames(self, count: int): self.L.pth_render_frames(self.h, count)

    def RenderAdaptive(self, threshold: float, min_spp: int, step: int, max_spp: int) -> dict:
        """ResetImage() + adaptive render (include/ptk.h ptk_render_adaptive) with this tracer's seed; the 8-bit image goes to
        the hand-off target.  Returns rounds, max_count, pixel_samples, active_pixels."""
        r = _ptk.AdaptiveResult()
        if not self.L.pth_render_adaptive(self.h, float(threshold), int(min_spp), int(step), int(max_spp), C.byref(r)):
            raise _ptk.PtkError("RenderAdaptive failed: " + self.LastError())
        return r.as_dict()

    def ReadSampleCounts(self) -> np.ndarray:
        """[H][W] uint32 samples per pixel, rows bottom-up like ReadAccumulation(); 0 = not owned."""
        w, h = self.GetResolution()
        out = np.empty((h, w), np.uint32)
        if not self.L.pth_read_sample_counts(self.h, out.ctypes.data):
            raise _ptk.PtkError("ReadSampleCounts failed: " + self.LastError())
        return out

    def RenderFeatures(self, mask: int, sample: int = 0):
        """First-hit feature planes (include/ptk.h ptk_render_features) of the planes in `mask` (bit k = ptk.FEAT_*), for sample
        `sample` of this tracer's seed; pending edits apply as for RenderFrame(), the image is not touched."""
        if not self.L.pth_render_features(self.h, int(mask), int(sample)):
            raise _ptk.PtkError("RenderFeatures failed: " + self.LastError())

    def ReadFeature(self, feature: int) -> np.ndarray:
        """One plane of the last RenderFeatures(): [H, W] or [H, W, c], float32 or int32, rows bottom-up."""
        w, h = self.GetResolution()
        out = _ptk.feature_array(feature, w, h)
        if not self.L.pth_read_feature(self.h, int(feature), out.ctypes.data):
            raise _ptk.PtkError("ReadFeature failed: " + self.LastError())
        return out

    def DenoiseFrame(self, params=None, variance: bool = False):
        """Extension: the a-trous denoiser (include/ptk.h ptk_denoise_frame) over the frame as last rendered; variance: the
        variance-guided mode, legal after RenderAdaptive().  params: ptk.DenoiseParams or a dict of its fields; None takes
        ptk.denoise_defaults for the staged scene's extent.  The guide planes are rendered first (sample 0 of this tracer's seed)
        when they are missing or stale; the image and the sample count are not touched."""
        if params is None:
            v = np.asarray(self.StagedScene()["verts"], np.float64).reshape(-1, 3)
            params = _ptk.denoise_defaults(float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))) if len(v) else 1.0, variance)
        prm = _ptk._denoise_params(params)
        if not self.L.pth_denoise_frame(self.h, C.byref(prm), 1 if variance else 0):
            raise _ptk.PtkError("DenoiseFrame failed: " + self.LastError())

    def ReadDenoised(self) -> np.ndarray:
        """[H][W][3] float32, the last DenoiseFrame()'s result, rows bottom-up like ReadAccumulation()."""
        w, h = self.GetResolution()
        out = np.empty((h, w, 3), np.float32)
        if not self.L.pth_read_denoised(self.h, out.ctypes.data):
            raise _ptk.PtkError("ReadDenoised failed: " + self.LastError())
        return out

    def ResolveDenoised(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The 8-bit resolve of the denoised frame, [H][W][3] uint8 in the out image's layout."""
        w, h = self.GetResolution()
        if out is None:
            out = np.empty((h, w, 3), np.uint8)
        if not self.L.pth_resolve_denoised(self.h, out.ctypes.data):
            raise _ptk.PtkError("ResolveDenoised failed: " + self.LastError())
        return out

    denoise_frame, read_denoised, resolve_denoised_rgb8 = DenoiseFrame, ReadDenoised, ResolveDenoised

    def TemporalFrame(self, params=None, reset: bool = False):
        """Extension: temporal reprojection (include/ptk.h ptk_temporal_frame) over the frame as last rendered: the previous
        TemporalFrame()'s result is carried into the current camera's frame and blended with it by sample counts; reset drops that
        history.  params: ptk.TemporalParams or a dict of its fields; None takes ptk.temporal_defaults for the staged scene's
        extent.  The guide planes are rendered first (sample 0 of this tracer's seed) when they are missing or stale; the image
        and the sample count are not touched."""
        prm = self._temporal_params(params)
        if not self.L.pth_temporal_frame(self.h, C.byref(prm), 1 if reset else 0):
            raise _ptk.PtkError("TemporalFrame failed: " + self.LastError())

    def _temporal_params(self, params):
        if params is None:
            v = np.asarray(self.StagedScene()["verts"], np.float64).reshape(-1, 3)
            params = _ptk.temporal_defaults(float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))) if len(v) else 1.0)
        return _ptk._temporal_params(params)

    def TrackMotion(self, on: bool = True):
        """Extension: with tracking on, the render call that applies SetObjectTransform() edits first keeps the resident geometry
        (include/ptk.h ptk_geometry_snapshot) - once per TemporalFrame*() call - as the previous geometry of TemporalFrameMoving()."""
        self.L.pth_track_motion(self.h, 1 if on else 0)

    def TemporalFrameMoving(self, params=None, reset: bool = False):
        """Extension: TemporalFrame() over objects that move (include/ptk.h ptk_temporal_frame_moving): the history follows the
        triangles SetObjectTransform() moved since the last TemporalFrame*() call (TrackMotion).  Shares history, result and
        ReadTemporal() with TemporalFrame(); ReadMotion() gives where the surface points were."""
        prm = self._temporal_params(params)
        if not self.L.pth_temporal_frame_moving(self.h, C.byref(prm), 1 if reset else 0):
            raise _ptk.PtkError("TemporalFrameMoving failed: " + self.LastError())

    def ReadMotion(self):
        """(prev_position [H][W][3], prev_normal [H][W][3], motion [H][W][2]) float32 of the last TemporalFrameMoving(), rows
        bottom-up: motion is (columns, top-down rows) from the pixel to where its surface point was under the history's view; NaN
        where the pixel sees nothing or there was no history."""
        w, h = self.GetResolution()
        pp = np.empty((h, w, 3), np.float32); pn = np.empty((h, w, 3), np.float32); mv = np.empty((h, w, 2), np.float32)
        if not self.L.pth_read_motion(self.h, pp.ctypes.data, pn.ctypes.data, mv.ctypes.data):
            raise _ptk.PtkError("ReadMotion failed: " + self.LastError())
        return pp, pn, mv

    def ReadTemporal(self):
        """(color [H][W][3], count [H][W]) float32, the last TemporalFrame()'s result, rows bottom-up like ReadAccumulation()."""
        w, h = self.GetResolution()
        color = np.empty((h, w, 3), np.float32); count = np.empty((h, w), np.float32)
        if not self.L.pth_read_temporal(self.h, color.ctypes.data, count.ctypes.data):
            raise _ptk.PtkError("ReadTemporal failed: " + self.LastError())
        return color, count

    def GetView(self) -> "_ptk.View":
        """ptk.View: the image-plane set-up of the device layer's current camera and resolution (include/ptk.h ptk_get_view)."""
        v = _ptk.View()
        if not self.L.pth_get_view(self.h, C.byref(v)):
            raise _ptk.PtkError("GetView failed: " + self.LastError())
        return v

    def _extent(self) -> float:
        v = np.asarray(self.StagedScene()["verts"], np.float64).reshape(-1, 3)
        return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))) if len(v) else 1.0

    def TemporalFrameMoments(self, params=None, reset: bool = False, moving: bool = False):
        """Extension: TemporalFrame() - moving: TemporalFrameMoving() - that also carries the first and second moment of
        demodulated luminance (include/ptk.h ptk_temporal_frame_moments).  Shares history, result and ReadTemporal() with the
        two; a moments call behind a plain one starts its history over.  TemporalVariance() and DenoiseTemporal() follow it."""
        prm = self._temporal_params(params)
        if not self.L.pth_temporal_frame_moments(self.h, C.byref(prm), 1 if reset else 0, 1 if moving else 0):
            raise _ptk.PtkError("TemporalFrameMoments failed: " + self.LastError())

    def TemporalVariance(self, params=None):
        """Extension: the per-pixel variance of the accumulated demodulated luminance from the moments of the last
        TemporalFrameMoments() (include/ptk.h ptk_temporal_variance).  params: ptk.VarianceParams or a dict of its fields; None
        takes ptk.variance_defaults for the staged scene's extent."""
        prm = _ptk._variance_params(_ptk.variance_defaults(self._extent()) if params is None else params)
        if not self.L.pth_temporal_variance(self.h, C.byref(prm)):
            raise _ptk.PtkError("TemporalVariance failed: " + self.LastError())

    def ReadTemporalVariance(self, variance: bool = True):
        """(moments [H][W][2], variance [H][W]) float32 of the last TemporalFrameMoments() and TemporalVariance(), rows bottom-up;
        variance=False: (moments, None), legal before TemporalVariance()."""
        w, h = self.GetResolution()
        mom = np.empty((h, w, 2), np.float32)
        var = np.empty((h, w), np.float32) if variance else None
        if not self.L.pth_read_temporal_variance(self.h, mom.ctypes.data, var.ctypes.data if variance else None):
            raise _ptk.PtkError("ReadTemporalVariance failed: " + self.LastError())
        return mom, var

    def DenoiseTemporal(self, params=None, variance: bool = True):
        """Extension: the a-trous denoiser over the last TemporalFrame*() result, on the device (include/ptk.h
        ptk_denoise_temporal); variance: guided by TemporalVariance()'s plane.  params: ptk.DenoiseParams or a dict of its fields;
        None takes ptk.denoise_defaults for the staged scene's extent.  ReadDenoised() and ResolveDenoised() give the result."""
        prm = _ptk._denoise_params(_ptk.denoise_defaults(self._extent(), variance) if params is None else params)
        if not self.L.pth_denoise_temporal(self.h, C.byref(prm), 1 if variance else 0):
            raise _ptk.PtkError("DenoiseTemporal failed: " + self.LastError())

    def DisplayFrame(self, source: int = _ptk.DISPLAY_ACCUM, params=None):
        """Extension: the display transform (include/ptk.h ptk_display_frame) - exposure, given or metered and adapted on the
        device from call to call, a tone curve and the sRGB transfer - over the frame as last rendered (ptk.DISPLAY_ACCUM), the
        DenoiseFrame() / DenoiseTemporal() result (ptk.DISPLAY_DENOISED) or the TemporalFrame*() result (ptk.DISPLAY_TEMPORAL).
        params: ptk.DisplayParams or a dict of its fields; None takes ptk.display_defaults.  ReadDisplay() gives the bytes."""
        prm = _ptk._display_params(params)
        if not self.L.pth_display_frame(self.h, int(source), C.byref(prm)):
            raise _ptk.PtkError("DisplayFrame failed: " + self.LastError())

    def ReadDisplay(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """[H][W][3] uint8, the last DisplayFrame()'s result, in the out image's layout."""
        if out is None:
            w, h = self.GetResolution()
            out = np.empty((h, w, 3), np.uint8)
        if not self.L.pth_read_display(self.h, out.ctypes.data):
            raise _ptk.PtkError("ReadDisplay failed: " + self.LastError())
        return out

    def DisplayState(self) -> dict:
        """The exposure state behind the last DisplayFrame() (Context.display_state)."""
        st = _ptk.DisplayState()
        if not self.L.pth_display_state(self.h, C.byref(st)):
            raise _ptk.PtkError("DisplayState failed: " + self.LastError())
        return st.as_dict()

    def ResetDisplay(self):
        """Forgets the exposure state: the next metered DisplayFrame() lands on its target."""
        if not self.L.pth_display_reset(self.h):
            raise _ptk.PtkError("ResetDisplay failed: " + self.LastError())

    display_frame, read_display, display_state, display_reset = DisplayFrame, ReadDisplay, DisplayState, ResetDisplay

    def RenderGuides(self, width: int, height: int):
        """Extension: guide planes at a resolution of their own (include/ptk.h ptk_render_guides) - the first-hit planes MATERIAL,
        POSITION, NORMAL and ALBEDO of the current camera at width x height, whatever SetResolution set; sample 0 of this tracer's
        seed.  The image and the sample count are not touched.  UpsampleFrame() brings the frame up to this resolution."""
        if not self.L.pth_render_guides(self.h, int(width), int(height)):
            raise _ptk.PtkError("RenderGuides failed: " + self.LastError())
        self._guide_size = (int(width), int(height))

    def ReadGuide(self, feature: int) -> np.ndarray:
        """One plane of the last RenderGuides(): [H, W] or [H, W, c] at the guides' size, rows bottom-up."""
        w, h = getattr(self, "_guide_size", (0, 0))
        out = _ptk.feature_array(feature, w, h)
        if not self.L.pth_read_guide(self.h, int(feature), out.ctypes.data if out.size else None):
            raise _ptk.PtkError("ReadGuide failed: " + self.LastError())
        return out

    def UpsampleFrame(self, source: int = _ptk.UPSAMPLE_ACCUM, params=None):
        """Extension: guided upsampling (include/ptk.h ptk_upsample_frame) of the frame as last rendered (ptk.UPSAMPLE_ACCUM), the
        DenoiseFrame() / DenoiseTemporal() result (ptk.UPSAMPLE_DENOISED) or the TemporalFrame*() result (ptk.UPSAMPLE_TEMPORAL)
        up to the resolution of the last RenderGuides().  params: ptk.UpsampleParams or a dict of its fields; None takes
        ptk.upsample_defaults for the staged scene's extent.  The frame's own guide planes are rendered first (sample 0 of this
        tracer's seed) when they are missing or stale.  ReadUpsampled() gives the result."""
        prm = _ptk._upsample_params(_ptk.upsample_defaults(self._extent()) if params is None else params)
        if not self.L.pth_upsample_frame(self.h, int(source), C.byref(prm)):
            raise _ptk.PtkError("UpsampleFrame failed: " + self.LastError())

    def ReadUpsampled(self):
        """(color [H][W][3] float32, class [H][W] int32 - 0 bilinear, 1 wide ring, 2 a hole) of the last UpsampleFrame(), at the
        guides' size, rows bottom-up."""
        w, h = getattr(self, "_guide_size", (0, 0))
        color = np.empty((h, w, 3), np.float32); cls = np.empty((h, w), np.int32)
        if not self.L.pth_read_upsampled(self.h, color.ctypes.data if color.size else None, cls.ctypes.data if cls.size else None):
            raise _ptk.PtkError("ReadUpsampled failed: " + self.LastError())
        return color, cls

    render_guides, read_guide, upsample_frame, read_upsampled = RenderGuides, ReadGuide, UpsampleFrame, ReadUpsampled
    temporal_frame, read_temporal, get_view = TemporalFrame, ReadTemporal, GetView
    temporal_frame_moments, temporal_variance, read_temporal_variance, denoise_temporal = (TemporalFrameMoments, TemporalVariance,
                                                                                          ReadTemporalVariance, DenoiseTemporal)
    track_motion, temporal_frame_moving, read_motion = TrackMotion, TemporalFrameMoving, ReadMotion

    def Pick(self, x: int, y: int):
        """(object, element, triangle) under pixel (x, y), y from the top row; (-1, -1, -1) where the pixel sees nothing."""
        o, e, t = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        if not self.L.pth_pick(self.h, int(x), int(y), C.byref(o), C.byref(e), C.byref(t)):
            raise _ptk.PtkError("Pick failed: " + self.LastError())
        return o.value, e.value, t.value

    def GetCamera(self):
        """Extension: (pos, dir, up) as SetCamera last received them (not normalised), float32 [3] each."""
        p, d, u = (np.zeros(3, np.float32) for _ in range(3))
        self.L.pth_get_camera(self.h, _fp(p), _fp(d), _fp(u))
        return p, d, u

    def TraceRays(self, origins, dirs, first_sample: int, spp: int, key_base: int = 0, out=None, lens_draws: bool = False) -> np.ndarray:
        """Extension: radiance along caller-supplied rays (include/ptk.h ptk_trace_rays) at this tracer's seed and trace depth;
        [n, 3] float32 numpy arrays in, the float32 in-order sums over samples [first_sample, first_sample + spp) out.  Valid
        after BuildBVH(); pending material / geometry edits apply as for RenderFrame().  out: sums of earlier samples to add to."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        assert len(d) == len(o), "as many directions as origins"
        flags = (_ptk.RAYS_ACCUMULATE if out is not None else 0) | (_ptk.RAYS_LENS_DRAWS if lens_draws else 0)
        if out is None:
            out = np.empty((len(o), 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == o.size
        ptr = (lambda a: a.ctypes.data if len(o) else None)
        if not self.L.pth_trace_rays(self.h, len(o), ptr(o), ptr(d), int(first_sample), int(spp), int(key_base) & 0xffffffff, flags, ptr(out)):
            raise _ptk.PtkError("TraceRays failed: " + self.LastError())
        return out

    def IntersectRays(self, origins, dirs, sample: int = 0, key_base: int = 0):
        """Extension: closest hits along caller-supplied rays (include/ptk.h ptk_intersect_rays) at this tracer's seed; [n, 3]
        float32 numpy arrays in, (tri [n] int32, t [n] float32, bary [n, 2] float32, material [n] int32) out, -1 / inf / 0 / -1 on
        a miss.  Valid after BuildBVH(); pending material / geometry edits apply as for RenderFrame()."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n, "as many directions as origins"
        out = (np.empty(n, np.int32), np.empty(n, np.float32), np.empty((n, 2), np.float32), np.empty(n, np.int32))
        if n and not self.L.pth_intersect_rays(self.h, n, o.ctypes.data, d.ctypes.data, int(sample), int(key_base) & 0xffffffff,
                                         *(a.ctypes.data for a in out)):
            raise _ptk.PtkError("IntersectRays failed: " + self.LastError())
        return out

    def OccludedRays(self, origins, dirs, tmax=None, sample: int = 0, key_base: int = 0) -> np.ndarray:
        """Extension: occlusion along caller-supplied rays (include/ptk.h ptk_occluded_rays) at this tracer's seed: [n] uint8, 1
        where an accepted triangle lies at t < tmax[i] (None: no bound)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n, "as many directions as origins"
        tm = None if tmax is None else np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
        assert tm is None or len(tm) == n, "one tmax per ray"
        out = np.empty(n, np.uint8)
        if n and not self.L.pth_occluded_rays(self.h, n, o.ctypes.data, d.ctypes.data, tm.ctypes.data if tm is not None else None, int(sample),
                                        int(key_base) & 0xffffffff, out.ctypes.data):
            raise _ptk.PtkError("OccludedRays failed: " + self.LastError())
        return out

    def closest_points(self, points, max_dist=None):
        """Extension: the nearest surface point to each of the points [n, 3] (include/ptk.h ptk_closest_points), strictly nearer
        than max_dist[i] where max_dist is given; (tri [n] int32, dist [n] float32, point [n, 3] float32, bary [n, 2] float32),
        misses -1 / inf / 0 / 0.  Pending geometry edits apply as for RenderFrame()."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        md = None if max_dist is None else np.ascontiguousarray(max_dist, dtype=np.float32).reshape(-1)
        assert md is None or len(md) == n, "one max_dist per point"
        out = (np.empty(n, np.int32), np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 2), np.float32))
        if n and not self.L.pth_closest_points(self.h, n, p.ctypes.data, md.ctypes.data if md is not None else None,
                                               *(a.ctypes.data for a in out)):
            raise _ptk.PtkError("ClosestPoints failed: " + self.LastError())
        return out

    ClosestPoints = closest_points

    def _overlap(self, fn, who, a, b, width_b, k, tri_from):
        """the host entry fn over queries a [n, 3], b [n, width_b]: (count [n], tris [n, k])"""
        K = int(k)
        if K < 0 or K > _ptk.OVERLAP_MAX_K:
            raise _ptk.PtkError(f"{who}: k must be in 0 .. {_ptk.OVERLAP_MAX_K}")
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        n = len(a)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        assert len(b) == n * width_b, "one box corner or radius per query"
        tf = None if tri_from is None else np.ascontiguousarray(tri_from, dtype=np.int32).reshape(-1)
        assert tf is None or len(tf) == n, "one tri_from per query"
        out = (np.empty(n, np.int32), np.empty((n, K), np.int32))
        if n and not fn(self.h, n, a.ctypes.data, b.ctypes.data, tf.ctypes.data if tf is not None else None, K, out[0].ctypes.data,
                        out[1].ctypes.data if K else None):
            raise _ptk.PtkError(who + " failed: " + self.LastError())
        return out

    def overlap_boxes(self, lo, hi, k: int = 0, tri_from=None):
        """Extension: (count [n] int32, tris [n, k] int32) - how many triangles of index >= tri_from[i] (None: 0) meet the closed
        box [lo[i], hi[i]], and the k (0 .. 16) smallest of their indices, -1 behind the last (include/ptk.h ptk_overlap_boxes).
        Pending geometry edits apply as for RenderFrame()."""
        return self._overlap(self.L.pth_overlap_boxes, "OverlapBoxes", lo, hi, 3, k, tri_from)

    def overlap_spheres(self, centers, radius, k: int = 0, tri_from=None):
        """Extension: overlap_boxes' answer for the spheres (centers[i], radius[i]): the triangles strictly nearer to the centre
        than the radius under closest_points' rule (include/ptk.h ptk_overlap_spheres)."""
        return self._overlap(self.L.pth_overlap_spheres, "OverlapSpheres", centers, radius, 1, k, tri_from)

    OverlapBoxes = overlap_boxes
    OverlapSpheres = overlap_spheres

    def crossings_rays(self, origins, dirs, tmax=None):
        """Extension: (front [n] int32, back [n] int32), how many triangles each ray crosses before tmax[i] (None: no bound) from
        their front and from their back (include/ptk.h ptk_crossings_rays).  Pending geometry edits apply as for RenderFrame()."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n, "as many directions as origins"
        tm = None if tmax is None else np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
        assert tm is None or len(tm) == n, "one tmax per ray"
        out = (np.empty(n, np.int32), np.empty(n, np.int32))
        if n and not self.L.pth_crossings_rays(self.h, n, o.ctypes.data, d.ctypes.data, tm.ctypes.data if tm is not None else None,
                                               *(a.ctypes.data for a in out)):
            raise _ptk.PtkError("CrossingsRays failed: " + self.LastError())
        return out

    @staticmethod
    def _inside_dirs(dirs):
        d = None if dirs is None else np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        return d, (3 if d is None else len(d)), (None if d is None else d.ctypes.data)

    def contains_points(self, points, dirs=None, mode=_ptk.INSIDE_WINDING, want_winding: bool = False):
        """Extension: inside [n] uint8 - the majority vote of the rays from each point along dirs [D, 3] (None: the built-in three)
        under mode "winding" or "parity" (include/ptk.h ptk_contains_points); with want_winding (inside, winding [n, D] int32).
        Pending geometry edits apply as for RenderFrame()."""
        m = _ptk.inside_mode(mode)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        d, D, dptr = self._inside_dirs(dirs)
        inside = np.empty(n, np.uint8)
        winding = np.empty((n, D), np.int32) if want_winding else None
        if n and not self.L.pth_contains_points(self.h, n, p.ctypes.data, D, dptr, m, inside.ctypes.data,
                                                winding.ctypes.data if want_winding else None):
            raise _ptk.PtkError("ContainsPoints failed: " + self.LastError())
        return (inside, winding) if want_winding else inside

    def signed_distance(self, points, max_dist=None, dirs=None, mode=_ptk.INSIDE_WINDING):
        """Extension: closest_points(points, max_dist) with the sign bit of dist set where contains_points(points, dirs, mode) says
        inside (include/ptk.h ptk_signed_distance).  Pending geometry edits apply as for RenderFrame()."""
        m = _ptk.inside_mode(mode)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        md = None if max_dist is None else np.ascontiguousarray(max_dist, dtype=np.float32).reshape(-1)
        assert md is None or len(md) == n, "one max_dist per point"
        d, D, dptr = self._inside_dirs(dirs)
        out = (np.empty(n, np.int32), np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 2), np.float32))
        if n and not self.L.pth_signed_distance(self.h, n, p.ctypes.data, md.ctypes.data if md is not None else None, D, dptr, m,
                                                *(a.ctypes.data for a in out)):
            raise _ptk.PtkError("SignedDistance failed: " + self.LastError())
        return out

    CrossingsRays, ContainsPoints, SignedDistance = crossings_rays, contains_points, signed_distance

    def multihit_rays(self, origins, dirs, max_hits, tmax=None):
        """Extension: (count [n] int32, tri [n, K] int32, t [n, K] float32, bary [n, K, 2] float32, side [n, K] int8), the first
        K = max_hits (1 .. 16) triangles each ray crosses before tmax[i] (None: no bound), ascending by (t, triangle index)
        (include/ptk.h ptk_multihit_rays).  Pending geometry edits apply as for RenderFrame()."""
        K = int(max_hits)
        if K < 1 or K > _ptk.MULTIHIT_MAX:
            raise _ptk.PtkError(f"MultiHitRays: max_hits must be in 1 .. {_ptk.MULTIHIT_MAX}")
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n, "as many directions as origins"
        tm = None if tmax is None else np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
        assert tm is None or len(tm) == n, "one tmax per ray"
        out = (np.empty(n, np.int32), np.empty((n, K), np.int32), np.empty((n, K), np.float32), np.empty((n, K, 2), np.float32),
               np.empty((n, K), np.int8))
        if n and not self.L.pth_multihit_rays(self.h, n, o.ctypes.data, d.ctypes.data, tm.ctypes.data if tm is not None else None, K,
                                              *(a.ctypes.data for a in out)):
            raise _ptk.PtkError("MultiHitRays failed: " + self.LastError())
        return out

    MultiHitRays = multihit_rays

    def nearest_triangles(self, points, k, max_dist=None):
        """Extension: (count [n] int32, tri [n, K] int32, dist [n, K] float32, point [n, K, 3] float32, bary [n, K, 2] float32), the
        K = k (1 .. 16) triangles nearest to each point, strictly nearer than max_dist[i] where max_dist is given, ascending by
        (distance, triangle index) (include/ptk.h ptk_nearest_triangles); behind count -1 / inf / 0 / 0.  Pending geometry edits
        apply as for RenderFrame()."""
        K = int(k)
        if K < 1 or K > _ptk.NEAREST_MAX_K:
            raise _ptk.PtkError(f"NearestTriangles: k must be in 1 .. {_ptk.NEAREST_MAX_K}")
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        md = None if max_dist is None else np.ascontiguousarray(max_dist, dtype=np.float32).reshape(-1)
        assert md is None or len(md) == n, "one max_dist per point"
        out = (np.empty(n, np.int32), np.empty((n, K), np.int32), np.empty((n, K), np.float32), np.empty((n, K, 3), np.float32),
               np.empty((n, K, 2), np.float32))
        if n and not self.L.pth_nearest_triangles(self.h, n, p.ctypes.data, md.ctypes.data if md is not None else None, K,
                                                  *(a.ctypes.data for a in out)):
            raise _ptk.PtkError("NearestTriangles failed: " + self.LastError())
        return out

    NearestTriangles = nearest_triangles

    def sample_surface(self, n, key_base=0, sample=0):
        """Extension: (tri [n] int32, bary [n, 2], position [n, 3], normal [n, 3] float32, material [n] int32) - n points of the
        scene's surface at this tracer's seed, a triangle drawn in proportion to its area times its weight, the point uniform on it
        (include/ptk.h ptk_sample_surface).  Pending geometry edits apply as for RenderFrame()."""
        n = int(n)
        out = (np.empty(n, np.int32), np.empty((n, 2), np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32),
               np.empty(n, np.int32))
        if not self.L.pth_sample_surface(self.h, n, int(key_base) & 0xffffffff, int(sample) & 0xffffffff, *(a.ctypes.data for a in out)):
            raise _ptk.PtkError("SampleSurface failed: " + self.LastError())
        return out

    def set_surface_weights(self, weights=None):
        """Extension: per-triangle weights [triangles] float32, finite and >= 0, multiplied onto the areas sample_surface draws by;
        None: the areas alone (include/ptk.h ptk_surface_weights).  BuildBVH() drops them."""
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        assert w is None or len(w) == self.GetTriangleCount(), "one weight per triangle"
        if not self.L.pth_set_surface_weights(self.h, w.ctypes.data if w is not None else None):
            raise _ptk.PtkError("SetSurfaceWeights failed: " + self.LastError())

    def surface_info(self):
        """Extension: (total, exponent E, drawable triangles, largest weight) of the sampling table in force (ptk_surface_info)"""
        total, e, dr, m = C.c_uint64(0), C.c_int32(0), C.c_int32(0), C.c_float(0)
        if not self.L.pth_surface_info(self.h, C.byref(total), C.byref(e), C.byref(dr), C.byref(m)):
            raise _ptk.PtkError("SurfaceInfo failed: " + self.LastError())
        return total.value, e.value, dr.value, np.float32(m.value)

    SampleSurface, SetSurfaceWeights, SurfaceInfo = sample_surface, set_surface_weights, surface_info

    def surface_attributes(self, tri, bary, dirs=None, want=_ptk.ATTR_ALL):
        """Extension: dict name (ptk.ATTR_NAMES) -> array of what is at the surface points (tri[i], bary[i] = u, v): material, uv,
        position, normal_geom, normal (flipped against dirs[i] where dirs is given), albedo, emission, gloss, opacity
        (include/ptk.h ptk_surface_attributes).  want: bit k = attribute k.  A triangle index outside the scene gives material -1
        and zeros.  Pending material and geometry edits apply as for RenderFrame()."""
        want = int(want) & _ptk.ATTR_ALL
        if not want:
            raise _ptk.PtkError("SurfaceAttributes: no output array")
        t = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1)
        n = len(t)
        b = np.ascontiguousarray(bary, dtype=np.float32).reshape(-1, 2)
        assert len(b) == n, "one (u, v) per triangle index"
        d = None if dirs is None else np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        assert d is None or len(d) == n, "one direction per query"
        out = {nm: _ptk.attribute_array(k, n) for k, nm in enumerate(_ptk.ATTR_NAMES) if want >> k & 1}
        ptrs = [out[nm].ctypes.data if nm in out else None for nm in _ptk.ATTR_NAMES]
        if n and not self.L.pth_surface_attributes(self.h, n, t.ctypes.data, b.ctypes.data, d.ctypes.data if d is not None else None, *ptrs):
            raise _ptk.PtkError("SurfaceAttributes failed: " + self.LastError())
        return out

    SurfaceAttributes = surface_attributes

    def _chart_uvs(self, uvs):
        if uvs is None:
            return None, None
        u = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6)
        assert len(u) == self.GetTriangleCount(), "one chart (6 floats) per triangle"
        return u, u.ctypes.data

    def BakeLightmap(self, width: int, height: int, offset: float, first_sample: int, spp: int, uvs=None, key_base: int = 0, out=None,
                     back: bool = False):
        """Extension: bake a width x height lightmap (include/ptk.h ptk_bake_lightmap) at this tracer's seed and trace depth.
        uvs: [triangles, 6] chart corners (lightmap.grid_atlas), None for the scene's own.  Returns (sums [H, W, 3] float32, rows
        bottom-up; owner [H, W] int32, -1 uncovered).  out: sums of earlier samples to add to (PTK_BAKE_ACCUMULATE)."""
        u, up = self._chart_uvs(uvs)
        flags = (_ptk.BAKE_ACCUMULATE if out is not None else 0) | (_ptk.BAKE_BACK if back else 0)
        if out is None:
            out = np.empty((height, width, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == width * height * 3
        owner = np.empty((height, width), np.int32)
        if not self.L.pth_bake_lightmap(self.h, int(width), int(height), up, float(offset), int(first_sample), int(spp),
                                        int(key_base) & 0xffffffff, flags, out.ctypes.data, owner.ctypes.data):
            raise _ptk.PtkError("BakeLightmap failed: " + self.LastError())
        return out, owner

    def TraceRaysAdaptive(self, origins, dirs, threshold: float, min_spp: int, step: int, max_spp: int, key_base: int = 0,
                          lens_draws: bool = False):
        """Extension: adaptive ray query (include/ptk.h ptk_trace_rays_adaptive) at this tracer's seed and trace depth.  Returns
        (sum [n, 3] float32, sumsq [n, 3] float32, counts [n] uint32, result dict); the mean is sum / counts."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        assert len(d) == len(o), "as many directions as origins"
        s1 = np.empty((len(o), 3), np.float32); s2 = np.empty((len(o), 3), np.float32); counts = np.empty((len(o),), np.uint32)
        r = _ptk.RaysAdaptiveResult()
        ptr = (lambda a: a.ctypes.data if len(o) else None)
        if not self.L.pth_trace_rays_adaptive(self.h, len(o), ptr(o), ptr(d), float(threshold), int(min_spp), int(step), int(max_spp),
                                              int(key_base) & 0xffffffff, _ptk.RAYS_LENS_DRAWS if lens_draws else 0, ptr(s1), ptr(s2),
                                              ptr(counts), C.byref(r)):
            raise _ptk.PtkError("TraceRaysAdaptive failed: " + self.LastError())
        return s1, s2, counts, r.as_dict()

    def BakeLightmapAdaptive(self, width: int, height: int, offset: float, threshold: float, min_spp: int, step: int, max_spp: int,
                             uvs=None, key_base: int = 0, back: bool = False):
        """Extension: adaptive lightmap bake (include/ptk.h ptk_bake_lightmap_adaptive) at this tracer's seed and trace depth.
        Returns (sums [H, W, 3] float32, counts [H, W] uint32, owner [H, W] int32, result dict), rows bottom-up."""
        u, up = self._chart_uvs(uvs)
        out = np.empty((height, width, 3), np.float32)
        counts = np.empty((height, width), np.uint32)
        owner = np.empty((height, width), np.int32)
        r = _ptk.RaysAdaptiveResult()
        if not self.L.pth_bake_lightmap_adaptive(self.h, int(width), int(height), up, float(offset), float(threshold), int(min_spp),
                                                 int(step), int(max_spp), int(key_base) & 0xffffffff, _ptk.BAKE_BACK if back else 0,
                                                 out.ctypes.data, counts.ctypes.data, owner.ctypes.data, C.byref(r)):
            raise _ptk.PtkError("BakeLightmapAdaptive failed: " + self.LastError())
        return out, counts, owner, r.as_dict()

    def BakeCoverage(self, width: int, height: int, uvs=None):
        """Extension: (owner [H, W] int32, bary [H, W, 2], pos [H, W, 3]) of a lightmap's texels (ptk_bake_coverage); no tracing."""
        u, up = self._chart_uvs(uvs)
        owner = np.empty((height, width), np.int32)
        bary = np.empty((height, width, 2), np.float32); pos = np.empty((height, width, 3), np.float32)
        if not self.L.pth_bake_coverage(self.h, int(width), int(height), up, owner.ctypes.data, bary.ctypes.data, pos.ctypes.data):
            raise _ptk.PtkError("BakeCoverage failed: " + self.LastError())
        return owner, bary, pos

    def DilateLightmap(self, image: np.ndarray, owner: np.ndarray, passes: int):
        """Extension: chart padding in place (ptk_lightmap_dilate); returns (image, owner)."""
        h, w = owner.shape
        assert image.dtype == np.float32 and image.flags.c_contiguous and image.size == w * h * 3
        assert owner.dtype == np.int32 and owner.flags.c_contiguous
        if not self.L.pth_lightmap_dilate(self.h, w, h, int(passes), image.ctypes.data, owner.ctypes.data):
            raise _ptk.PtkError("DilateLightmap failed: " + self.LastError())
        return image, owner

    def BakeProbes(self, positions, dirs, first_sample: int, spp: int, weight: float, key_base: int = 0, radiance=None):
        """Extension: bake irradiance probes (include/ptk.h ptk_bake_probes) at this tracer's seed and trace depth.  positions
        [P, 3], dirs [D, 3] (probes.grid_positions, probes.fibonacci_dirs); returns (radiance [P, D, 3], coefs [P, 9, 3]) float32.
        radiance: the table of earlier samples' sums, added to in place (PTK_PROBES_ACCUMULATE)."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        flags = _ptk.PROBES_ACCUMULATE if radiance is not None else 0
        if radiance is None:
            radiance = np.empty((len(pos), len(d), 3), np.float32)
        assert radiance.dtype == np.float32 and radiance.flags.c_contiguous and radiance.size == len(pos) * len(d) * 3
        coefs = np.empty((len(pos), 9, 3), np.float32)
        ptr = (lambda a: a.ctypes.data if a.size else None)
        if not self.L.pth_bake_probes(self.h, len(pos), ptr(pos), len(d), ptr(d), int(first_sample), int(spp), int(key_base) & 0xffffffff,
                                      flags, float(weight), ptr(radiance), ptr(coefs)):
            raise _ptk.PtkError("BakeProbes failed: " + self.LastError())
        return radiance, coefs

    def SampleProbes(self, dims, origin, spacing, coefs, points, normals) -> np.ndarray:
        """Extension: [n, 3] float32 irradiance at (points, normals) from a probe grid (ptk_probes_irradiance); coefs
        [nz, ny, nx, 9, 3] as BakeProbes gave them for probes.grid_positions(dims, origin, spacing)."""
        g_dims = (C.c_int32 * 3)(*(int(n) for n in dims))
        g_origin = (C.c_float * 3)(*(float(x) for x in origin))
        g_spacing = (C.c_float * 3)(*(float(x) for x in spacing))
        c = np.ascontiguousarray(coefs, dtype=np.float32)
        q = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        assert c.size == int(g_dims[0]) * int(g_dims[1]) * int(g_dims[2]) * 27 and len(nrm) == len(q)
        out = np.empty((len(q), 3), np.float32)
        ptr = (lambda a: a.ctypes.data if a.size else None)
        if not self.L.pth_sample_probes(self.h, g_dims, g_origin, g_spacing, ptr(c), len(q), ptr(q), ptr(nrm), ptr(out)):
            raise _ptk.PtkError("SampleProbes failed: " + self.LastError())
        return out

    def BakeProbeVisibility(self, positions, dirs, res: int, max_dist: float, sample: int = 0, key_base: int = 0):
        """Extension: probe visibility (include/ptk.h ptk_bake_probe_visibility) at this tracer's seed.  positions [P, 3], dirs
        [D, 3]; returns (depth [P, D], moments [P, res * res, 2]) float32."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        depth = np.empty((len(pos), len(d)), np.float32)
        moments = np.empty((len(pos), int(res) * int(res) if 1 <= int(res) <= 16 else 1, 2), np.float32)
        ptr = (lambda a: a.ctypes.data if a.size else None)
        if not self.L.pth_bake_probe_visibility(self.h, len(pos), ptr(pos), len(d), ptr(d), int(res), float(max_dist), int(sample),
                                                int(key_base) & 0xffffffff, ptr(depth), ptr(moments)):
            raise _ptk.PtkError("BakeProbeVisibility failed: " + self.LastError())
        return depth, moments

    def SampleProbesVisible(self, dims, origin, spacing, coefs, res: int, moments, points, normals, normal_bias: float = 0.0) -> np.ndarray:
        """Extension: SampleProbes with the probes weighted by their visibility (ptk_probes_irradiance_visible); moments
        [nz, ny, nx, res * res, 2] as BakeProbeVisibility gave them for probes.grid_positions(dims, origin, spacing)."""
        g_dims = (C.c_int32 * 3)(*(int(n) for n in dims))
        g_origin = (C.c_float * 3)(*(float(x) for x in origin))
        g_spacing = (C.c_float * 3)(*(float(x) for x in spacing))
        c = np.ascontiguousarray(coefs, dtype=np.float32)
        mo = np.ascontiguousarray(moments, dtype=np.float32)
        q = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        probes = int(g_dims[0]) * int(g_dims[1]) * int(g_dims[2])
        assert c.size == probes * 27 and mo.size == probes * int(res) * int(res) * 2 and len(nrm) == len(q)
        out = np.empty((len(q), 3), np.float32)
        ptr = (lambda a: a.ctypes.data if a.size else None)
        if not self.L.pth_sample_probes_visible(self.h, g_dims, g_origin, g_spacing, ptr(c), int(res), ptr(mo), float(normal_bias), len(q),
                                                ptr(q), ptr(nrm), ptr(out)):
            raise _ptk.PtkError("SampleProbesVisible failed: " + self.LastError())
        return out

    def ReadAccumulation(self) -> np.ndarray:
        w, h = self.GetResolution()
        out = np.empty((h, w, 3), np.float32)
        if not self.L.pth_read_accum(self.h, out.ctypes.data):
            raise _ptk.PtkError("ReadAccumulation failed: " + self.LastError())
        return out

    def LastError(self) -> str: return self.L.pth_last_error(self.h).decode()

    def LoadSceneFile(self, pts_path: str):
        """.pts -> LoadObject/SetMaterial/Set*Texture/BuildBVH/SetCamera/... (main.cpp:261-438,
        previewer.cpp:770-817, :924-930)."""
        if self.L.pth_load_scene_file(self.h, pts_path.encode()) != 0:
            raise _ptk.PtkError(self.LastError())

    def context(self) -> "_ptk.Context":
        """Borrowed view of this tracer's ptk context (for stats / timing / device pointers)."""
        c = _ptk.Context.__new__(_ptk.Context)
        c.L = self.L
        c.h = C.c_void_p(self.L.pth_context(self.h))
        if not c.h:
            raise _ptk.PtkError("no HIP device: " + self.LastError())
        c.width, c.height = self.GetResolution()
        c.guide_width, c.guide_height = getattr(self, "_guide_size", (0, 0))
        c._keep = self
        c.close = lambda: None
        return c

    def StagedScene(self) -> dict:
        """The staged scene as numpy arrays in the boundary layout (host only, no GPU needed)."""
        d = self.L.pth_staged_scene(self.h).contents
        n = d.num_triangles

        def arr(ptr, count, dtype):
            if not ptr or count == 0:
                return np.zeros(0, dtype)
            nbytes = count * np.dtype(dtype).itemsize
            buf = (C.c_char * nbytes).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype, count=count).copy()

        return {
            "verts": arr(d.verts, n * 9, np.float32).reshape(n, 9),
            "normals": arr(d.normals, n * 9, np.float32).reshape(n, 9),
            "uvs": arr(d.uvs, n * 6, np.float32).reshape(n, 6),
            "tbn": arr(d.tbn, n * 9, np.float32).reshape(n, 9),
            "smoothing": arr(d.smoothing, n, np.uint8),
            "material": arr(d.material, n, np.int32),
            "materials": arr(d.materials, d.num_materials, _ptk.MATERIAL_DTYPE),
            "textures": arr(d.textures, d.num_textures, _ptk.TEXTURE_DTYPE),
            "texels": arr(d.texels, d.texel_bytes, np.uint8),
            "lights": arr(d.lights, d.num_lights, np.int32),
        }


# ---- host-only helpers (no GPU) ---------------------------------------------------------------------

def trs_matrix(loc, rot_deg, scl) -> np.ndarray:
    out = np.zeros(16, np.float32)
    lib().pth_trs_matrix(_fp(_f3(loc)), _fp(_f3(rot_deg)), _fp(_f3(scl)), _fp(out))
    return out.reshape(4, 4)       # [column][row], glm layout


def euler_camera(rot_deg):
    out = np.zeros(6, np.float32)
    lib().pth_euler_camera(_fp(_f3(rot_deg)), _fp(out))
    return out[:3].copy(), out[3:].copy()


def triangle_init(in15) -> np.ndarray:
    i = np.ascontiguousarray(in15, np.float32); out = np.zeros(9, np.float32)
    lib().pth_triangle_init(_fp(i), _fp(out))
    return out


def image_load(path: str):
    w = C.c_int(); h = C.c_int()
    ok = lib().pth_image_load(path.encode(), C.byref(w), C.byref(h))
    if not ok:
        return None
    data = np.zeros((h.value, w.value, 4), np.uint8)
    lib().pth_image_data(data.ctypes.data)
    return data


def image_tex2d(u: float, v: float) -> np.ndarray:
    out = np.zeros(4, np.float32)
    lib().pth_image_tex2d(u, v, _fp(out))
    return out


def export_png(path: str, rgb8_bottom_up: np.ndarray) -> bool:
    """ExportAt (main.cpp:760-771): the bottom-up RGB8 buffer as a top-down PNG."""
    a = np.ascontiguousarray(rgb8_bottom_up, np.uint8)
    h, w, c = a.shape
    assert c == 3
    return bool(lib().pth_export_png(path.encode(), a.ctypes.data, w, h))


def camera_from_scene(scene):
    """(pos, dir, up, focal, fovy, focal_dist, aperture) of a scenes.SceneDesc, the way
    Previewer::SetPathTracerCamera derives them (previewer.cpp:924-930)."""
    from . import scenes as S
    d, u = euler_camera(scene.cam_rot)
    return dict(pos=np.array(scene.cam_pos, np.float32), dir=d, up=u, focal=S.PTS_FOCAL, fovy=S.PTS_FOVY,
                focal_dist=float(scene.focal_dist), aperture=float(np.float32(S.PTS_FOCAL) / np.float32(scene.camera_f)))

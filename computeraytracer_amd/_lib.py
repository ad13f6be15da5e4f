"""ctypes binding of libcrt.so (the C ABI declared in include/crt.h).

There is no fallback of any kind: if the shared library is missing or a HIP
device is not available, loading / crt_create raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CRT_LIB") or os.path.join(_HERE, "libcrt.so")   # CRT_LIB: tuning builds only

NCOUNTERS = 8
ACCEL_NONE, ACCEL_BVH2, ACCEL_LBVH, ACCEL_PLOC = 0, 1, 2, 3
QUERY_CLOSEST, QUERY_ANY = 0, 1
CNT = dict(rays=0, nodes=1, prims=2, paths=3, bounces=4, shadow=5, hits=6, walked=7)

# name -> (restype, argtypes); kept in one place so tests can check that every
# symbol include/crt.h declares is exported.
_P = C.c_void_p
SIGNATURES = {
    "crt_create": (C.c_int, [C.POINTER(_P), C.c_int]),
    "crt_destroy": (None, [_P]),
    "crt_last_error": (C.c_char_p, [_P]),
    "crt_abi_version": (C.c_int, []),
    "crt_upload_scene": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t, _P, _P]),
    "crt_set_tile": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "crt_set_row_bands": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "crt_build_accel": (C.c_int, [_P, C.c_int]),
    "crt_reset": (C.c_int, [_P]),
    "crt_trace": (C.c_int, [_P, C.c_uint32]),
    "crt_sync": (C.c_int, [_P]),
    "crt_sample_count": (C.c_int, [_P, _P]),
    "crt_tile": (C.c_int, [_P, _P]),
    "crt_read_accum": (C.c_int, [_P, _P]),
    "crt_read_rgba8": (C.c_int, [_P, _P]),
    "crt_write_accum": (C.c_int, [_P, _P, C.c_uint32]),
    "crt_read_latest_rgba8": (C.c_int, [_P, _P, _P]),
    "crt_latest_sample": (C.c_int, [_P, _P]),
    "crt_pin_host": (C.c_int, [_P, C.c_size_t]),
    "crt_unpin_host": (C.c_int, [_P]),
    "crt_read_sample_rgba8": (C.c_int, [_P, C.c_uint32, _P]),
    "crt_device_buffers": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "crt_bind_output": (C.c_int, [_P, _P, _P]),
    "crt_set_stream": (C.c_int, [_P, _P]),
    "crt_enable_counters": (C.c_int, [_P, C.c_int]),
    "crt_counters": (C.c_int, [_P, _P]),
    "crt_reset_counters": (C.c_int, [_P]),
    "crt_last_trace_ms": (C.c_int, [_P, _P, _P]),
    "crt_last_kernel_ms": (C.c_int, [_P, _P, _P]),
    "crt_set_option": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "crt_accel_stats": (C.c_int, [_P, _P]),
    "crt_get_device": (C.c_int, [_P, _P]),
    "crt_get_stream": (C.c_int, [_P, C.POINTER(_P)]),
    "crt_image_size": (C.c_int, [_P, _P]),
    "crt_comm_unique_id": (C.c_int, [_P, C.c_int]),
    "crt_comm_init": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "crt_comm_partition": (C.c_int, [_P, C.c_uint32]),
    "crt_gather": (C.c_int, [_P, C.c_int]),
    "crt_read_frame_rgba8": (C.c_int, [_P, _P]),
    "crt_read_frame_accum": (C.c_int, [_P, _P]),
    "crt_frame_device_buffers": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "crt_comm_info": (C.c_int, [_P, _P]),
    "crt_comm_destroy": (C.c_int, [_P]),
    "crt_layout_rows": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P]),
    "crt_denoise": (C.c_int, [_P, _P, _P, _P]),
    "crt_denoise_latest": (C.c_int, [_P, _P, _P, _P, _P]),
    "crt_read_gbuffer": (C.c_int, [_P, _P]),
    "crt_read_motion": (C.c_int, [_P, _P]),
    "crt_render_aovs": (C.c_int, [_P, C.c_uint32, _P]),
    "crt_spectrum_rgb": (C.c_int, [_P, _P, _P]),
    "crt_read_albedo_table": (C.c_int, [_P, _P]),
    "crt_render_mattes": (C.c_int, [_P, C.c_uint32, C.c_int, C.c_uint32, _P]),
    "crt_set_primitive_ids": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "crt_read_primitive_ids": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "crt_query_rays": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "crt_query_rays_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P]),
    "crt_pick": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "crt_radiance_rays": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint32, _P]),
    "crt_radiance_rays_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_uint32, _P, _P]),
    "crt_debug_radiance_lanes": (C.c_int, [_P, C.c_size_t, _P]),
    "crt_debug_intersect": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "crt_debug_trace_rays": (C.c_int, [_P, _P, C.c_size_t, _P, _P]),
    "crt_debug_walk_rays": (C.c_int, [_P, C.c_int, _P, C.c_size_t, _P, _P]),
    "crt_debug_read_accel": (C.c_int, [_P, C.c_int, _P, C.c_size_t, _P]),
    "crt_debug_probes": (C.c_int, [_P, _P]),
    "crt_debug_gen_culled": (C.c_int, [_P, _P]),
    "crt_debug_deferred_nee": (C.c_int, [_P, _P]),
    "crt_debug_tile_classes": (C.c_int, [_P, _P, C.c_size_t]),
    "crt_debug_tile_classes_host": (C.c_int, [_P, _P, C.c_size_t]),
    "crt_debug_tile_class_setups": (C.c_int, [_P, _P]),
    "crt_debug_mapped_gen_launches": (C.c_int, [_P, _P]),
    "crt_debug_math": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_size_t]),
    "crt_set_camera": (C.c_int, [_P, _P]),
    "crt_update_primitives": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "crt_transform_primitives": (C.c_int, [_P, _P, C.c_uint32]),
    "crt_remove_primitives": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_size_t]),
    "crt_append_primitives": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_size_t]),
    "crt_read_primitives": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "crt_update_lights": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "crt_refit_accel": (C.c_int, [_P, _P]),
    "crt_accel_quality": (C.c_int, [_P, _P]),
    "crt_debug_hit_pad": (C.c_int, [_P, _P]),
    "crt_trace_adaptive": (C.c_int, [_P, _P, _P]),
    "crt_read_adaptive": (C.c_int, [_P, _P, _P]),
    "crt_adaptive_defaults": (C.c_int, [_P]),
    "crt_trace_adaptive_filtered": (C.c_int, [_P, _P, _P, _P]),
    "crt_read_adaptive_filtered": (C.c_int, [_P, _P, _P, _P]),
    "crt_denoise_adaptive": (C.c_int, [_P, _P, _P, _P, _P]),
    "crt_denoise_adaptive_defaults": (C.c_int, [_P]),
    "crt_read_frame_adaptive": (C.c_int, [_P, _P, _P]),
    "crt_denoise_frame": (C.c_int, [_P, _P, _P, _P]),
    "crt_denoise_adaptive_frame": (C.c_int, [_P, _P, _P, _P, _P]),
    "crt_set_sample_offset": (C.c_int, [_P, C.c_uint32]),
    "crt_sample_offset": (C.c_int, [_P, _P]),
    "crt_denoise_temporal": (C.c_int, [_P, _P, _P, _P, _P]),
    "crt_denoise_temporal_defaults": (C.c_int, [_P]),
    "crt_denoise_temporal_reset": (C.c_int, [_P]),
    "crt_denoise_svgf": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "crt_denoise_svgf_defaults": (C.c_int, [_P]),
    "crt_debug_read_moments": (C.c_int, [_P, _P]),
    "crt_debug_read_clip_box": (C.c_int, [_P, _P]),
}


class AdaptiveParams(C.Structure):
    """crt_adaptive_params of include/crt.h."""
    _fields_ = [("samples", C.c_uint32), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("threshold", C.c_float)]


def adaptive_defaults() -> AdaptiveParams:
    """The library's defaults for crt_trace_adaptive (crt_adaptive_defaults)."""
    p = AdaptiveParams()
    if load().crt_adaptive_defaults(C.byref(p)) != 0:
        raise RuntimeError("crt_adaptive_defaults failed")
    return p


class PrimTransform(C.Structure):
    """crt_prim_transform of include/crt.h (60 bytes; scene.TRANSFORM_DTYPE is the numpy form)."""
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("m", C.c_float * 12), ("radius_scale", C.c_float)]


class DenoiseParams(C.Structure):
    """crt_denoise_params of include/crt.h."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float)]


class AovPlanes(C.Structure):
    """crt_aov_planes of include/crt.h."""
    _fields_ = [("hits", C.c_void_p), ("alpha", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p)]


class MattePlanes(C.Structure):
    """crt_matte_planes of include/crt.h."""
    _fields_ = [("ids", C.c_void_p), ("counts", C.c_void_p), ("hits", C.c_void_p), ("overflow", C.c_void_p)]


class Ray(C.Structure):
    """crt_ray of include/crt.h (32 bytes; renderer.RAY_DTYPE is the numpy form)."""
    _fields_ = [("o", C.c_float * 3), ("t_max", C.c_float), ("d", C.c_float * 3), ("exclude", C.c_uint32)]


class QueryPlanes(C.Structure):
    """crt_query_planes of include/crt.h."""
    _fields_ = [("hit", C.c_void_p), ("prim", C.c_void_p), ("id", C.c_void_p), ("t", C.c_void_p), ("position", C.c_void_p),
                ("normal", C.c_void_p), ("uv", C.c_void_p)]


class PathKey(C.Structure):
    """crt_path_key of include/crt.h (16 bytes; renderer.PATH_KEY_DTYPE is the numpy form)."""
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("first_sample", C.c_uint32), ("reserved", C.c_uint32)]


class RadiancePlanes(C.Structure):
    """crt_radiance_planes of include/crt.h."""
    _fields_ = [("xyz", C.c_void_p), ("y2", C.c_void_p), ("rgba8", C.c_void_p)]


class DenoiseAdaptiveParams(C.Structure):
    """crt_denoise_adaptive_params of include/crt.h."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_variance", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float)]


def denoise_adaptive_defaults() -> DenoiseAdaptiveParams:
    """The library's defaults for crt_denoise_adaptive (crt_denoise_adaptive_defaults)."""
    p = DenoiseAdaptiveParams()
    if load().crt_denoise_adaptive_defaults(C.byref(p)) != 0:
        raise RuntimeError("crt_denoise_adaptive_defaults failed")
    return p


class DenoiseTemporalParams(C.Structure):
    """crt_denoise_temporal_params of include/crt.h."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float),
                ("max_history", C.c_float), ("normal_tol", C.c_float), ("plane_tol", C.c_float)]


def denoise_temporal_defaults() -> DenoiseTemporalParams:
    """The library's defaults for crt_denoise_temporal (crt_denoise_temporal_defaults)."""
    p = DenoiseTemporalParams()
    if load().crt_denoise_temporal_defaults(C.byref(p)) != 0:
        raise RuntimeError("crt_denoise_temporal_defaults failed")
    return p


class DenoiseSvgfParams(C.Structure):
    """crt_denoise_svgf_params of include/crt.h."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_variance", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float),
                ("max_history", C.c_float), ("normal_tol", C.c_float), ("plane_tol", C.c_float), ("min_frames", C.c_float)]


def denoise_svgf_defaults() -> DenoiseSvgfParams:
    """The library's defaults for crt_denoise_svgf (crt_denoise_svgf_defaults)."""
    p = DenoiseSvgfParams()
    if load().crt_denoise_svgf_defaults(C.byref(p)) != 0:
        raise RuntimeError("crt_denoise_svgf_defaults failed")
    return p


_lib = None


class CrtError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libcrt error {code}: {message}")
        self.code = code


def load():
    """dlopen libcrt.so and bind every entry point. Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C computeraytracer_amd/csrc)")
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)       # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib

"""Host driver over the C ABI: the Python counterpart of the reference's
``Main()`` / ``frame()`` (src/main.js:7-624) minus the browser.

    Main():  requestDevice                -> Renderer(device)
             createBuffer(b4..b8) + unmap -> Renderer.upload(PackedScene)
             accumulator + sample = 0     -> (done by upload / reset)
    frame(): dispatch(1); dispatch(W/8,H/8) -> Renderer.frame(n)   (n frames fused)
    (the reference never reads back; read_accum/read_rgba8 replace its blit pass)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ACCEL_BVH2, ACCEL_LBVH, ACCEL_NONE, ACCEL_PLOC, CNT, CrtError, NCOUNTERS
from .scene import PackedScene

_ACCEL = {"none": ACCEL_NONE, "brute": ACCEL_NONE, "bvh2": ACCEL_BVH2, "bvh": ACCEL_BVH2, "lbvh": ACCEL_LBVH, ACCEL_LBVH: ACCEL_LBVH,
          "ploc": ACCEL_PLOC, ACCEL_PLOC: ACCEL_PLOC, ACCEL_NONE: ACCEL_NONE, ACCEL_BVH2: ACCEL_BVH2}
AOV_PLANES = ("hits", "alpha", "depth", "normal", "albedo")
MATTE_PLANES = ("ids", "counts", "hits", "overflow")
MATTE_SOURCES = {"primitive": 0, "object": 1, "material": 2}
MATTE_NONE = 0xFFFFFFFF          # the id of a rank without an entry
QUERY_PLANES = ("hit", "prim", "id", "t", "position", "normal", "uv")
QUERY_MODES = {"closest": 0, "any": 1}
QUERY_NONE = 0xFFFFFFFF          # prim and id at a miss; the exclude index that excludes nothing
QUERY_NO_LIMIT = 2139095040.0    # t_max: the kernels' "infinity" (+inf means the same)
RAY_DTYPE = np.dtype([("o", np.float32, 3), ("t_max", np.float32), ("d", np.float32, 3), ("exclude", np.uint32)])   # crt_ray
_QUERY_SHAPE = {"hit": ((), np.uint32), "prim": ((), np.uint32), "id": ((), np.uint32), "t": ((), np.float32),
                "position": ((4,), np.float32), "normal": ((4,), np.float32), "uv": ((2,), np.float32)}
RADIANCE_PLANES = ("xyz", "y2", "rgba8")
PATH_KEY_DTYPE = np.dtype([("x", np.uint32), ("y", np.uint32), ("first_sample", np.uint32), ("reserved", np.uint32)])   # crt_path_key
_RADIANCE_SHAPE = {"xyz": ((4,), np.float32), "y2": ((), np.float32), "rgba8": ((4,), np.uint8)}


def pack_rays(origins, directions, t_max=None, exclude=None) -> np.ndarray:
    """n crt_ray records (RAY_DTYPE) from (n, 3) origins and directions; t_max None = no limit, a scalar or (n,) float32;
    exclude None = nothing, a scalar or (n,) uint32."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError("origins and directions must have the same length")
    rays = np.zeros(len(o), RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    rays["t_max"] = np.float32(QUERY_NO_LIMIT) if t_max is None else np.asarray(t_max, np.float32)
    rays["exclude"] = np.uint32(QUERY_NONE) if exclude is None else np.asarray(exclude, np.uint32)
    return rays


def pack_keys(x, y, first_sample=1) -> np.ndarray:
    """n crt_path_key records (PATH_KEY_DTYPE) from (n,) x and y and a scalar or (n,) first_sample, all uint32: the paths
    of a ray with key (x, y, s0) are seeded as samples s0, s0 + 1, ... of pixel (x, y)."""
    x = np.asarray(x, np.int64).reshape(-1)
    y, s = np.broadcast_to(np.asarray(y, np.int64), x.shape), np.broadcast_to(np.asarray(first_sample, np.int64), x.shape)
    for name, a in (("x", x), ("y", y), ("first_sample", s)):
        if ((a < 0) | (a > 0xFFFFFFFF)).any():
            raise ValueError(f"{name} must fit an unsigned 32-bit integer")
    keys = np.zeros(len(x), PATH_KEY_DTYPE)
    keys["x"], keys["y"], keys["first_sample"] = x, y, s
    return keys


def spectrum_rgb(spectrum, cie) -> np.ndarray:
    """crt_spectrum_rgb: the linear sRGB reflectance of spectrum (301 floats) under an equal-energy illuminant with white
    Y = 1, given the scene's CIE table (3 x 471): one row of Renderer.albedo_table.  Needs no context and no GPU."""
    s = np.ascontiguousarray(spectrum, np.float32)
    c = np.ascontiguousarray(cie, np.float32)
    if s.size != 301 or c.size != 3 * 471:
        raise ValueError("spectrum must be 301 floats, cie 3 x 471")
    out = np.empty(3, np.float32)
    rc = _lib.load().crt_spectrum_rgb(s.ctypes.data, c.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise CrtError(rc, "crt_spectrum_rgb failed")
    return out


def matte_coverage(planes: dict, n, id: int) -> np.ndarray:
    """(H, W) float32: the share of each pixel's n camera rays that hit `id`, count / n as one float32 division, from
    Renderer.render_mattes' dict (0 where the id holds no rank).  n is the sample count the planes were rendered with: a
    scalar, or an (H, W) array in the adaptive state (each pixel its tile's count; 0 / 0 is NaN)."""
    ids, counts = np.asarray(planes["ids"]), np.asarray(planes["counts"])
    count = np.where(ids == np.uint32(id), counts, np.uint32(0)).sum(axis=0, dtype=np.uint32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (count.astype(np.float32) / np.asarray(n).astype(np.float32)).astype(np.float32)


class Renderer:
    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.crt_create(C.byref(h), int(device))
        if rc != 0:
            raise CrtError(rc, (self._lib.crt_last_error(None) or b"").decode())
        self._h = h
        self.device = int(device)
        self.scene: PackedScene | None = None

    # -- plumbing
    def _chk(self, rc: int):
        if rc != 0:
            raise CrtError(rc, (self._lib.crt_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.crt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- Main()
    def upload(self, ps: PackedScene):
        prim = np.ascontiguousarray(ps.primitives)
        lights = np.ascontiguousarray(ps.lights)
        spectra = np.ascontiguousarray(ps.spectra, np.float32)
        cie = np.ascontiguousarray(ps.cie, np.float32)
        cam = np.ascontiguousarray(ps.camera, np.float32)
        if prim.nbytes % 80 or lights.nbytes % 80:
            raise ValueError("primitive / light buffers must be multiples of 80 bytes")
        if spectra.size % 301 or cie.size != 3 * 471 or cam.size != 16:
            raise ValueError("spectra must be n x 301, cie 3 x 471, camera 16 floats")
        self._chk(self._lib.crt_upload_scene(self._h, prim.ctypes.data, prim.nbytes // 80,
                                             lights.ctypes.data, lights.nbytes // 80,
                                             spectra.ctypes.data, spectra.size // 301,
                                             cie.ctypes.data, cam.ctypes.data))
        self.scene = ps
        if getattr(ps, "object_ids", None) is not None:
            self.set_primitive_ids(0, ps.object_ids)
        return self

    def set_tile(self, x0: int, y0: int, x1: int, y1: int):
        self._chk(self._lib.crt_set_tile(self._h, x0, y0, x1, y1))
        return self

    def set_row_bands(self, band_rows: int, parts: int, part: int):
        self._chk(self._lib.crt_set_row_bands(self._h, band_rows, parts, part))
        return self

    def build_accel(self, mode="bvh2"):
        self._chk(self._lib.crt_build_accel(self._h, _ACCEL[mode]))
        return self

    def reset(self):
        self._chk(self._lib.crt_reset(self._h))
        return self

    def set_option(self, name: str, value: int):
        self._chk(self._lib.crt_set_option(self._h, name.encode(), int(value)))
        return self

    # -- scene edits (include/crt.h, "Scene edits"): each finishes what is in flight and restarts the accumulation
    def set_camera(self, camera):
        """A new camera (16 floats as packed by scene.pack_camera; width and height unchanged)."""
        cam = np.ascontiguousarray(camera, np.float32)
        if cam.size != 16:
            raise ValueError("camera must be 16 floats")
        self._chk(self._lib.crt_set_camera(self._h, cam.ctypes.data))
        if self.scene is not None:
            self.scene = PackedScene(self.scene.primitives, self.scene.lights, cam.copy(), self.scene.spectra, self.scene.cie,
                                     self.scene.patches, self.scene.spectrum_index)
        return self

    @staticmethod
    def _records(records) -> np.ndarray:
        rec = np.ascontiguousarray(records)
        if rec.nbytes % 80:
            raise ValueError("records must be a multiple of 80 bytes")
        return rec

    def update_primitives(self, first: int, records):
        """Replace primitive records [first, first + len(records)); the tree goes stale until refit_accel()."""
        rec = self._records(records)
        self._chk(self._lib.crt_update_primitives(self._h, int(first), rec.nbytes // 80, rec.ctypes.data))
        return self

    def transform_primitives(self, ops):
        """Move primitive ranges on the device (crt_transform_primitives): ops as scene.transform_ops takes them, e.g.
        [(first, count, m)] with m the 3 x 4 matrix (R | t), or (first, count, m, radius_scale) where spheres scale.
        The tree goes stale until refit_accel(); read_primitives shows the moved records."""
        from .scene import transform_ops
        t = transform_ops(ops)
        self._chk(self._lib.crt_transform_primitives(self._h, t.ctypes.data if len(t) else None, len(t)))
        return self

    def _edited(self, ps: PackedScene, lights):
        """self.scene after a topology edit: the records of `ps`, and its remapped lights unless the caller gave a list."""
        if lights is not None:
            from .scene import PRIM_DTYPE
            ps = PackedScene(ps.primitives, np.ascontiguousarray(lights).view(PRIM_DTYPE).reshape(-1).copy(), ps.camera, ps.spectra,
                             ps.cie, ps.patches, ps.spectrum_index)
        self.scene = ps

    def remove_primitives(self, ranges, lights=None):
        """Remove primitive ranges [(first, count), ...] on the device (crt_remove_primitives): the survivors close ranks and
        are renumbered.  lights None keeps the light list (its primitive indices follow); else the new list, whole.  With a
        tree, refit_accel() then rebuilds it.  self.scene becomes scene.remove_records(self.scene, ranges)."""
        from .scene import remove_records
        rg = np.ascontiguousarray(np.asarray(ranges, np.int64).reshape(-1, 2).astype(np.uint32))
        lt = None if lights is None else self._records(lights)
        self._chk(self._lib.crt_remove_primitives(self._h, rg.ctypes.data if len(rg) else None, len(rg),
                                                  None if lt is None else lt.ctypes.data, 0 if lt is None else lt.nbytes // 80))
        if self.scene is not None:
            self._edited(remove_records(self.scene, rg, remap_lights=lights is None), lights)
        return self

    def append_primitives(self, records, lights=None):
        """Add records after the last primitive (crt_append_primitives; each record's index is its position in the new
        list).  lights as for remove_primitives.  With a tree, refit_accel() then rebuilds it."""
        from .scene import append_records
        rec = self._records(records)
        lt = None if lights is None else self._records(lights)
        self._chk(self._lib.crt_append_primitives(self._h, rec.ctypes.data if rec.nbytes else None, rec.nbytes // 80,
                                                  None if lt is None else lt.ctypes.data, 0 if lt is None else lt.nbytes // 80))
        if self.scene is not None:
            self._edited(append_records(self.scene, rec), lights)
        return self

    def read_primitives(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """Primitive records [first, first + count) as they lie on the device (PRIM_DTYPE; count None: to the end)."""
        from .scene import PRIM_DTYPE
        if count is None:
            count = len(self.scene.primitives) - int(first)
        out = np.zeros(int(count), PRIM_DTYPE)
        self._chk(self._lib.crt_read_primitives(self._h, int(first), int(count), out.ctypes.data if count else None))
        return out

    def update_lights(self, first: int, records):
        """Replace light records [first, first + len(records)) (e.g. scene.lights_of(edited primitives))."""
        rec = self._records(records)
        self._chk(self._lib.crt_update_lights(self._h, int(first), rec.nbytes // 80, rec.ctypes.data))
        return self

    def refit_accel(self) -> bool:
        """Recompute the tree's boxes on the GPU; True when it had to be rebuilt instead."""
        rebuilt = C.c_int()
        self._chk(self._lib.crt_refit_accel(self._h, C.byref(rebuilt)))
        return bool(rebuilt.value)

    def accel_quality(self) -> dict:
        """The surface-area cost of the trees as they lie on the device (crt_accel_quality): now = (boxes2, prims2,
        boxes4, prims4), built = the same for the tree before any refit, q_now / q_built = boxes + prims of the tree the
        wavefront kernels walk (what option "refit_rebuild_pct" compares), refits since the build, the policy's rebuilds
        since the context was created, and has4 (False: the 8-wide tree is walked; boxes4 / prims4, q_now and q_built are
        NaN, and the policy never acts).  A sync point; works on a stale tree; reads only."""
        out = np.zeros(12, np.float64)
        self._chk(self._lib.crt_accel_quality(self._h, out.ctypes.data))
        names = ("boxes2", "prims2", "boxes4", "prims4")
        now, built = dict(zip(names, map(float, out[0:4]))), dict(zip(names, map(float, out[4:8])))
        def q(d):                         # (has4 False: NaN, as the library's own comparison, which then takes no action)
            return d["boxes4"] + d["prims4"]
        return dict(now=now, built=built, q_now=q(now), q_built=q(built), refits=int(out[8]), rebuilds=int(out[9]),
                    has4=bool(out[10]), raw=out)

    @property
    def debug_hit_pad(self) -> float:
        v = C.c_float()
        self._chk(self._lib.crt_debug_hit_pad(self._h, C.byref(v)))
        return v.value

    # -- frame()
    def frame(self, n_samples: int = 1):
        """n x { sample++ ; trace }  (asynchronous)."""
        self._chk(self._lib.crt_trace(self._h, int(n_samples)))
        return self

    def sync(self):
        self._chk(self._lib.crt_sync(self._h))
        return self

    # -- adaptive sampling (include/crt.h, "Adaptive sampling")
    def trace_adaptive(self, samples: int | None = None, threshold: float | None = None, min_samples: int | None = None,
                       max_samples: int | None = None) -> int:
        """`samples` more samples for every 8x8 tile that is still active (asynchronous); returns how many tiles that
        was -- 0 when every tile has converged or reached max_samples (0 = no limit).  The first call needs sample 0.
        A parameter left out takes the library's default (crt_adaptive_defaults)."""
        n = C.c_uint32()
        self._chk(self._lib.crt_trace_adaptive(self._h, C.byref(self._adaptive_params(samples, threshold, min_samples, max_samples)),
                                               C.byref(n)))
        return int(n.value)

    @staticmethod
    def _adaptive_params(samples, threshold, min_samples, max_samples):
        p = _lib.adaptive_defaults()
        for k, v in (("samples", samples), ("min_samples", min_samples), ("max_samples", max_samples)):
            if v is not None:
                setattr(p, k, int(v))
        if threshold is not None:
            p.threshold = float(threshold)
        return p

    @staticmethod
    def _filter_params(iterations, sigma_variance, sigma_normal, sigma_plane):
        d = _lib.denoise_adaptive_defaults()
        if iterations is not None:
            d.iterations = int(iterations)
        for k, v in (("sigma_variance", sigma_variance), ("sigma_normal", sigma_normal), ("sigma_plane", sigma_plane)):
            if v is not None:
                setattr(d, k, float(v))
        return d

    def trace_adaptive_filtered(self, samples: int | None = None, threshold: float | None = None, min_samples: int | None = None,
                                max_samples: int | None = None, iterations: int | None = None,
                                sigma_variance: float | None = None, sigma_normal: float | None = None,
                                sigma_plane: float | None = None) -> int:
        """trace_adaptive with the tiles judged by what denoise_adaptive(iterations, sigma_variance, sigma_normal,
        sigma_plane) leaves of their noise (include/crt.h "Adaptive sampling judged by the filtered preview"): E' =
        sqrt(max of the filter's var over the tile) in E's place.  Returns the tiles it sampled.  A parameter left out
        takes the library's default (crt_adaptive_defaults, crt_denoise_adaptive_defaults)."""
        n = C.c_uint32()
        p = self._adaptive_params(samples, threshold, min_samples, max_samples)
        d = self._filter_params(iterations, sigma_variance, sigma_normal, sigma_plane)
        self._chk(self._lib.crt_trace_adaptive_filtered(self._h, C.byref(p), C.byref(d), C.byref(n)))
        return int(n.value)

    def read_adaptive_filtered(self, iterations: int | None = None, sigma_variance: float | None = None,
                               sigma_normal: float | None = None, sigma_plane: float | None = None):
        """read_adaptive with errors = E' as the next trace_adaptive_filtered with this filter judges it; the same
        shapes.  Reads only; finishes what is in flight."""
        _, _, tw, th = self.tile
        tx, ty = (tw + 7) // 8, (th + 7) // 8
        counts = np.zeros((ty, tx), np.uint32)
        errors = np.zeros((ty, tx), np.float32)
        d = self._filter_params(iterations, sigma_variance, sigma_normal, sigma_plane)
        self._chk(self._lib.crt_read_adaptive_filtered(self._h, C.byref(d), counts.ctypes.data, errors.ctypes.data))
        return counts, errors

    def read_adaptive(self):
        """(counts (tiles_y, tiles_x) uint32, errors (tiles_y, tiles_x) float32): the samples each tile holds and its
        error E as the next trace_adaptive judges it."""
        _, _, tw, th = self.tile
        tx, ty = (tw + 7) // 8, (th + 7) // 8
        counts = np.zeros((ty, tx), np.uint32)
        errors = np.zeros((ty, tx), np.float32)
        self._chk(self._lib.crt_read_adaptive(self._h, counts.ctypes.data, errors.ctypes.data))
        return counts, errors

    @property
    def sample(self) -> int:
        v = C.c_uint32()
        self._chk(self._lib.crt_sample_count(self._h, C.byref(v)))
        return v.value

    @property
    def tile(self):
        out = (C.c_uint32 * 4)()
        self._chk(self._lib.crt_tile(self._h, out))
        return tuple(out)

    # -- readback
    def read_accum(self) -> np.ndarray:
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.float32)
        self._chk(self._lib.crt_read_accum(self._h, out.ctypes.data))
        return out

    def read_rgba8(self) -> np.ndarray:
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.uint8)
        self._chk(self._lib.crt_read_rgba8(self._h, out.ctypes.data))
        return out

    def read_latest_rgba8(self):
        """(frame, sample index): the newest complete frame in stream order, without finishing what is in flight."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.uint8)
        s = C.c_uint32()
        self._chk(self._lib.crt_read_latest_rgba8(self._h, out.ctypes.data, C.byref(s)))
        return out, s.value

    @property
    def latest_sample(self) -> int:
        v = C.c_uint32()
        self._chk(self._lib.crt_latest_sample(self._h, C.byref(v)))
        return v.value

    def read_sample_rgba8(self, sample: int) -> np.ndarray:
        """The frame after exactly `sample` samples (option frame_ring = F keeps the last F)."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.uint8)
        self._chk(self._lib.crt_read_sample_rgba8(self._h, int(sample), out.ctypes.data))
        return out

    def write_accum(self, accum: np.ndarray, sample: int):
        a = np.ascontiguousarray(accum, np.float32)
        _, _, tw, th = self.tile
        if a.size != tw * th * 4:
            raise ValueError("accum must be th x tw x 4 float32")
        self._chk(self._lib.crt_write_accum(self._h, a.ctypes.data, int(sample)))
        return self

    def device_buffers(self):
        a, r = C.c_void_p(), C.c_void_p()
        self._chk(self._lib.crt_device_buffers(self._h, C.byref(a), C.byref(r)))
        return a.value, r.value

    def bind_output(self, accum_dev_ptr: int | None, rgba_dev_ptr: int | None):
        self._chk(self._lib.crt_bind_output(self._h, C.c_void_p(accum_dev_ptr or 0), C.c_void_p(rgba_dev_ptr or 0)))
        return self

    def set_stream(self, hip_stream: int | None):
        self._chk(self._lib.crt_set_stream(self._h, C.c_void_p(hip_stream or 0)))
        return self

    # -- denoised preview (include/crt.h, "Denoised preview")
    def _denoise(self, call, p, overrides: dict, rgb: bool, plane: bool | None = None, shape=None):
        """One filter call.  The overrides that are not None replace fields of the parameter struct p, as the field's
        type.  Returns rgba8, or a tuple of it, the linear rgb (rgb) and the filter's own float plane (plane; None: the
        call has none).  shape: (W, H) of the outputs, the tile's by default."""
        tw, th = shape if shape else self.tile[2:]
        for k, v in overrides.items():
            if v is not None:
                setattr(p, k, type(getattr(p, k))(v))
        rgba = np.empty((th, tw, 4), np.uint8)
        lin = np.empty((th, tw, 4), np.float32) if rgb else None
        extra = np.empty((th, tw), np.float32) if plane else None
        args = [lin.ctypes.data if rgb else None, rgba.ctypes.data]
        if plane is not None:
            args.append(extra.ctypes.data if plane else None)
        self._chk(call(self._h, C.byref(p), *args))
        out = tuple(a for a in (rgba, lin, extra) if a is not None)
        return out if len(out) > 1 else rgba

    def denoise(self, iterations: int = 5, sigma_color: float = 1.0, sigma_normal: float = 0.5,
                sigma_plane: float = 0.3, rgb: bool = False):
        """The edge-aware a-trous filter of the accumulator's average: rgba8 (H, W, 4), or (rgba8, linear rgb
        (H, W, 4) float32, channel 3 = pad) with rgb=True.  Reads the accumulator only; finishes what is in flight."""
        return self._denoise(self._lib.crt_denoise, _lib.DenoiseParams(), dict(
            iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_plane=sigma_plane), rgb)

    def denoise_latest(self, iterations: int = 5, sigma_color: float = 1.0, sigma_normal: float = 0.5,
                       sigma_plane: float = 0.3, rgb: bool = True, rgba8: bool = True):
        """denoise() of the newest complete frame without finishing what is in flight (crt_denoise_latest): (linear rgb
        (H, W, 4) float32 or None, rgba8 (H, W, 4) or None, s), the filtered frame of exactly s samples.  CrtError
        (CRT_ESTATE) while no frame is complete yet."""
        _, _, tw, th = self.tile
        p = _lib.DenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_plane))
        lin = np.empty((th, tw, 4), np.float32) if rgb else None
        out = np.empty((th, tw, 4), np.uint8) if rgba8 else None
        s = C.c_uint32()
        self._chk(self._lib.crt_denoise_latest(self._h, C.byref(p), lin.ctypes.data if rgb else None,
                                               out.ctypes.data if rgba8 else None, C.byref(s)))
        return lin, out, s.value

    def denoise_adaptive(self, iterations: int | None = None, sigma_variance: float | None = None,
                         sigma_normal: float | None = None, sigma_plane: float | None = None, rgb: bool = False,
                         var: bool = False):
        """The variance-guided a-trous filter of an adaptive render (include/crt.h "Denoised preview of an adaptive
        render"): rgba8 (H, W, 4); with rgb=True also linear rgb (H, W, 4) float32 (channel 3 = the variance), with
        var=True also the variance left after filtering (H, W) float32 -- a tuple in that order.  A parameter left out
        takes the library's default (crt_denoise_adaptive_defaults).  Reads only; finishes what is in flight."""
        return self._denoise(self._lib.crt_denoise_adaptive, _lib.denoise_adaptive_defaults(), dict(
            iterations=iterations, sigma_variance=sigma_variance, sigma_normal=sigma_normal, sigma_plane=sigma_plane), rgb, bool(var))

    # -- temporal reuse (include/crt.h, "Sample offset" and "Temporal reuse across camera moves")
    def set_sample_offset(self, offset: int):
        """Sample j since the reset is drawn with the reference's index offset + j (set at sample 0; wavefront only).
        trace_adaptive takes it with set_option("adaptive_temporal", 1), which also lets denoise_temporal, denoise_svgf
        and read_motion work on an adaptive frame, each pixel blended with its own tile's count."""
        self._chk(self._lib.crt_set_sample_offset(self._h, int(offset)))
        return self

    @property
    def sample_offset(self) -> int:
        v = C.c_uint32()
        self._chk(self._lib.crt_sample_offset(self._h, C.byref(v)))
        return v.value

    def denoise_temporal(self, iterations: int | None = None, sigma_color: float | None = None,
                         sigma_normal: float | None = None, sigma_plane: float | None = None,
                         max_history: float | None = None, normal_tol: float | None = None, plane_tol: float | None = None,
                         rgb: bool = False, history: bool = False):
        """The frame blended with the previous frame's reprojected result, then the a-trous filter: rgba8 (H, W, 4); with
        rgb=True also linear rgb (H, W, 4) float32 (channel 3 = the history weight Hw in samples), with history=True
        also Hw (H, W) float32 -- a tuple in that order.  A parameter left out takes the library's default
        (crt_denoise_temporal_defaults).  Reads the accumulator only; finishes what is in flight.
        set_option("temporal_clip_pct", P) (0 = off, the default; 25..10000) clamps the reprojected history of every pixel
        to mean +- (P / 100) standard deviations of the frame's own colours over its 7x7 neighbourhood before the blend, so
        lighting that changed on an unchanged surface (a shadow that moved on) stops trailing, and update_lights keeps the
        history (include/crt.h "Clipped history"; debug_read_clip_box returns the boxes)."""
        return self._denoise(self._lib.crt_denoise_temporal, _lib.denoise_temporal_defaults(), dict(
            iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_plane=sigma_plane,
            max_history=max_history, normal_tol=normal_tol, plane_tol=plane_tol), rgb, bool(history))

    def temporal_reset(self):
        """Drop the history: the next denoise_temporal equals denoise."""
        self._chk(self._lib.crt_denoise_temporal_reset(self._h))
        return self

    def denoise_svgf(self, iterations: int | None = None, sigma_variance: float | None = None,
                     sigma_normal: float | None = None, sigma_plane: float | None = None,
                     max_history: float | None = None, normal_tol: float | None = None, plane_tol: float | None = None,
                     min_frames: float | None = None, rgb: bool = False, history: bool = False, var: bool = False):
        """denoise_temporal's blend followed by the variance-guided filter, the variance taken from the temporal moments
        of the pixel's luminance (include/crt.h "Variance-guided temporal filter"): rgba8 (H, W, 4); with rgb=True also
        linear rgb (H, W, 4) float32 (channel 3 = the variance), with history=True also Hw, with var=True also the
        variance left after filtering, both (H, W) float32 -- a tuple in that order.  A parameter left out takes the
        library's default (crt_denoise_svgf_defaults).  Reads the accumulator only; finishes what is in flight.
        set_option("svgf_spatial_pct", P) (0 = off, the default; 25..10000) gives the pixels whose history is too short for
        that variance one from the spread of their 7x7 neighbourhood, times P / 100; the history does not depend on it.
        set_option("temporal_clip_pct", P) clips the history as it does for denoise_temporal: the colour CURRENT keeps is
        the clipped blend, the moments are untouched, so a relit pixel's variance rises and the passes blur it more for a
        few frames."""
        _, _, tw, th = self.tile
        p = _lib.denoise_svgf_defaults()
        for k, v in dict(iterations=iterations, sigma_variance=sigma_variance, sigma_normal=sigma_normal, sigma_plane=sigma_plane,
                         max_history=max_history, normal_tol=normal_tol, plane_tol=plane_tol, min_frames=min_frames).items():
            if v is not None:
                setattr(p, k, type(getattr(p, k))(v))
        rgba = np.empty((th, tw, 4), np.uint8)
        lin = np.empty((th, tw, 4), np.float32) if rgb else None
        hw = np.empty((th, tw), np.float32) if history else None
        vv = np.empty((th, tw), np.float32) if var else None
        self._chk(self._lib.crt_denoise_svgf(self._h, C.byref(p), lin.ctypes.data if rgb else None, rgba.ctypes.data,
                                             hw.ctypes.data if history else None, vv.ctypes.data if var else None))
        out = tuple(a for a in (rgba, lin, hw, vv) if a is not None)
        return out if len(out) > 1 else rgba

    def read_moments(self) -> np.ndarray:
        """(H, W, 4) float32 per tile pixel: (m1, s, Mw, 0) of the slot the last denoise_svgf of this frame left -- mean
        luminance, variance of the frame means, the weight in samples behind both (crt_debug_read_moments, a test
        hook)."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.float32)
        self._chk(self._lib.crt_debug_read_moments(self._h, out.ctypes.data))
        return out

    def debug_read_clip_box(self) -> np.ndarray:
        """(H, W, 8) float32 per tile pixel: lo.rgb, N, hi.rgb, valid (1.0 / 0.0) -- the box the last temporal call of this
        frame clamped the pixel's history to under option "temporal_clip_pct", the number of taps behind it, and whether it
        was used; N = 0 where the pixel has no box (crt_debug_read_clip_box, a test hook)."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 8), np.float32)
        self._chk(self._lib.crt_debug_read_clip_box(self._h, out.ctypes.data))
        return out

    def read_motion(self) -> np.ndarray:
        """(H, W, 2) float32 per tile pixel: the film position (u, v), in the tile's own pixel coordinates, where the
        last denoise_temporal looked for the pixel in the previous frame; NaN where there is none (no previous frame, a
        miss, glass, behind the previous camera, a primitive edit the map refuses).  Option "temporal_motion" = 1 makes
        it follow update_primitives."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 2), np.float32)
        self._chk(self._lib.crt_read_motion(self._h, out.ctypes.data))
        return out

    def read_gbuffer(self) -> np.ndarray:
        """(H, W, 8) float32 per tile pixel: t, position, normal, hit index bits (0xFFFFFFFF = miss) of the primary
        ray of sample 8 -- the crt_debug_intersect record."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 8), np.float32)
        self._chk(self._lib.crt_read_gbuffer(self._h, out.ctypes.data))
        return out

    # -- feature planes (include/crt.h, "Feature planes")
    def render_aovs(self, n_samples: int = 0, planes=AOV_PLANES) -> dict:
        """The feature planes of the tile (crt_render_aovs), averaged over the camera rays of n_samples samples from the
        sample offset on; n_samples = 0: the samples the accumulator holds (in the adaptive state each 8x8 tile's own
        count).  A dict of the planes asked for: hits (H, W) uint32, alpha and depth (H, W) float32, normal and albedo
        (H, W, 4) float32 with channel 3 = 0.  Finishes what is in flight; only reads."""
        _, _, tw, th = self.tile
        unknown = [p for p in planes if p not in AOV_PLANES]
        if unknown:
            raise ValueError(f"unknown planes {unknown}: choose from {AOV_PLANES}")
        out = {p: np.empty((th, tw, 4) if p in ("normal", "albedo") else (th, tw), np.uint32 if p == "hits" else np.float32)
               for p in AOV_PLANES if p in planes}
        arg = _lib.AovPlanes(**{p: a.ctypes.data for p, a in out.items()})
        self._chk(self._lib.crt_render_aovs(self._h, int(n_samples), C.byref(arg)))
        return out

    def albedo_table(self) -> np.ndarray:
        """(nspectra, 3) float32: spectrum_rgb of every spectra row of the uploaded scene, the table render_aovs reads."""
        if self.scene is None:
            raise ValueError("upload a scene first")
        out = np.empty((np.asarray(self.scene.spectra).size // 301, 3), np.float32)
        self._chk(self._lib.crt_read_albedo_table(self._h, out.ctypes.data))
        return out

    # -- id mattes (include/crt.h, "ID mattes")
    def render_mattes(self, n_samples: int = 0, source="object", slots: int = 8, planes=MATTE_PLANES) -> dict:
        """The id mattes of the tile (crt_render_mattes) over the camera rays of n_samples samples from the sample offset
        on; n_samples = 0: the samples the accumulator holds (in the adaptive state each 8x8 tile's own count).  source:
        "primitive", "object" (the id table: set_primitive_ids) or "material".  A dict of the planes asked for, all
        uint32: ids and counts (slots, H, W), rank 0 first, MATTE_NONE / 0 where a rank has no entry; hits and overflow
        (H, W).  matte_coverage turns an id's counts into its coverage.  Finishes what is in flight; only reads."""
        _, _, tw, th = self.tile
        unknown = [p for p in planes if p not in MATTE_PLANES]
        if unknown:
            raise ValueError(f"unknown planes {unknown}: choose from {MATTE_PLANES}")
        if source not in MATTE_SOURCES and source not in MATTE_SOURCES.values():
            raise ValueError(f"unknown source {source!r}: choose from {tuple(MATTE_SOURCES)}")
        out = {p: np.empty((int(slots), th, tw) if p in ("ids", "counts") else (th, tw), np.uint32)
               for p in MATTE_PLANES if p in planes}
        arg = _lib.MattePlanes(**{p: a.ctypes.data for p, a in out.items()})
        self._chk(self._lib.crt_render_mattes(self._h, int(n_samples), int(MATTE_SOURCES.get(source, source)), int(slots), C.byref(arg)))
        return out

    def set_primitive_ids(self, first: int, ids):
        """Replace entries [first, first + len(ids)) of the id table (crt_set_primitive_ids): the ids source "object"
        reports.  Touches nothing else: no reset, no stale tree."""
        a = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        self._chk(self._lib.crt_set_primitive_ids(self._h, int(first), len(a), a.ctypes.data if len(a) else None))
        return self

    def primitive_ids(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """Entries [first, first + count) of the id table (uint32; count None: to the end).  No GPU work."""
        if count is None:
            count = len(self.scene.primitives) - int(first)
        out = np.zeros(int(count), np.uint32)
        self._chk(self._lib.crt_read_primitive_ids(self._h, int(first), int(count), out.ctypes.data if count else None))
        return out

    # -- ray queries (include/crt.h, "Ray queries")
    @staticmethod
    def _query_planes(mode, planes):
        if mode not in QUERY_MODES and mode not in QUERY_MODES.values():
            raise ValueError(f"unknown mode {mode!r}: choose from {tuple(QUERY_MODES)}")
        mode = int(QUERY_MODES.get(mode, mode))
        if planes is None:
            planes = ("hit",) if mode == 1 else QUERY_PLANES
        unknown = [p for p in planes if p not in QUERY_PLANES]
        if unknown:
            raise ValueError(f"unknown planes {unknown}: choose from {QUERY_PLANES}")
        return mode, [p for p in QUERY_PLANES if p in planes]

    def query_rays(self, origins=None, directions=None, t_max=None, exclude=None, mode="closest", planes=None, rays=None) -> dict:
        """What the rays hit (crt_query_rays): the closest hit of each ray, or with mode "any" only whether there is one.
        Rays: (n, 3) origins and directions with optional t_max (None = no limit) and exclude (a primitive index, None =
        nothing) -- or rays=: n packed records (RAY_DTYPE, see pack_rays), or a torch tensor (n, 8) float32, contiguous, on
        this context's device, each row (o, t_max, d, exclude bits) (crt_query_rays_device on torch's current stream: nothing
        is copied through the host and nothing waits).  A dict of the planes asked for (default: all; mode "any": hit
        alone): hit, prim, id uint32 (n,), t float32 (n,), position and normal float32 (n, 4), uv float32 (n, 2) -- numpy
        arrays, or torch tensors for a torch input.  Does not finish or disturb what is in flight; only reads."""
        mode, names = self._query_planes(mode, planes)
        if rays is not None and not isinstance(rays, np.ndarray) and type(rays).__module__.split(".")[0] == "torch":
            return self._query_rays_torch(rays, mode, names)
        if rays is None:
            rays = pack_rays(origins, directions, t_max, exclude)
        else:
            rays = np.ascontiguousarray(rays)
            if rays.dtype != RAY_DTYPE:
                rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8).view(RAY_DTYPE).reshape(-1)
        n = len(rays)
        out = {p: np.empty((n,) + _QUERY_SHAPE[p][0], _QUERY_SHAPE[p][1]) for p in names}
        arg = _lib.QueryPlanes(**{p: a.ctypes.data for p, a in out.items()})
        self._chk(self._lib.crt_query_rays(self._h, rays.ctypes.data if n else None, n, mode, C.byref(arg)))
        return out

    def _query_rays_torch(self, rays, mode, names) -> dict:
        import torch
        if rays.device.type != "cuda" or rays.device.index != self.device:
            raise ValueError(f"rays are on {rays.device}, the context on cuda:{self.device}")
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
            raise ValueError("rays must be a contiguous (n, 8) float32 tensor: (o, t_max, d, exclude bits) per row")
        n = rays.shape[0]
        kinds = {np.uint32: torch.int32, np.float32: torch.float32}     # (uint32 planes as int32 storage: view them as needed)
        with torch.cuda.device(self.device):
            out = {p: torch.empty((n,) + _QUERY_SHAPE[p][0], dtype=kinds[_QUERY_SHAPE[p][1]], device=rays.device) for p in names}
            if n == 0:                                          # (an empty tensor has no pointer to pass)
                return out
            arg = _lib.QueryPlanes(**{p: a.data_ptr() for p, a in out.items()})
            stream = torch.cuda.current_stream(rays.device).cuda_stream
            self._chk(self._lib.crt_query_rays_device(self._h, rays.data_ptr() if n else None, n, mode, C.byref(arg), stream))
        return out

    def pick(self, x: int, y: int):
        """What is under pixel (x, y) of the full image (crt_pick; global coordinates, whatever the tile): a dict of
        scalars -- prim, id, t, position (3,), normal (3,), uv (2,) -- of the G-buffer's ray of that pixel, or None where
        it hits nothing.  Does not finish or disturb what is in flight."""
        got = self.pick_pixels([(x, y)])
        if not got["hit"][0]:
            return None
        return dict(prim=int(got["prim"][0]), id=int(got["id"][0]), t=float(got["t"][0]), position=got["position"][0, :3].copy(),
                    normal=got["normal"][0, :3].copy(), uv=got["uv"][0].copy())

    def pick_pixels(self, xy, planes=QUERY_PLANES) -> dict:
        """crt_pick for n pixels at once: xy (n, 2) global (x, y); the planes as query_rays returns them."""
        _, names = self._query_planes("closest", planes)
        p = np.ascontiguousarray(np.asarray(xy, np.int64).reshape(-1, 2))
        if ((p < 0) | (p > 0xFFFFFFFF)).any():
            raise ValueError("pixel coordinates must be non-negative")
        p = np.ascontiguousarray(p.astype(np.uint32))
        n = len(p)
        out = {k: np.empty((n,) + _QUERY_SHAPE[k][0], _QUERY_SHAPE[k][1]) for k in names}
        arg = _lib.QueryPlanes(**{k: a.ctypes.data for k, a in out.items()})
        self._chk(self._lib.crt_pick(self._h, p.ctypes.data if n else None, n, C.byref(arg)))
        return out

    # -- radiance queries (include/crt.h, "Radiance queries")
    @staticmethod
    def _radiance_args(n_samples, planes):
        n_samples = int(n_samples)
        if not 1 <= n_samples <= 0xFFFFFFFF:
            raise ValueError("n_samples must be 1 .. 2^32 - 1")
        if planes is None:
            planes = RADIANCE_PLANES
        unknown = [p for p in planes if p not in RADIANCE_PLANES]
        if unknown:
            raise ValueError(f"unknown planes {unknown}: choose from {RADIANCE_PLANES}")
        names = [p for p in RADIANCE_PLANES if p in planes]
        if not names:
            raise ValueError(f"no plane asked for: choose from {RADIANCE_PLANES}")
        return n_samples, names

    def radiance_rays(self, origins=None, directions=None, keys=None, n_samples=1, t_max=None, exclude=None, planes=None,
                      rays=None) -> dict:
        """How much light arrives along the rays (crt_radiance_rays): n_samples paths of the path tracer from each ray,
        summed.  Rays as for query_rays (directions must be unit vectors; t_max and exclude bear on the first segment
        only).  keys: n records (PATH_KEY_DTYPE, see pack_keys) or an (n, 4) integer array (x, y, first_sample, 0): the
        paths of a ray are seeded as samples first_sample, first_sample + 1, ... of pixel (x, y); None = (i, 0, 1).  With a
        torch (n, 8) float32 tensor on this context's device as rays= the call is crt_radiance_rays_device on torch's
        current stream, and keys is a torch (n, 4) int32 or uint32 tensor there, or None.  A dict of the planes asked for
        (default: all): xyz float32 (n, 4) the sum of the paths' XYZ, y2 float32 (n,) the sum of Y * Y, rgba8 uint8 (n, 4)
        the tone-mapped mean -- numpy arrays, or torch tensors for a torch input.  Does not finish or disturb what is in
        flight; only reads."""
        n_samples, names = self._radiance_args(n_samples, planes)
        if rays is not None and not isinstance(rays, np.ndarray) and type(rays).__module__.split(".")[0] == "torch":
            return self._radiance_rays_torch(rays, keys, n_samples, names)
        if rays is None:
            rays = pack_rays(origins, directions, t_max, exclude)
        else:
            rays = np.ascontiguousarray(rays)
            if rays.dtype != RAY_DTYPE:
                rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8).view(RAY_DTYPE).reshape(-1)
        n = len(rays)
        if keys is not None:
            keys = np.ascontiguousarray(keys)
            if keys.dtype != PATH_KEY_DTYPE:
                if keys.dtype.kind not in "iu":
                    raise ValueError("keys must be PATH_KEY_DTYPE records or an (n, 4) integer array")
                keys = np.ascontiguousarray(keys.reshape(-1, 4).astype(np.uint32)).view(PATH_KEY_DTYPE).reshape(-1)
            if len(keys) != n:
                raise ValueError(f"{len(keys)} keys for {n} rays")
        out = {p: np.empty((n,) + _RADIANCE_SHAPE[p][0], _RADIANCE_SHAPE[p][1]) for p in names}
        arg = _lib.RadiancePlanes(**{p: a.ctypes.data for p, a in out.items()})
        self._chk(self._lib.crt_radiance_rays(self._h, rays.ctypes.data if n else None, keys.ctypes.data if keys is not None and n else None,
                                              n, n_samples, C.byref(arg)))
        return out

    def _radiance_rays_torch(self, rays, keys, n_samples, names) -> dict:
        import torch
        if rays.device.type != "cuda" or rays.device.index != self.device:
            raise ValueError(f"rays are on {rays.device}, the context on cuda:{self.device}")
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
            raise ValueError("rays must be a contiguous (n, 8) float32 tensor: (o, t_max, d, exclude bits) per row")
        n = rays.shape[0]
        if keys is not None:
            if not isinstance(keys, torch.Tensor) or keys.device != rays.device:
                raise ValueError(f"keys must be a torch tensor on {rays.device}, as the rays are")
            if keys.dtype not in (torch.int32, torch.uint32) or tuple(keys.shape) != (n, 4) or not keys.is_contiguous():
                raise ValueError("keys must be a contiguous (n, 4) int32 or uint32 tensor: (x, y, first_sample, 0) per row")
        kinds = {np.float32: torch.float32, np.uint8: torch.uint8}
        with torch.cuda.device(self.device):
            out = {p: torch.empty((n,) + _RADIANCE_SHAPE[p][0], dtype=kinds[_RADIANCE_SHAPE[p][1]], device=rays.device) for p in names}
            if n == 0:                                          # (an empty tensor has no pointer to pass)
                return out
            arg = _lib.RadiancePlanes(**{p: a.data_ptr() for p, a in out.items()})
            stream = torch.cuda.current_stream(rays.device).cuda_stream
            self._chk(self._lib.crt_radiance_rays_device(self._h, rays.data_ptr(), keys.data_ptr() if keys is not None else None,
                                                         n, n_samples, C.byref(arg), stream))
        return out

    def radiance_lanes(self, n: int) -> int:
        """crt_debug_radiance_lanes: the lanes G of the grid a radiance call of n rays launches (lane g owns rays g, g + G, ...)."""
        v = C.c_uint64()
        self._chk(self._lib.crt_debug_radiance_lanes(self._h, int(n), C.byref(v)))
        return int(v.value)

    @staticmethod
    def panorama_rays(width: int, height: int, eye, first_sample: int = 1):
        """The rays and keys of panorama(): (width * height RAY_DTYPE records, as many PATH_KEY_DTYPE records), row-major."""
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError("width and height must be at least 1")
        u, v = np.meshgrid(np.arange(width, dtype=np.float32), np.arange(height, dtype=np.float32))
        pi = np.float32(np.pi)
        phi = ((u + np.float32(0.5)) / np.float32(width) * np.float32(2.0) - np.float32(1.0)) * pi
        theta = (v + np.float32(0.5)) / np.float32(height) * pi
        st = np.sin(theta, dtype=np.float32)
        d = np.stack([st * np.sin(phi, dtype=np.float32), np.cos(theta, dtype=np.float32), st * np.cos(phi, dtype=np.float32)], axis=-1)
        d = (d / np.sqrt((d * d).sum(axis=-1, dtype=np.float32), dtype=np.float32)[..., None]).astype(np.float32).reshape(-1, 3)
        o = np.broadcast_to(np.asarray(eye, np.float32).reshape(1, 3), d.shape)
        return pack_rays(o, d), pack_keys(u.reshape(-1).astype(np.uint32), v.reshape(-1).astype(np.uint32), first_sample)

    def panorama(self, width: int, height: int, eye, n_samples: int, first_sample: int = 1):
        """An equirectangular (360 x 180 degree) image of the scene around `eye`: (xyz (H, W, 4) float32 sums over n_samples
        paths, rgba8 (H, W, 4) the tone-mapped mean), through radiance_rays.  The rays are made on the host in float32.
        Pixel (u, v), u = 0 .. width-1 from left to right, v = 0 .. height-1 from top to bottom, looks along
            phi = ((u + 0.5) / width * 2 - 1) * pi        (azimuth: 0 at the image's centre column, -pi at its left edge)
            theta = (v + 0.5) / height * pi                 (polar angle from +y: 0 at the top row's upper edge)
            d = normalize(sin(theta) sin(phi), cos(theta), sin(theta) cos(phi))
        so the centre looks along +z, the right half towards +x and the top towards +y.  Its key is (u, v, first_sample):
        its paths are seeded as samples first_sample .. first_sample + n_samples - 1 of pixel (u, v)."""
        rays, keys = self.panorama_rays(width, height, eye, first_sample)
        got = self.radiance_rays(rays=rays, keys=keys, n_samples=n_samples, planes=("xyz", "rgba8"))
        return got["xyz"].reshape(int(height), int(width), 4), got["rgba8"].reshape(int(height), int(width), 4)

    # -- multi-GPU: the frame across the ranks of a communicator (include/crt.h, "Multi-GPU")
    @staticmethod
    def comm_unique_id(local: bool = False) -> bytes:
        """128-byte communicator id: RCCL (one rank makes it, every rank gets it) or, local=True, the in-process transport."""
        lib = _lib.load()
        buf = C.create_string_buffer(128)
        rc = lib.crt_comm_unique_id(buf, 1 if local else 0)
        if rc != 0:
            raise CrtError(rc, (lib.crt_last_error(None) or b"").decode())
        return buf.raw

    def comm_init(self, comm_id: bytes, rank: int, world: int):
        if len(comm_id) != 128:
            raise ValueError("communicator id must be 128 bytes")
        self._chk(self._lib.crt_comm_init(self._h, C.create_string_buffer(comm_id, 128), int(rank), int(world)))
        return self

    def comm_partition(self, band_rows: int = 8):
        self._chk(self._lib.crt_comm_partition(self._h, int(band_rows)))
        return self

    def gather(self, rgba8: bool = True, accum: bool = False, preview: bool = False):
        """Post the gathers of this rank's strips.  preview=True (CRT_GATHER_PREVIEW) is a sync point and ships what
        read_frame_adaptive, denoise_frame and denoise_adaptive_frame need: the accumulator and, in the adaptive state,
        the second moments and the tile counts."""
        self._chk(self._lib.crt_gather(self._h, (1 if rgba8 else 0) | (2 if accum else 0) | (4 if preview else 0)))
        return self

    # -- the frame of a partition (include/crt.h, "The frame of a partition"): any rank, after gather(preview=True) on every rank
    def read_frame_adaptive(self):
        """read_adaptive of the whole frame: (counts, errors), each (ceil(H/8), ceil(W/8))."""
        W, H = self.image_size
        tx, ty = (W + 7) // 8, (H + 7) // 8
        counts = np.zeros((ty, tx), np.uint32)
        errors = np.zeros((ty, tx), np.float32)
        self._chk(self._lib.crt_read_frame_adaptive(self._h, counts.ctypes.data, errors.ctypes.data))
        return counts, errors

    def denoise_frame(self, iterations: int = 5, sigma_color: float = 1.0, sigma_normal: float = 0.5,
                      sigma_plane: float = 0.3, rgb: bool = False):
        """denoise of the gathered uniform frame, (H, W, ...) of the whole image: what one unpartitioned context returns."""
        return self._denoise(self._lib.crt_denoise_frame, _lib.DenoiseParams(), dict(
            iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_plane=sigma_plane), rgb,
            shape=self.image_size)

    def denoise_adaptive_frame(self, iterations: int | None = None, sigma_variance: float | None = None,
                               sigma_normal: float | None = None, sigma_plane: float | None = None, rgb: bool = False,
                               var: bool = False):
        """denoise_adaptive of the gathered adaptive frame, (H, W, ...) of the whole image; the same tuple."""
        return self._denoise(self._lib.crt_denoise_adaptive_frame, _lib.denoise_adaptive_defaults(), dict(
            iterations=iterations, sigma_variance=sigma_variance, sigma_normal=sigma_normal, sigma_plane=sigma_plane), rgb, bool(var),
            shape=self.image_size)

    @property
    def image_size(self):
        out = (C.c_uint32 * 2)()
        self._chk(self._lib.crt_image_size(self._h, out))
        return int(out[0]), int(out[1])

    def read_frame_rgba8(self) -> np.ndarray:
        W, H = self.image_size
        out = np.empty((H, W, 4), np.uint8)
        self._chk(self._lib.crt_read_frame_rgba8(self._h, out.ctypes.data))
        return out

    def read_frame_accum(self) -> np.ndarray:
        W, H = self.image_size
        out = np.empty((H, W, 4), np.float32)
        self._chk(self._lib.crt_read_frame_accum(self._h, out.ctypes.data))
        return out

    def frame_device_buffers(self):
        a, r = C.c_void_p(), C.c_void_p()
        self._chk(self._lib.crt_frame_device_buffers(self._h, C.byref(a), C.byref(r)))
        return a.value, r.value

    def comm_info(self) -> dict:
        out = (C.c_int * 4)()
        self._chk(self._lib.crt_comm_info(self._h, out))
        return dict(rank=out[0], world=out[1], transport={0: "rccl", 1: "local"}.get(out[2]), rows=out[3])

    def comm_destroy(self):
        self._chk(self._lib.crt_comm_destroy(self._h))
        return self

    # -- measurement
    def enable_counters(self, on: bool = True):
        self._chk(self._lib.crt_enable_counters(self._h, 1 if on else 0))
        return self

    def reset_counters(self):
        self._chk(self._lib.crt_reset_counters(self._h))
        return self

    def counters(self) -> dict:
        out = np.zeros(NCOUNTERS, np.uint64)
        self._chk(self._lib.crt_counters(self._h, out.ctypes.data))
        return {k: int(out[i]) for k, i in CNT.items()}

    def last_trace_ms(self):
        ms, n = C.c_float(), C.c_uint32()
        self._chk(self._lib.crt_last_trace_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_kernel_ms(self):
        ms, n = C.c_float(), C.c_uint32()
        self._chk(self._lib.crt_last_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def accel_stats(self) -> dict:
        out = np.zeros(8, np.uint64)
        self._chk(self._lib.crt_accel_stats(self._h, out.ctypes.data))
        return dict(nodes=int(out[0]), leaves=int(out[1]), max_depth=int(out[2]), bytes=int(out[3]),
                    bytes_per_box=int(out[4]), width=int(out[5]), wide_nodes=int(out[6]),
                    builder=("sah-host", "lbvh-gpu", "ploc-gpu")[int(out[7])])

    # -- test hooks
    def debug_intersect(self, origins, directions, exclude=None) -> np.ndarray:
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        d = np.asarray(directions, np.float32).reshape(-1, 3)
        n = o.shape[0]
        rays = np.zeros((n, 8), np.float32)
        rays[:, 0:3] = o
        rays[:, 3:6] = d
        ex = np.full(n, 0xFFFFFFFF, np.uint32) if exclude is None else np.asarray(exclude, np.uint32)
        rays[:, 6] = ex.view(np.float32)
        out = np.zeros((n, 8), np.float32)
        self._chk(self._lib.crt_debug_intersect(self._h, rays.ctypes.data, n, out.ctypes.data))
        return out

    TRACE_KERNELS = ("k_wf_trace<,0>", "k_wf_trace<,1>", "k_wf_trace<,2>", "k_wf_trace2")

    def debug_trace_rays(self, origins, directions, exclude=None, shadow=None, t_light=None, light=None):
        """Rays through the traversal kernel frame() launches for the current tree and options (crt_debug_trace_rays).
        shadow: bool mask of the shadow rays, which take t_light / light (the light primitive's own t and index).
        Returns (t float32 (n,), index uint32 (n,) -- 0xFFFFFFFF = miss --, visible uint32 (n,), report dict); t and
        index hold zeros / the visibility bit at shadow rays, visible is 0 at extension rays."""
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        d = np.asarray(directions, np.float32).reshape(-1, 3)
        n = o.shape[0]
        rays = np.zeros((n, 12), np.float32)
        rays[:, 0:3] = o
        rays[:, 3:6] = d
        ru = rays.view(np.uint32)
        ru[:, 6] = 0xFFFFFFFF if exclude is None else np.asarray(exclude, np.uint32)
        sh = np.zeros(n, bool) if shadow is None else np.asarray(shadow, bool)
        if sh.any():
            ru[:, 7] = sh
            rays[sh, 8] = np.asarray(t_light, np.float32)[sh]
            ru[sh, 9] = np.asarray(light, np.uint32)[sh]
        out = np.zeros((n, 2), np.uint32)
        rep = np.zeros(8, np.uint64)
        self._chk(self._lib.crt_debug_trace_rays(self._h, rays.ctypes.data, n, out.ctypes.data, rep.ctypes.data))
        report = dict(width=int(rep[0]), depth=int(rep[1]), lds_entries=int(rep[2]), overflow_levels=int(rep[3]),
                      capacity=int(rep[4]), deepest=int(rep[5]), kernel=self.TRACE_KERNELS[int(rep[6])], counting=bool(rep[7]))
        t = np.where(sh, np.uint32(0), out[:, 0]).astype(np.uint32).view(np.float32)
        return t, np.where(sh, np.uint32(0), out[:, 1]).astype(np.uint32), np.where(sh, out[:, 0], np.uint32(0)).astype(np.uint32), report

    WALKS = {"finish": 0, "bvh2": 1}

    def debug_walk_rays(self, origins, directions, exclude=None, shadow=None, t_light=None, light=None, walk="finish"):
        """Rays through the single-ray walks (crt_debug_walk_rays): walk="finish" as k_wf_finish calls them (the quantised
        4-wide tree where it is live, the BVH2 on overflow), walk="bvh2" as the pipeline = 0 kernel does (a shadow ray
        tests its light's primitive itself).  Arguments as debug_trace_rays.  Returns (t, index, visible, flags uint32
        (n,) -- bit 0: walked the 4-wide tree, bit 1: fell back --, t_light float32 (n,) -- what the kernel computed,
        walk="bvh2" shadow rays only --, report dict)."""
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        d = np.asarray(directions, np.float32).reshape(-1, 3)
        n = o.shape[0]
        rays = np.zeros((n, 12), np.float32)
        rays[:, 0:3] = o
        rays[:, 3:6] = d
        ru = rays.view(np.uint32)
        ru[:, 6] = 0xFFFFFFFF if exclude is None else np.asarray(exclude, np.uint32)
        sh = np.zeros(n, bool) if shadow is None else np.asarray(shadow, bool)
        if sh.any():
            ru[:, 7] = sh
            rays[sh, 8] = np.asarray(t_light, np.float32)[sh]
            ru[sh, 9] = np.asarray(light, np.uint32)[sh]
        out = np.zeros((n, 4), np.uint32)
        rep = np.zeros(8, np.uint64)
        self._chk(self._lib.crt_debug_walk_rays(self._h, self.WALKS[walk], rays.ctypes.data, n, out.ctypes.data, rep.ctypes.data))
        report = dict(walked_wide=int(rep[0]), fell_back=int(rep[1]), stack_entries=int(rep[2]), depth4=int(rep[3]), depth2=int(rep[4]),
                      wide=bool(rep[5]))
        t = np.where(sh, np.uint32(0), out[:, 0]).astype(np.uint32).view(np.float32)
        return (t, np.where(sh, np.uint32(0), out[:, 1]).astype(np.uint32), np.where(sh, out[:, 0], np.uint32(0)).astype(np.uint32),
                out[:, 2].copy(), out[:, 3].copy().view(np.float32), report)

    ACCEL_HEADER = ("accel_mode", "builder", "nprim", "root", "root4", "root8", "n2", "n4", "n8", "live4", "live4q", "live8q",
                    "qbase_x", "qbase_y", "qbase_z", "qscale_x", "qscale_y", "qscale_z", "hit_pad", "tree_pad", "depth2", "depth4",
                    "depth8", "wf_depth", "wf_stack_need", "wf_stack_lds", "wf_overflow_levels", "overflow_allocated", "stale",
                    "device_route")
    ACCEL_PARTS = (("nodes2", np.float32, 16), ("nodes4", np.float32, 32), ("nodes4q", np.uint32, 16), ("nodes8q", np.uint32, 32),
                   ("prim", np.float32, 12), ("primD", np.float32, 4), ("slot_of_index", np.uint32, 1))

    def debug_read_accel(self) -> dict:
        """The current acceleration structure as it lies on the device (crt_debug_read_accel): the header's scalars by
        name (ints; qbase / qscale / hit_pad / tree_pad as float32) and the arrays, one row per node / slot (empty where
        the part is not live).  Works on a stale tree; reads only."""
        def part(what, dtype):
            nbytes = C.c_size_t()
            self._chk(self._lib.crt_debug_read_accel(self._h, what, None, 0, C.byref(nbytes)))
            out = np.zeros(nbytes.value // np.dtype(dtype).itemsize, dtype)
            if nbytes.value:
                self._chk(self._lib.crt_debug_read_accel(self._h, what, out.ctypes.data, out.nbytes, None))
            return out
        h = part(0, np.float64)
        floats = ("qbase_x", "qbase_y", "qbase_z", "qscale_x", "qscale_y", "qscale_z", "hit_pad", "tree_pad")   # (a pad may be inf)
        out = {k: int(v) for k, v in zip(self.ACCEL_HEADER, h) if k not in floats}
        out["qbase"], out["qscale"] = h[12:15].astype(np.float32), h[15:18].astype(np.float32)
        out["hit_pad"], out["tree_pad"] = np.float32(h[18]), np.float32(h[19])
        for what, (name, dtype, cols) in enumerate(self.ACCEL_PARTS, 1):
            a = part(what, dtype)
            out[name] = a.reshape(-1, cols) if cols > 1 else a
        return out

    def debug_probes(self) -> list:
        out = np.zeros(8, np.uint64)
        self._chk(self._lib.crt_debug_probes(self._h, out.ctypes.data))
        return [int(v) for v in out]

    def gen_culled(self) -> int:
        """(pixel, sample) pairs the generate kernel decided itself since reset_counters() (crt_debug_gen_culled):
        camera rays that miss the tree's root boxes, by whole 8x8 tiles of one sample.  A sync point."""
        n = C.c_uint64()
        self._chk(self._lib.crt_debug_gen_culled(self._h, C.byref(n)))
        return int(n.value)

    def deferred_nee(self) -> int:
        """Paths the shade kernel finished at once since reset_counters() (crt_debug_deferred_nee): roulette ended them
        while their NEE shadow ray was pending, and the term was added one iteration later (option "wf_defer_nee").
        A sync point."""
        n = C.c_uint64()
        self._chk(self._lib.crt_debug_deferred_nee(self._h, C.byref(n)))
        return int(n.value)

    def tile_classes(self, host: bool = False) -> np.ndarray:
        """The class of every 8x8 tile of the tile rectangle, (tiles_y, tiles_x) uint8: 1 = its camera rays miss the
        tree's root boxes for every sample, 2 = they all enter one, 0 = it depends on the sample (option
        "wf_cull_classes").  From the device kernel (crt_debug_tile_classes) or, with host=True, from the same definition
        evaluated on the CPU (crt_debug_tile_classes_host).  A sync point."""
        t = np.zeros(4, np.uint32)
        self._chk(self._lib.crt_tile(self._h, t.ctypes.data))
        ty, tx = (int(t[3]) + 7) // 8, (int(t[2]) + 7) // 8
        out = np.zeros((ty, tx), np.uint8)
        fn = self._lib.crt_debug_tile_classes_host if host else self._lib.crt_debug_tile_classes
        self._chk(fn(self._h, out.ctypes.data, out.size))
        return out

    def tile_class_setups(self) -> int:
        """Run set-ups of this context that launched the tile classifier so far (crt_debug_tile_class_setups)."""
        n = C.c_uint64()
        self._chk(self._lib.crt_debug_tile_class_setups(self._h, C.byref(n)))
        return int(n.value)

    def mapped_gen_launches(self) -> int:
        """Generate launches of this context that handed out region-major work so far (option "wf_affinity",
        crt_debug_mapped_gen_launches)."""
        n = C.c_uint64()
        self._chk(self._lib.crt_debug_mapped_gen_launches(self._h, C.byref(n)))
        return int(n.value)

    def debug_math(self, fn: int, a, b=None) -> np.ndarray:
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b if b is not None else np.zeros_like(a), np.float32)
        out = np.empty_like(a)
        self._chk(self._lib.crt_debug_math(self._h, int(fn), a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size))
        return out

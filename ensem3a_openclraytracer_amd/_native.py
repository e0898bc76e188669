"""ctypes binding of the native library ``lib/libensem3a_rt.so`` (include/rt_api.h).

There is no fallback: if the library is missing or fails to load, every entry
point raises.  The library is built in-tree by ``_build.build()``.
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np

from ._build import LIB

_lock = threading.Lock()
_lib = None
_host = None

RT_TRAVERSAL_FAST = 0
RT_TRAVERSAL_REF = 1
RT_BVH_REFERENCE = 0
RT_BVH_SAH = 1
RT_ERR_ARG = 1
RT_ERR_STATE = 3
RT_ACCUM_MAX_SAMPLES = 1 << 24   # rt_api.h: the most samples per pixel an accumulation may reach
SPEC_PICK = 10   # rt_debug.h RT_SPEC_PICK (rt_internal.h kSpecPick): a pass-2 pick word above it means trails
PILOT_FIELDS = ("two_pass", "nloc", "pilot", "chunk", "levels", "lanes", "left", "pick")   # rt_debug_last_pilot

# Every symbol of include/rt_api.h and include/rt_debug.h (checked by tests).
EXPORTED = (
    "rt_create", "rt_destroy", "rt_last_error", "rt_set_scene", "rt_set_env", "rt_set_option",
    "rt_render", "rt_render_device", "rt_tile_rows", "rt_count_work", "rt_count_work_detail", "rt_work_bytes", "rt_gamma",
    "rt_render_rgb8", "rt_rgb8_device", "rt_rgb8",
    "rt_accum_begin", "rt_accum_add", "rt_accum_add_rgb8", "rt_accum_read", "rt_accum_samples", "rt_accum_end",
    "rt_accum_begin_device", "rt_accum_add_device",
    "rt_accum_mark", "rt_accum_select", "rt_accum_select_mask", "rt_accum_select_all", "rt_accum_selection",
    "rt_accum_sample_map", "rt_accum_add_selected", "rt_accum_mark_device", "rt_accum_select_device",
    "rt_accum_select_mask_device", "rt_accum_select_all_device", "rt_accum_add_selected_device",
    "rt_accum_guides", "rt_accum_guides_device", "rt_denoise_device", "rt_accum_denoise", "rt_denoise",
    "rt_reproject_basis", "rt_reproject_device", "rt_accum_reproject",
    "rt_trace", "rt_trace_device",
    "rt_radiance", "rt_radiance_device", "rt_camera_rays", "rt_camera_rays_device",
    "rt_lens_radiance", "rt_lens_radiance_device", "rt_lens_rays", "rt_lens_rays_device", "rt_radiance_resolve_device",
    "rt_accum_begin_lens", "rt_accum_begin_lens_device", "rt_debug_accum_state",
    "rt_bvh_build", "rt_device_count", "rt_debug_math", "rt_debug_fn", "rt_debug_trace", "rt_debug_trace_clustered", "rt_debug_scene_info", "rt_debug_pixel_log",
    "rt_debug_wave_counts", "rt_debug_quantise_axis", "rt_debug_timings", "rt_debug_brute_layout",
    "rt_debug_brute_clusters", "rt_debug_brute_shell", "rt_debug_brute_near", "rt_debug_brute_quad",
    "rt_debug_brute_direct", "rt_debug_last_direct", "rt_debug_shell_word",
    "rt_debug_brute_slices",
    "rt_debug_last_slices",
    "rt_debug_brute_refill", "rt_debug_last_refill", "rt_debug_last_launch", "rt_debug_brute_lean",
    "rt_debug_pilot_order", "rt_debug_pilot_pick", "rt_debug_last_pilot",
    "rt_obj_parse", "rt_obj_size", "rt_obj_copy", "rt_obj_free", "rt_obj_last_error",
    "rt_scene_check", "rt_scene_last_error",
)
# The host-only entry points (no GPU, no HIP call): the sanitizer build (oracle/Makefile asan,
# tools/sanitize.sh) compiles exactly these into an ASan/UBSan library that ENSEM3A_HOST_LIB selects.
HOST_ONLY = ("rt_bvh_build", "rt_obj_parse", "rt_obj_size", "rt_obj_copy", "rt_obj_free", "rt_obj_last_error",
             "rt_scene_check", "rt_scene_last_error", "rt_debug_quantise_axis", "rt_debug_brute_layout",
             "rt_debug_brute_clusters", "rt_debug_brute_shell", "rt_debug_brute_near", "rt_debug_brute_quad",
             "rt_reproject_basis")

_c_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int


class DenoiseParams(ctypes.Structure):
    """rt_denoise_params of rt_api.h; the defaults are the library's."""
    _fields_ = [("passes", ctypes.c_int), ("normal_squarings", ctypes.c_int),
                ("sigma_c", ctypes.c_float), ("sigma_p", ctypes.c_float)]

    def __init__(self, passes: int = 5, normal_squarings: int = 5, sigma_c: float = 1.5, sigma_p: float = 0.02):
        super().__init__(int(passes), int(normal_squarings), float(sigma_c), float(sigma_p))


class ReprojectParams(ctypes.Structure):
    """rt_reproject_params of rt_api.h; the defaults are the library's."""
    _fields_ = [("sigma_p", ctypes.c_float), ("normal_min", ctypes.c_float), ("max_history", ctypes.c_float),
                ("min_weight", ctypes.c_float)]

    def __init__(self, sigma_p: float = 0.02, normal_min: float = 0.9, max_history: float = 64.0,
                 min_weight: float = 0.25):
        super().__init__(float(sigma_p), float(normal_min), float(max_history), float(min_weight))


GUIDE_FLOATS = 12   # three float4 per pixel: n | k, P | f, a | m (rt_api.h)

# Ray queries (rt_trace*, rt_api.h): rt_hit, and a ray's eight floats dir.xyz, origin.xyz, tmax, reserved
HIT_DTYPE = np.dtype([("k", np.float32), ("tri", np.int32), ("u", np.float32), ("v", np.float32)])
RAY_FLOATS = 8
RT_QUERY_CLOSEST = 0
RT_QUERY_ANY = 1
QUERY_HORIZON = 1000.0   # the reference's horizon: a hit has k < min(tmax, 1000)


def pack_rays(origins, directions, tmax=None) -> np.ndarray:
    """float32 ``[n, 8]`` rays of rt_trace from ``[n, 3]`` origins and directions: ``dir, origin, tmax, 0``.
    ``tmax`` is a scalar or ``[n]``; None packs the horizon, 1000."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError(f"{len(o)} origins but {len(d)} directions")
    rays = np.zeros((len(o), RAY_FLOATS), np.float32)
    rays[:, 0:3] = d
    rays[:, 3:6] = o
    rays[:, 6] = QUERY_HORIZON if tmax is None else np.asarray(tmax, dtype=np.float32)
    return rays


# Radiance queries (rt_radiance*, rt_api.h): rt_radiance_state, and a ray's eight words dir.xyz, origin.xyz, seed0,
# seed1 (the seeds' uint bits where rt_trace has tmax and reserved)
RADIANCE_STATE_DTYPE = np.dtype([("sum", np.float32, (3,)), ("k", np.float32), ("seed0", np.uint32),
                                 ("seed1", np.uint32), ("tri", np.int32), ("n", np.int32)])
RT_RADIANCE_RESUME = 1
RT_ACCUM_MAX_SAMPLES = 1 << 24


class Lens(ctypes.Structure):
    """rt_lens of rt_api.h: the box filter's width in pixels, the lens's radius, the distance of the plane in focus
    and the seed of the sample rays' uniforms."""
    _fields_ = [("jitter", ctypes.c_float), ("aperture", ctypes.c_float), ("focus", ctypes.c_float),
                ("seed", ctypes.c_uint32)]

    def __init__(self, jitter: float = 1.0, aperture: float = 0.0, focus: float = 1.0, seed: int = 0):
        super().__init__(float(jitter), float(aperture), float(focus), int(seed) & 0xffffffff)


def pack_radiance_rays(origins, directions, seeds=None) -> np.ndarray:
    """float32 ``[n, 8]`` rays of rt_radiance from ``[n, 3]`` origins and directions: ``dir, origin``, then the bits
    of ``seeds`` (uint32 ``[n, 2]``; None: ``(ray index, 0)``, the decorrelation a frame gives its pixels)."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError(f"{len(o)} origins but {len(d)} directions")
    rays = np.zeros((len(o), RAY_FLOATS), np.float32)
    rays[:, 0:3] = d
    rays[:, 3:6] = o
    words = rays.view(np.uint32)
    if seeds is None:
        words[:, 6] = np.arange(len(o), dtype=np.uint32)
    else:
        sd = np.asarray(seeds)
        if sd.dtype.kind not in "iu":
            raise TypeError(f"seeds must be integers, got {sd.dtype}")
        if sd.shape != (len(o), 2):
            raise ValueError(f"seeds must be [{len(o)}, 2], got {list(sd.shape)}")
        words[:, 6:8] = sd.astype(np.uint32)
    return rays


class NativeError(RuntimeError):
    """A non-zero status from the native library (mirrors pyopencl raising)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"[rt status {status}] {message}")
        self.status = status


def _preload_hip_runtime() -> None:
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for d in (spec.submodule_search_locations or []) if spec else []:
        p = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(p):
            ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)
            return


def lib():
    """Load (once) and return the native library; raise loudly when absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        # torch ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7, the
        # same SONAME as ROCm's): whichever is loaded first serves the whole process, and torch
        # cannot initialise its GPUs on ROCm's.  So when torch is installed its runtime is loaded
        # first -- as a plain shared library, without importing torch: the single-GPU drop-in path
        # (KernelLauncher) needs no torch, and a torch imported later finds its own runtime
        # already loaded (tests/test_gpu_boundary.py).
        _preload_hip_runtime()
        lib_path = os.environ.get("ENSEM3A_RT_LIB", LIB)  # experimental variants (tools/variants.py)
        if not os.path.exists(lib_path):
            raise RuntimeError(
                f"native library {lib_path} is missing: build it with "
                "`python -m ensem3a_openclraytracer_amd._build` (there is no CPU fallback)")
        L = ctypes.CDLL(lib_path)
        sig = {
            "rt_create": (_i32, [_i32, _c_p, ctypes.POINTER(_c_p)]),
            "rt_destroy": (None, [_c_p]),
            "rt_last_error": (ctypes.c_char_p, [_c_p]),
            "rt_set_scene": (_i32, [_c_p, _c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64]),
            "rt_set_env": (_i32, [_c_p, _c_p, _i32, _i32]),
            "rt_set_option": (_i32, [_c_p, ctypes.c_char_p, _i64]),
            "rt_render": (_i32, [_c_p, _c_p, _c_p, _i64, _i32, _i32, _c_p]),
            "rt_render_device": (_i32, [_c_p, _i32, _c_p, _c_p, _i64, _i32, _i32, _i32, _i32, _c_p, _c_p]),
            "rt_tile_rows": (_i64, [_i64, _i32, _i32, _i32]),
            "rt_count_work": (_i32, [_c_p, _c_p, _c_p, _i64, _i32, _i32, _i32, _i32, _c_p]),
            "rt_count_work_detail": (_i32, [_c_p, _c_p, _c_p, _i64, _i32, _i32, _i32, _i32, _c_p]),
            "rt_work_bytes": (_i32, [_c_p, _c_p]),
            "rt_gamma": (_i32, [_c_p, _c_p, _c_p, _i64]),
            "rt_render_rgb8": (_i32, [_c_p, _c_p, _c_p, _i64, _i32, _i32, _i32, _c_p]),
            "rt_rgb8_device": (_i32, [_c_p, _i32, _c_p, _c_p, _i64, _i32, _c_p]),
            "rt_rgb8": (_i32, [_c_p, _c_p, _c_p, _i64, _i32]),
            "rt_accum_begin": (_i32, [_c_p, _c_p, _c_p, _i64, _i32]),
            "rt_accum_add": (_i32, [_c_p, _i32, _c_p]),
            "rt_accum_add_rgb8": (_i32, [_c_p, _i32, _i32, _c_p]),
            "rt_accum_read": (_i32, [_c_p, _c_p]),
            "rt_accum_samples": (_i64, [_c_p]),
            "rt_accum_end": (_i32, [_c_p]),
            "rt_accum_begin_device": (_i32, [_c_p, _i32, _c_p, _c_p, _i64, _i32, _i32, _i32]),
            "rt_accum_add_device": (_i32, [_c_p, _i32, _i32, _c_p, _c_p]),
            "rt_accum_mark": (_i32, [_c_p]),
            "rt_accum_select": (_i32, [_c_p, ctypes.c_float, ctypes.POINTER(_i64)]),
            "rt_accum_select_mask": (_i32, [_c_p, _c_p]),
            "rt_accum_select_all": (_i32, [_c_p]),
            "rt_accum_selection": (_i32, [_c_p, _c_p]),
            "rt_accum_sample_map": (_i32, [_c_p, _c_p]),
            "rt_accum_add_selected": (_i32, [_c_p, _i32, _c_p]),
            "rt_accum_mark_device": (_i32, [_c_p, _i32, _c_p]),
            "rt_accum_select_device": (_i32, [_c_p, _i32, ctypes.c_float, _c_p]),
            "rt_accum_select_mask_device": (_i32, [_c_p, _i32, _c_p, _c_p]),
            "rt_accum_select_all_device": (_i32, [_c_p, _i32, _c_p]),
            "rt_accum_add_selected_device": (_i32, [_c_p, _i32, _i32, _c_p, _c_p]),
            "rt_accum_guides": (_i32, [_c_p, _c_p]),
            "rt_accum_guides_device": (_i32, [_c_p, _i32, _c_p, _c_p]),
            "rt_denoise_device": (_i32, [_c_p, _i32, _c_p, _c_p, _i64, _i32, ctypes.POINTER(DenoiseParams), _c_p, _c_p]),
            "rt_accum_denoise": (_i32, [_c_p, ctypes.POINTER(DenoiseParams), _c_p]),
            "rt_denoise": (_i32, [_c_p, _c_p, _c_p, _i64, _i32, ctypes.POINTER(DenoiseParams), _c_p]),
            "rt_reproject_basis": (_i32, [_c_p, _c_p]),
            "rt_reproject_device": (_i32, [_c_p, _i32, _c_p, _c_p, _c_p, _c_p, _c_p, _i64, _i32,
                                           ctypes.POINTER(ReprojectParams), _c_p, _c_p, _c_p]),
            "rt_accum_reproject": (_i32, [_c_p, _c_p, _c_p, _c_p, ctypes.POINTER(ReprojectParams), _c_p, _c_p]),
            "rt_trace": (_i32, [_c_p, _c_p, _i64, _i32, _c_p]),
            "rt_trace_device": (_i32, [_c_p, _i32, _c_p, _i64, _i32, _c_p, _c_p]),
            "rt_radiance": (_i32, [_c_p, _c_p, _i64, _c_p, _i32, _i32, _i32, _c_p]),
            "rt_radiance_device": (_i32, [_c_p, _i32, _c_p, _i64, _c_p, _i32, _i32, _i32, _c_p, _c_p]),
            "rt_camera_rays": (_i32, [_c_p, _c_p, _i64, _i64, _i64, _c_p]),
            "rt_camera_rays_device": (_i32, [_c_p, _i32, _c_p, _i64, _i64, _i64, _c_p, _c_p]),
            "rt_lens_radiance": (_i32, [_c_p, _c_p, _c_p, _c_p, _i64, _i64, _i64, _i32, _i32, _i32, _c_p]),
            "rt_lens_radiance_device": (_i32, [_c_p, _i32, _c_p, _c_p, _c_p, _i64, _i64, _i64, _i32, _i32, _i32, _c_p,
                                               _c_p]),
            "rt_lens_rays": (_i32, [_c_p, _c_p, _c_p, _i64, _i64, _i64, _i32, _i32, _c_p]),
            "rt_lens_rays_device": (_i32, [_c_p, _i32, _c_p, _c_p, _i64, _i64, _i64, _i32, _i32, _c_p, _c_p]),
            "rt_radiance_resolve_device": (_i32, [_c_p, _i32, _c_p, _i64, _c_p, _c_p]),
            "rt_accum_begin_lens": (_i32, [_c_p, _c_p, _c_p, _c_p, _i64, _i32]),
            "rt_accum_begin_lens_device": (_i32, [_c_p, _i32, _c_p, _c_p, _c_p, _i64, _i32, _i32, _i32]),
            "rt_debug_accum_state": (_i32, [_c_p, _c_p]),
            "rt_bvh_build": (_i32, [_c_p, _i64, _c_p, _i64, _c_p, ctypes.POINTER(_i64)]),
            "rt_device_count": (_i32, []),
            "rt_obj_parse": (_i32, [_c_p, _i64, ctypes.POINTER(_c_p)]),
            "rt_obj_size": (_i64, [_c_p, _i32]),
            "rt_obj_copy": (_i32, [_c_p, _c_p, _c_p, _c_p, _c_p]),
            "rt_obj_free": (None, [_c_p]),
            "rt_obj_last_error": (ctypes.c_char_p, []),
            "rt_scene_check": (_i32, [_c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _i32, _c_p]),
            "rt_scene_last_error": (ctypes.c_char_p, []),
            "rt_debug_brute_layout": (_i32, [_c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _i32, _c_p, _i64,
                                             _c_p]),
            "rt_debug_brute_clusters": (_i32, [_c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _i32, _i32,
                                               _c_p, _i64, _c_p, _i64, _c_p]),
            "rt_debug_brute_shell": (_i32, [_c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _i32, _i32, _i32,
                                            _c_p, _i64, _c_p]),
            "rt_debug_brute_near": (_i32, [_c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _i32, _i32, _i32,
                                           _c_p, _i64, _c_p, _c_p]),
            "rt_debug_brute_quad": (_i32, [_c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _i32, _i32, _i32,
                                           _i32, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
            "rt_debug_brute_slices": (_i32, [_i64, _i64, _i32, _i32, _i32, _c_p]),
            "rt_debug_last_slices": (_i32, []),
            "rt_debug_brute_refill": (_i32, [_i64, _i64, _i32, _c_p]),
            "rt_debug_last_refill": (_i32, [_c_p]),
            "rt_debug_last_launch": (_i32, [_c_p]),
            "rt_debug_pilot_order": (_i32, [_c_p, _c_p, _i64, _i32, _i32, _i32, _i32, _c_p]),
            "rt_debug_pilot_pick": (_i32, [_c_p, _c_p, _i64, _i64, _i32, _c_p]),
            "rt_debug_last_pilot": (_i32, [_c_p, _c_p, _c_p, _c_p, _i64]),
            "rt_debug_math": (_i32, [_c_p, _i32, _c_p, _c_p, _c_p, _i64]),
            "rt_debug_fn": (_i32, [_c_p, _i32, _c_p, _c_p, _i64]),
            "rt_debug_trace": (_i32, [_c_p, _i32, _c_p, _c_p, _i64]),
            "rt_debug_trace_clustered": (_i32, [_c_p, _c_p, _c_p, _i64, _c_p]),
            "rt_debug_scene_info": (_i32, [_c_p, _c_p]),
            "rt_debug_timings": (_i32, [_c_p, _c_p]),
            "rt_debug_wave_counts": (_i32, [_c_p, _c_p, _c_p, _i64, _i32, _i32, _c_p]),
            "rt_debug_pixel_log": (_i32, [_c_p, _i32, _c_p, _c_p, _i64, _i32, _i32, _i64, _c_p, _i32, _c_p, _c_p]),
        }
        _bind(L, sig)
        _lib = L
    return _lib


_HOST_SIG = {}


def _bind(L, sig, names=None):
    for name, (res, args) in sig.items():
        if names is not None and name not in names:
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
        if name in HOST_ONLY:
            _HOST_SIG[name] = (res, args)


def host_lib():
    """The library serving the host-only entry points (HOST_ONLY): the product library, or the
    sanitizer build named by ENSEM3A_HOST_LIB (tools/sanitize.sh)."""
    global _host
    if _host is not None:
        return _host
    L = lib()
    path = os.environ.get("ENSEM3A_HOST_LIB")
    if path:
        with _lock:
            if _host is None:
                H = ctypes.CDLL(path)
                _bind(H, _HOST_SIG)
                _host = H
        return _host
    _host = L
    return _host


def check(status: int, ctx=None) -> None:
    if status != 0:
        msg = lib().rt_last_error(ctx)
        raise NativeError(status, msg.decode(errors="replace") if msg else "unknown error")


def f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def ptr(a: np.ndarray):
    return a.ctypes.data if a is not None and a.size else None


def reproject_basis(cam) -> np.ndarray:
    """rt_reproject_basis: the 16 floats the reprojection kernel takes of a camera (host only, no GPU)."""
    c = f32(cam).reshape(-1)
    if c.size != 10:
        raise ValueError("cam must have 10 floats")
    out = np.zeros(16, np.float32)
    st = host_lib().rt_reproject_basis(ptr(c), out.ctypes.data)
    if st != 0:
        raise NativeError(st, "rt_reproject_basis: cam must be finite")
    return out


def device_count() -> int:
    return int(lib().rt_device_count())


class Context:
    """Owner of one ``rt_ctx`` (one per host thread)."""

    def __init__(self, n_devices: int = 1, device_ids=None):
        ids = None
        if device_ids is not None:
            ids = (ctypes.c_int * len(device_ids))(*device_ids)
            n_devices = len(device_ids)
        out = _c_p()
        check(lib().rt_create(int(n_devices), ids, ctypes.byref(out)))
        self._ctx = out
        self.n_devices = int(n_devices)

    @property
    def handle(self):
        if self._ctx is None:
            raise RuntimeError("context destroyed")
        return self._ctx

    def close(self) -> None:
        if getattr(self, "_ctx", None) is not None:
            lib().rt_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int) -> None:
        check(st, self.handle)

    def set_option(self, key: str, value: int) -> None:
        self._check(lib().rt_set_option(self.handle, key.encode(), int(value)))

    def set_scene(self, V_p, V_n, V_uv, faceData, materialData, bvh) -> None:
        vp, vn, vuv = f32(V_p), f32(V_n), f32(V_uv if V_uv is not None else np.zeros(0, np.float32))
        face, mat, bv = i32(faceData), f32(materialData), f32(bvh)
        self._check(lib().rt_set_scene(self.handle, ptr(vp), vp.size, ptr(vn), vn.size, ptr(vuv), vuv.size,
                                       ptr(face), face.size, ptr(mat), mat.size, ptr(bv), bv.size))

    def set_env(self, rgba: np.ndarray) -> None:
        img = np.ascontiguousarray(rgba, dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 4:
            raise ValueError(f"IBL must be an HxWx4 RGBA8 array, got shape {img.shape}")
        self._check(lib().rt_set_env(self.handle, ptr(img), img.shape[1], img.shape[0]))

    def render(self, cam, env, npix: int, spp: int, max_bounce: int, out: np.ndarray = None) -> np.ndarray:
        c, e = f32(cam), f32(env)
        if c.size != 10 or e.size != 5:
            raise ValueError("cam must have 10 floats and envData 5")
        if out is None:
            out = np.zeros(3 * int(npix), dtype=np.float32)
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.size < 3 * int(npix):
            raise ValueError("output must be a contiguous float32 array of 3*imgDim elements")
        self._check(lib().rt_render(self.handle, ptr(c), ptr(e), int(npix), int(spp), int(max_bounce),
                                    out.ctypes.data))
        return out

    def render_device(self, cam, env, npix, spp, max_bounce, row0, row_step, d_out_ptr: int, stream_ptr: int = 0,
                      device_index: int = 0) -> None:
        c, e = f32(cam), f32(env)
        self._check(lib().rt_render_device(self.handle, int(device_index), ptr(c), ptr(e), int(npix), int(spp),
                                           int(max_bounce), int(row0), int(row_step), _c_p(int(d_out_ptr)),
                                           _c_p(int(stream_ptr)) if stream_ptr else None))  # 0 = default stream

    def count_work(self, cam, env, npix, spp, max_bounce, row0=0, row_step=1):
        c, e = f32(cam), f32(env)
        out = np.zeros(5, dtype=np.uint64)
        self._check(lib().rt_count_work(self.handle, ptr(c), ptr(e), int(npix), int(spp), int(max_bounce),
                                        int(row0), int(row_step), out.ctypes.data))
        return dict(zip(("node_fetches", "tri_tests", "rays", "env_lookups", "stack_drops"), map(int, out)))

    COUNT_KEYS = ("node_fetches", "tri_tests", "rays", "env_lookups", "stack_drops", "wave_trav_iters",
                  "wave_render_iters", "cycles_shade", "cycles_trav", "box_tests", "ev_diffuse", "ev_glossy",
                  "ev_glass", "sun_terms", "samples", "refill_events")

    def count_work_detail(self, cam, env, npix, spp, max_bounce, row0=0, row_step=1):
        """rt_count_work_detail: every work counter of the instrumented render of the tile."""
        c, e = f32(cam), f32(env)
        out = np.zeros(16, dtype=np.uint64)
        self._check(lib().rt_count_work_detail(self.handle, ptr(c), ptr(e), int(npix), int(spp), int(max_bounce),
                                               int(row0), int(row_step), out.ctypes.data))
        return {k: int(v) for k, v in zip(self.COUNT_KEYS, out)}

    def work_bytes(self):
        out = np.zeros(4, dtype=np.float64)
        self._check(lib().rt_work_bytes(self.handle, out.ctypes.data))
        return dict(zip(("box_test", "tri_test", "ray", "env_lookup"), map(float, out)))

    def gamma(self, src, out=None):
        s = f32(src)
        if out is None:
            out = np.zeros_like(s)
        self._check(lib().rt_gamma(self.handle, ptr(s), out.ctypes.data, s.size))
        return out

    def render_rgb8(self, cam, env, npix: int, spp: int, max_bounce: int, gamma: bool = False,
                    out: np.ndarray = None) -> np.ndarray:
        """Render and quantize on the device: uint8[3*npix] = (frame*255).astype(uint8) (gamma first if asked)."""
        c, e = f32(cam), f32(env)
        if c.size != 10 or e.size != 5:
            raise ValueError("cam must have 10 floats and envData 5")
        if out is None:
            out = np.zeros(3 * int(npix), dtype=np.uint8)
        if out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < 3 * int(npix):
            raise ValueError("output must be a contiguous uint8 array of 3*imgDim elements")
        self._check(lib().rt_render_rgb8(self.handle, ptr(c), ptr(e), int(npix), int(spp), int(max_bounce),
                                         int(bool(gamma)), out.ctypes.data))
        return out

    # -- progressive accumulation (rt_accum_*): adds of a then b samples give the one-shot frame at a + b --
    def accum_begin(self, cam, env, npix: int, max_bounce: int) -> None:
        c, e = f32(cam), f32(env)
        if c.size != 10 or e.size != 5:
            raise ValueError("cam must have 10 floats and envData 5")
        self._check(lib().rt_accum_begin(self.handle, ptr(c), ptr(e), int(npix), int(max_bounce)))
        self._accum_npix = int(npix)

    def _accum_out(self, out, dtype) -> np.ndarray:
        n = 3 * getattr(self, "_accum_npix", 0)
        if out is None:
            return np.zeros(n, dtype=dtype)
        if not isinstance(out, np.ndarray) or out.dtype != dtype or not out.flags.c_contiguous or out.size < n:
            raise ValueError(f"output must be a contiguous {np.dtype(dtype).name} array of 3*imgDim elements")
        return out

    def accum_add(self, spp: int, out: np.ndarray = None) -> np.ndarray:
        """``spp`` more samples of every pixel; returns the frame at the samples done (float32[3*npix])."""
        out = self._accum_out(out, np.float32)
        self._check(lib().rt_accum_add(self.handle, int(spp), out.ctypes.data))
        return out

    def accum_add_rgb8(self, spp: int, gamma: bool = False, out: np.ndarray = None) -> np.ndarray:
        out = self._accum_out(out, np.uint8)
        self._check(lib().rt_accum_add_rgb8(self.handle, int(spp), int(bool(gamma)), out.ctypes.data))
        return out

    def accum_read(self, out: np.ndarray = None) -> np.ndarray:
        out = self._accum_out(out, np.float32)
        self._check(lib().rt_accum_read(self.handle, out.ctypes.data))
        return out

    def accum_samples(self) -> int:
        return int(lib().rt_accum_samples(self.handle))

    def accum_end(self) -> None:
        self._check(lib().rt_accum_end(self.handle))
        self._accum_npix = 0

    def accum_begin_device(self, cam, env, npix, max_bounce, row0, row_step, device_index: int = 0) -> None:
        c, e = f32(cam), f32(env)
        self._check(lib().rt_accum_begin_device(self.handle, int(device_index), ptr(c), ptr(e), int(npix),
                                                int(max_bounce), int(row0), int(row_step)))

    # -- progressive lens frames (rt_accum_begin_lens*): every other accum_* call works on whichever kind is open --
    def accum_begin_lens(self, cam, env, lens: "Lens", npix: int, max_bounce: int) -> None:
        c, e = f32(cam), f32(env)
        if c.size != 10 or e.size != 5:
            raise ValueError("cam must have 10 floats and envData 5")
        self._check(lib().rt_accum_begin_lens(self.handle, ptr(c), ptr(e),
                                              ctypes.byref(lens) if lens is not None else None, int(npix),
                                              int(max_bounce)))
        self._accum_npix = int(npix)

    def accum_begin_lens_device(self, cam, env, lens: "Lens", npix, max_bounce, row0, row_step,
                                device_index: int = 0) -> None:
        c, e = f32(cam), f32(env)
        self._check(lib().rt_accum_begin_lens_device(self.handle, int(device_index), ptr(c), ptr(e),
                                                     ctypes.byref(lens) if lens is not None else None, int(npix),
                                                     int(max_bounce), int(row0), int(row_step)))

    def debug_accum_state(self) -> np.ndarray:
        """rt_debug_accum_state: the open host accumulation's records, a ``RADIANCE_STATE_DTYPE`` array ``[npix]``
        in frame order (blocking; nothing is rendered)."""
        n = getattr(self, "_accum_npix", 0)
        out = np.zeros(max(n, 1), RADIANCE_STATE_DTYPE)
        self._check(lib().rt_debug_accum_state(self.handle, out.ctypes.data))
        return out[:n]

    def accum_add_device(self, spp: int, d_out_ptr: int, stream_ptr: int = 0, device_index: int = 0) -> None:
        self._check(lib().rt_accum_add_device(self.handle, int(device_index), int(spp), _c_p(int(d_out_ptr)),
                                              _c_p(int(stream_ptr)) if stream_ptr else None))

    # -- adaptive sampling (rt_accum_mark / rt_accum_select* / rt_accum_add_selected) --
    def accum_mark(self) -> None:
        self._check(lib().rt_accum_mark(self.handle))

    def accum_select(self, threshold: float) -> int:
        """Select the pixels whose error since the mark exceeds ``threshold``; returns how many."""
        n = _i64(0)
        self._check(lib().rt_accum_select(self.handle, ctypes.c_float(float(threshold)), ctypes.byref(n)))
        return int(n.value)

    def accum_select_mask(self, mask) -> None:
        m = np.asarray(mask)
        n = getattr(self, "_accum_npix", 0)
        if m.size != n:
            raise ValueError(f"mask has {m.size} elements, needs imgDim = {n}")
        m = np.ascontiguousarray(m.reshape(-1) != 0, dtype=np.uint8)
        self._check(lib().rt_accum_select_mask(self.handle, m.ctypes.data if m.size else None))

    def accum_select_all(self) -> None:
        self._check(lib().rt_accum_select_all(self.handle))

    def accum_selection(self) -> np.ndarray:
        """The current selection as a 0/1 uint8 mask of imgDim pixels."""
        out = np.zeros(max(getattr(self, "_accum_npix", 0), 1), np.uint8)
        self._check(lib().rt_accum_selection(self.handle, out.ctypes.data))
        return out[:getattr(self, "_accum_npix", 0)]

    def accum_sample_map(self) -> np.ndarray:
        """Samples done, pixel by pixel (int32[imgDim])."""
        out = np.zeros(max(getattr(self, "_accum_npix", 0), 1), np.int32)
        self._check(lib().rt_accum_sample_map(self.handle, out.ctypes.data))
        return out[:getattr(self, "_accum_npix", 0)]

    def accum_add_selected(self, spp: int, out: np.ndarray = None) -> np.ndarray:
        """``spp`` more samples of every selected pixel; returns the whole frame (float32[3*npix])."""
        out = self._accum_out(out, np.float32)
        self._check(lib().rt_accum_add_selected(self.handle, int(spp), out.ctypes.data))
        return out

    @staticmethod
    def _stream(stream_ptr: int):
        return _c_p(int(stream_ptr)) if stream_ptr else None

    def accum_mark_device(self, stream_ptr: int = 0, device_index: int = 0) -> None:
        self._check(lib().rt_accum_mark_device(self.handle, int(device_index), self._stream(stream_ptr)))

    def accum_select_device(self, threshold: float, stream_ptr: int = 0, device_index: int = 0) -> None:
        self._check(lib().rt_accum_select_device(self.handle, int(device_index), ctypes.c_float(float(threshold)),
                                                 self._stream(stream_ptr)))

    def accum_select_mask_device(self, d_mask_ptr: int, stream_ptr: int = 0, device_index: int = 0) -> None:
        self._check(lib().rt_accum_select_mask_device(self.handle, int(device_index), _c_p(int(d_mask_ptr)),
                                                      self._stream(stream_ptr)))

    def accum_select_all_device(self, stream_ptr: int = 0, device_index: int = 0) -> None:
        self._check(lib().rt_accum_select_all_device(self.handle, int(device_index), self._stream(stream_ptr)))

    def accum_add_selected_device(self, spp: int, d_out_ptr: int, stream_ptr: int = 0, device_index: int = 0) -> None:
        self._check(lib().rt_accum_add_selected_device(self.handle, int(device_index), int(spp), _c_p(int(d_out_ptr)),
                                                       self._stream(stream_ptr)))

    # -- denoised previews (rt_accum_guides* / rt_denoise_device / rt_accum_denoise) --
    def accum_guides(self) -> np.ndarray:
        """The guide buffers of the open accumulation, float32[npix, 12]: n | k, P | f, a | m (f, m: int bits)."""
        n = getattr(self, "_accum_npix", 0)
        out = np.zeros((max(n, 1), GUIDE_FLOATS), np.float32)
        self._check(lib().rt_accum_guides(self.handle, out.ctypes.data))
        return out[:n]

    def accum_guides_device(self, d_guides_ptr: int, stream_ptr: int = 0, device_index: int = 0) -> None:
        self._check(lib().rt_accum_guides_device(self.handle, int(device_index),
                                                 _c_p(int(d_guides_ptr)) if d_guides_ptr else None,
                                                 self._stream(stream_ptr)))

    def denoise_device(self, d_rgb_ptr: int, d_guides_ptr: int, npix: int, width: int, d_out_ptr: int,
                       params: "DenoiseParams" = None, stream_ptr: int = 0, device_index: int = 0) -> None:
        """rt_denoise_device: filter a frame in device memory (``params`` None = the defaults)."""
        self._check(lib().rt_denoise_device(self.handle, int(device_index),
                                            _c_p(int(d_rgb_ptr)) if d_rgb_ptr else None,
                                            _c_p(int(d_guides_ptr)) if d_guides_ptr else None, int(npix), int(width),
                                            ctypes.byref(params) if params is not None else None,
                                            _c_p(int(d_out_ptr)) if d_out_ptr else None, self._stream(stream_ptr)))

    def accum_denoise(self, params: "DenoiseParams" = None, out: np.ndarray = None) -> np.ndarray:
        """The open accumulation's frame, denoised (float32[3*npix]); the state is untouched."""
        out = self._accum_out(out, np.float32)
        self._check(lib().rt_accum_denoise(self.handle, ctypes.byref(params) if params is not None else None,
                                           out.ctypes.data))
        return out

    def denoise(self, rgb, guides, npix: int, width: int, params: "DenoiseParams" = None,
                out: np.ndarray = None) -> np.ndarray:
        """rt_denoise: the filter on host arrays (float32 ``[3*npix]``, ``[12*npix]``), blocking."""
        c, g = f32(rgb).reshape(-1), f32(guides).reshape(-1)
        if c.size < 3 * int(npix) or g.size < GUIDE_FLOATS * int(npix):
            raise ValueError("rgb needs 3*npix floats and guides 12*npix")
        if out is None:
            out = np.zeros(3 * int(npix), np.float32)
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.size < 3 * int(npix):
            raise ValueError("output must be a contiguous float32 array of 3*npix elements")
        self._check(lib().rt_denoise(self.handle, ptr(c), ptr(g), int(npix), int(width),
                                     ctypes.byref(params) if params is not None else None, out.ctypes.data))
        return out

    # -- temporal reprojection (rt_reproject_device / rt_accum_reproject) --
    def reproject_device(self, d_prev_rgb_ptr: int, d_prev_guides_ptr: int, prev_cam, d_cur_rgb_ptr: int,
                         d_cur_guides_ptr: int, npix: int, width: int, d_out_rgb_ptr: int, d_out_guides_ptr: int,
                         params: "ReprojectParams" = None, stream_ptr: int = 0, device_index: int = 0) -> None:
        """rt_reproject_device: frames and guides in device memory (``params`` None = the defaults); never waits."""
        cam = f32(prev_cam).reshape(-1)
        if cam.size != 10:
            raise ValueError("prev_cam must have 10 floats")

        def p(x):
            return _c_p(int(x)) if x else None
        self._check(lib().rt_reproject_device(self.handle, int(device_index), p(d_prev_rgb_ptr), p(d_prev_guides_ptr),
                                              ptr(cam), p(d_cur_rgb_ptr), p(d_cur_guides_ptr), int(npix), int(width),
                                              ctypes.byref(params) if params is not None else None,
                                              p(d_out_rgb_ptr), p(d_out_guides_ptr), self._stream(stream_ptr)))

    def accum_reproject(self, prev_rgb, prev_guides, prev_cam, params: "ReprojectParams" = None,
                        out: np.ndarray = None):
        """rt_accum_reproject: the previous frame and guides (host arrays of the open accumulation's size) gathered
        into its view.  Returns ``(rgb float32[3*npix], guides float32[npix, 12])``; the state is untouched."""
        n = getattr(self, "_accum_npix", 0)
        c, g, cam = f32(prev_rgb).reshape(-1), f32(prev_guides).reshape(-1), f32(prev_cam).reshape(-1)
        if cam.size != 10:
            raise ValueError("prev_cam must have 10 floats")
        if n and (c.size != 3 * n or g.size != GUIDE_FLOATS * n):
            raise ValueError(f"the history must hold 3*{n} colour and 12*{n} guide floats, got {c.size} and {g.size}")
        out = self._accum_out(out, np.float32)
        out_g = np.zeros((max(n, 1), GUIDE_FLOATS), np.float32)
        self._check(lib().rt_accum_reproject(self.handle, ptr(c), ptr(g), ptr(cam),
                                             ctypes.byref(params) if params is not None else None, out.ctypes.data,
                                             out_g.ctypes.data))
        return out, out_g[:n]

    # -- ray queries (rt_trace / rt_trace_device) --
    def trace(self, rays8, mode: int = RT_QUERY_CLOSEST) -> np.ndarray:
        """rt_trace: ``rays8`` float32 ``[n, 8]`` (``pack_rays``) -> a ``HIT_DTYPE`` array ``[n]``, blocking."""
        r = f32(rays8)
        if r.size % RAY_FLOATS:
            raise ValueError("rays must hold 8 floats each: dir.xyz, origin.xyz, tmax, reserved")
        n = r.size // RAY_FLOATS
        out = np.zeros(n, HIT_DTYPE)
        self._check(lib().rt_trace(self.handle, ptr(r), n, int(mode), out.ctypes.data if n else None))
        return out

    def trace_device(self, device_index: int, rays_ptr: int, n: int, mode: int, out_ptr: int,
                     stream_ptr: int = 0) -> None:
        """rt_trace_device: device arrays on slot ``device_index``, enqueued on the stream; never waits."""
        self._check(lib().rt_trace_device(self.handle, int(device_index), _c_p(int(rays_ptr)) if rays_ptr else None,
                                          int(n), int(mode), _c_p(int(out_ptr)) if out_ptr else None,
                                          self._stream(stream_ptr)))

    # -- radiance queries (rt_radiance / rt_radiance_device, rt_camera_rays*) --
    def radiance(self, rays8, env, spp: int, max_bounce: int, state: np.ndarray = None) -> np.ndarray:
        """rt_radiance: ``rays8`` float32 ``[n, 8]`` (``pack_radiance_rays``) -> a ``RADIANCE_STATE_DTYPE`` array
        ``[n]``, blocking.  ``state`` (such an array, updated in place and returned) resumes its records."""
        r = np.ascontiguousarray(rays8, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] != RAY_FLOATS:
            raise ValueError(f"rays must be [n, {RAY_FLOATS}] float32, got {list(r.shape)}")
        n = len(r)
        e = f32(env).reshape(-1)
        if e.size < 5:
            raise ValueError("env needs 5 floats")
        flags = 0
        if state is not None:
            if not isinstance(state, np.ndarray) or state.dtype != RADIANCE_STATE_DTYPE or not state.flags.c_contiguous:
                raise TypeError("state must be a C-contiguous RADIANCE_STATE_DTYPE numpy array")
            if state.shape != (n,):
                raise ValueError(f"state has shape {list(state.shape)}, needs [{n}]")
            flags = RT_RADIANCE_RESUME
        else:
            state = np.zeros(n, RADIANCE_STATE_DTYPE)
        self._check(lib().rt_radiance(self.handle, ptr(r) if n else None, n, ptr(e), int(spp), int(max_bounce), flags,
                                      state.ctypes.data if n else None))
        return state

    def radiance_device(self, device_index: int, rays_ptr: int, n: int, env, spp: int, max_bounce: int, flags: int,
                        state_ptr: int, stream_ptr: int = 0) -> None:
        """rt_radiance_device: device arrays on slot ``device_index``, enqueued on the stream; never waits."""
        e = f32(env).reshape(-1)
        if e.size < 5:
            raise ValueError("env needs 5 floats")
        self._check(lib().rt_radiance_device(self.handle, int(device_index), _c_p(int(rays_ptr)) if rays_ptr else None,
                                             int(n), ptr(e), int(spp), int(max_bounce), int(flags),
                                             _c_p(int(state_ptr)) if state_ptr else None, self._stream(stream_ptr)))

    def camera_rays(self, cam, npix: int, first: int = 0, count: int = None) -> np.ndarray:
        """rt_camera_rays: float32 ``[count, 8]`` rays (with seeds) of pixels ``first .. first + count - 1``."""
        c = f32(cam).reshape(-1)
        if c.size < 10:
            raise ValueError("cam needs 10 floats")
        count = int(npix) - int(first) if count is None else int(count)
        out = np.zeros((max(count, 0), RAY_FLOATS), np.float32)
        self._check(lib().rt_camera_rays(self.handle, ptr(c), int(npix), int(first), count,
                                         out.ctypes.data if count > 0 else None))
        return out

    def camera_rays_device(self, device_index: int, cam, npix: int, first: int, count: int, rays_ptr: int,
                           stream_ptr: int = 0) -> None:
        c = f32(cam).reshape(-1)
        if c.size < 10:
            raise ValueError("cam needs 10 floats")
        self._check(lib().rt_camera_rays_device(self.handle, int(device_index), ptr(c), int(npix), int(first),
                                                int(count), _c_p(int(rays_ptr)) if rays_ptr else None,
                                                self._stream(stream_ptr)))

    # -- lens frames (rt_lens_radiance*, rt_lens_rays*, rt_radiance_resolve_device) --
    def lens_radiance(self, cam, env, lens: Lens, npix: int, first: int, count: int, spp: int, max_bounce: int,
                      state: np.ndarray = None) -> np.ndarray:
        """rt_lens_radiance: pixels ``first .. first + count - 1`` -> a ``RADIANCE_STATE_DTYPE`` array ``[count]``,
        blocking.  ``state`` (such an array, updated in place and returned) resumes its records."""
        c, e = f32(cam).reshape(-1), f32(env).reshape(-1)
        if c.size < 10 or e.size < 5:
            raise ValueError("cam needs 10 floats and env 5")
        count = int(count)
        flags = 0
        if state is not None:
            if not isinstance(state, np.ndarray) or state.dtype != RADIANCE_STATE_DTYPE or not state.flags.c_contiguous:
                raise TypeError("state must be a C-contiguous RADIANCE_STATE_DTYPE numpy array")
            if state.shape != (count,):
                raise ValueError(f"state has shape {list(state.shape)}, needs [{count}]")
            flags = RT_RADIANCE_RESUME
        else:
            state = np.zeros(max(count, 0), RADIANCE_STATE_DTYPE)
        self._check(lib().rt_lens_radiance(self.handle, ptr(c), ptr(e), ctypes.byref(lens), int(npix), int(first), count,
                                           int(spp), int(max_bounce), flags, state.ctypes.data if count > 0 else None))
        return state

    def lens_radiance_device(self, device_index: int, cam, env, lens: Lens, npix: int, first: int, count: int,
                             spp: int, max_bounce: int, flags: int, state_ptr: int, stream_ptr: int = 0) -> None:
        """rt_lens_radiance_device: device records on slot ``device_index``, enqueued on the stream; never waits."""
        c, e = f32(cam).reshape(-1), f32(env).reshape(-1)
        if c.size < 10 or e.size < 5:
            raise ValueError("cam needs 10 floats and env 5")
        self._check(lib().rt_lens_radiance_device(self.handle, int(device_index), ptr(c), ptr(e), ctypes.byref(lens),
                                                  int(npix), int(first), int(count), int(spp), int(max_bounce),
                                                  int(flags), _c_p(int(state_ptr)) if state_ptr else None,
                                                  self._stream(stream_ptr)))

    def lens_rays(self, cam, lens: Lens, npix: int, first: int = 0, count: int = None, sample0: int = 0,
                  nsamples: int = 1) -> np.ndarray:
        """rt_lens_rays: float32 ``[count, nsamples, 8]`` rays (with the pixels' seeds)."""
        c = f32(cam).reshape(-1)
        if c.size < 10:
            raise ValueError("cam needs 10 floats")
        count = int(npix) - int(first) if count is None else int(count)
        out = np.zeros((max(count, 0), max(int(nsamples), 0), RAY_FLOATS), np.float32)
        self._check(lib().rt_lens_rays(self.handle, ptr(c), ctypes.byref(lens), int(npix), int(first), count,
                                       int(sample0), int(nsamples), out.ctypes.data if out.size else None))
        return out

    def lens_rays_device(self, device_index: int, cam, lens: Lens, npix: int, first: int, count: int, sample0: int,
                         nsamples: int, rays_ptr: int, stream_ptr: int = 0) -> None:
        c = f32(cam).reshape(-1)
        if c.size < 10:
            raise ValueError("cam needs 10 floats")
        self._check(lib().rt_lens_rays_device(self.handle, int(device_index), ptr(c), ctypes.byref(lens), int(npix),
                                              int(first), int(count), int(sample0), int(nsamples),
                                              _c_p(int(rays_ptr)) if rays_ptr else None, self._stream(stream_ptr)))

    def radiance_resolve_device(self, device_index: int, state_ptr: int, n: int, rgb_ptr: int,
                                stream_ptr: int = 0) -> None:
        """rt_radiance_resolve_device: ``n`` device records -> ``3 * n`` clamped floats, enqueued on the stream."""
        self._check(lib().rt_radiance_resolve_device(self.handle, int(device_index),
                                                     _c_p(int(state_ptr)) if state_ptr else None, int(n),
                                                     _c_p(int(rgb_ptr)) if rgb_ptr else None, self._stream(stream_ptr)))

    def rgb8(self, src, gamma: bool = False, out=None) -> np.ndarray:
        """Host float32 -> uint8 through the device output stage."""
        s = f32(src).reshape(-1)
        if out is None:
            out = np.zeros(s.size, dtype=np.uint8)
        self._check(lib().rt_rgb8(self.handle, ptr(s), out.ctypes.data, s.size, int(bool(gamma))))
        return out

    def rgb8_device(self, d_in_ptr: int, d_out_ptr: int, n: int, gamma: bool = False, stream_ptr: int = 0,
                    device_index: int = 0) -> None:
        self._check(lib().rt_rgb8_device(self.handle, int(device_index), _c_p(int(d_in_ptr)), _c_p(int(d_out_ptr)),
                                         int(n), int(bool(gamma)), _c_p(int(stream_ptr)) if stream_ptr else None))

    def debug_math(self, fn: int, x, y=None):
        x = f32(x)
        yy = f32(y) if y is not None else None
        out = np.zeros_like(x)
        self._check(lib().rt_debug_math(self.handle, int(fn), ptr(x), ptr(yy), out.ctypes.data, x.size))
        return out

    # rt_debug_fn's functions (rt_debug.h): name -> (id, input floats per item, output floats per item)
    DEBUG_FN = {"camera": (0, 11, 3), "sun": (1, 5, 3), "hemi": (2, 6, 24), "ggx": (3, 13, 3), "ibl": (4, 4, 6),
                "mt_ref": (5, 24, 2), "mt_fast": (6, 24, 2), "box_ref": (7, 12, 1), "box_fast": (8, 13, 3)}

    def debug_fn(self, name: str, items) -> np.ndarray:
        """rt_debug_fn: one call of the kernels' own device function ``name`` per row of ``items``
        (float32[n, input floats]; integer words as their bit patterns); returns float32[n, output floats]."""
        fn, wi, wo = self.DEBUG_FN[name]
        x = f32(items)
        if x.ndim != 2 or x.shape[1] != wi:
            raise ValueError(f"{name}: items must be [n, {wi}] floats")
        out = np.zeros((x.shape[0], wo), dtype=np.float32)
        if x.shape[0]:
            self._check(lib().rt_debug_fn(self.handle, fn, ptr(x), out.ctypes.data, x.shape[0]))
        return out

    def debug_trace(self, rays, traversal: int):
        r = f32(rays).reshape(-1)
        out = np.zeros(2 * (r.size // 6), dtype=np.float32)
        self._check(lib().rt_debug_trace(self.handle, int(traversal), ptr(r), out.ctypes.data, r.size // 6))
        return out.reshape(-1, 2)

    def debug_trace_clustered(self, rays6):
        """rt_debug_trace_clustered: the clustered product trace on ``rays6`` (float32[n, 6]: dir, origin), one ray
        per lane.  Returns (k float32[n], tri int32[n] with -1 for a miss, info int32[4]: clusters, shell, floor,
        split walls -- what the kernel walked).  Raises NativeError on a scene without clusters."""
        r = f32(rays6).reshape(-1, 6)
        out = np.zeros((len(r), 2), dtype=np.float32)
        info = np.zeros(4, dtype=np.int32)
        self._check(lib().rt_debug_trace_clustered(self.handle, r.ctypes.data, out.ctypes.data, len(r), info.ctypes.data))
        return out[:, 0].copy(), out[:, 1].copy().view(np.int32), info

    def shell_word(self) -> int:
        """rt_debug_shell_word: the count word of the uploaded shell record (faces | split faces << 8 | SHELL_DIRECT
        when option "brute_direct" is on), 0 without a shell."""
        fn = lib().rt_debug_shell_word
        fn.restype, fn.argtypes = _i32, [_c_p]
        return int(fn(self.handle))

    def debug_pixel_log(self, traversal, cam, env, npix, spp, max_bounce, pixel, cap=4096):
        c, e = f32(cam), f32(env)
        log = np.zeros((cap, 16), np.float32)
        n = ctypes.c_int(0)
        out3 = np.zeros(3, np.float32)
        self._check(lib().rt_debug_pixel_log(self.handle, int(traversal), ptr(c), ptr(e), int(npix), int(spp),
                                             int(max_bounce), int(pixel), log.ctypes.data, cap, ctypes.byref(n),
                                             out3.ctypes.data))
        return log[: n.value].copy(), out3

    def wave_counts(self, cam, env, npix, spp, max_bounce):
        """rt_debug_wave_counts: lane counters + wave-level loop iterations of one frame."""
        c, e = f32(cam), f32(env)
        out = np.zeros(9, dtype=np.uint64)
        self._check(lib().rt_debug_wave_counts(self.handle, ptr(c), ptr(e), int(npix), int(spp), int(max_bounce),
                                               out.ctypes.data))
        keys = ("node_fetches", "tri_tests", "rays", "env_lookups", "stack_drops", "wave_trav_iters",
                "wave_render_iters", "cycles_shade", "cycles_trav")
        return {k: int(v) for k, v in zip(keys, out)}

    def scene_info(self):
        out = np.zeros(8, dtype=np.int64)
        self._check(lib().rt_debug_scene_info(self.handle, out.ctypes.data))
        return dict(fast_ok=bool(out[0]), depth=int(out[1]), nodes=int(out[2]), tris=int(out[3]),
                    brute_records=int(out[4]), brute_boxes=int(out[5]), wdq_omax=int(out[6]) * 1e-6)

    def debug_pilot_order(self, cost, chunk: int, levels: int, pilot: int, max_bounce: int) -> np.ndarray:
        """rt_debug_pilot_order: the pass-2 pixel order (uint32[n]) the device computes from ``cost`` (uint32[n]) with
        the launches of a two-pass render.  Raises NativeError for arguments the entry point rejects."""
        c = np.ascontiguousarray(cost, dtype=np.uint32).reshape(-1)
        out = np.zeros(max(c.size, 1), np.uint32)
        self._check(lib().rt_debug_pilot_order(self.handle, c.ctypes.data, c.size, int(chunk), int(levels),
                                               int(pilot), int(max_bounce), out.ctypes.data))
        return out[: c.size]

    def debug_pilot_pick(self, cost, lanes: int, spec: int):
        """rt_debug_pilot_pick: ``(left, pick word)`` the device computes from ``cost`` (uint32[n]) for ``lanes``
        resident lanes; the word is 1, 2 or 4 lanes per pixel, or ``SPEC_PICK`` + trails."""
        c = np.ascontiguousarray(cost, dtype=np.uint32).reshape(-1)
        out = np.zeros(2, np.int32)
        self._check(lib().rt_debug_pilot_pick(self.handle, c.ctypes.data, c.size, int(lanes), int(spec),
                                              out.ctypes.data))
        return int(out[0]), int(out[1])

    def debug_last_pilot(self):
        """rt_debug_last_pilot: ``(info, cost, order)`` of the context's last render launch, which ran two passes
        (NativeError with status RT_ERR_STATE when it ran one): info by name (``PILOT_FIELDS``), and the costs pass 1
        wrote and the pass-2 order, uint32[nloc] each."""
        info = np.zeros(len(PILOT_FIELDS), np.int64)
        self._check(lib().rt_debug_last_pilot(self.handle, info.ctypes.data, None, None, 0))
        n = int(info[1])
        cost, order = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self._check(lib().rt_debug_last_pilot(self.handle, info.ctypes.data, cost.ctypes.data, order.ctypes.data, n))
        return {name: int(v) for name, v in zip(PILOT_FIELDS, info)}, cost, order

    def timings(self) -> dict:
        """Host wall times (ms) of the last set_scene (pack / upload), set_env and render (rt_debug_timings)."""
        out = np.zeros(4, dtype=np.float64)
        self._check(lib().rt_debug_timings(self.handle, out.ctypes.data))
        return dict(pack_ms=float(out[0]), upload_ms=float(out[1]), env_ms=float(out[2]), render_ms=float(out[3]))


def parse_obj(text):
    """Native OBJ import (include/rt_scene.h): ``(V_p, V_n, V_uv, faceData, matCounter)``
    with the reference importer's semantics (FileManager.py:253-304).  Host only."""
    data = text.encode() if isinstance(text, str) else bytes(text)
    h = _c_p()
    H = host_lib()
    if H.rt_obj_parse(data, len(data), ctypes.byref(h)) != 0:
        raise ValueError("OBJ parse failed: " + H.rt_obj_last_error().decode(errors="replace"))
    try:
        n = [int(H.rt_obj_size(h, k)) for k in range(5)]
        vp, vn, vuv = (np.zeros(n[k], np.float32) for k in range(3))
        face = np.zeros(n[3], np.int32)
        H.rt_obj_copy(h, vp.ctypes.data, vn.ctypes.data, vuv.ctypes.data, face.ctypes.data)
    finally:
        H.rt_obj_free(h)
    return vp, vn, vuv, face, n[4]


def scene_check(V_p, V_n, faceData, materialData, bvh, layout: int = RT_BVH_SAH) -> dict:
    """rt_scene_check (include/rt_scene.h): the validation and repacking rt_set_scene applies, on the
    host alone (no GPU).  Raises NativeError with rt_set_scene's status for arrays it would refuse;
    returns the packed layout's sizes and, when the FAST layouts are unavailable, why."""
    vp, vn, face, mat, b = f32(V_p), f32(V_n), i32(faceData), f32(materialData), f32(bvh)
    info = np.zeros(8, np.int64)
    H = host_lib()
    st = H.rt_scene_check(ptr(vp), vp.size, ptr(vn), vn.size, ptr(face), face.size, ptr(mat), mat.size,
                          ptr(b), b.size, int(layout), info.ctypes.data)
    msg = H.rt_scene_last_error().decode(errors="replace")
    if st != 0:
        raise NativeError(st, msg)
    return dict(tris=int(info[0]), nodes=int(info[1]), depth=int(info[2]), wnodes=int(info[3]),
                wdepth=int(info[4]), brute_records=int(info[5]), brute_boxes=int(info[6]), fast_ok=bool(info[7]),
                note=msg)


def brute_layout(V_p, V_n, faceData, materialData, bvh, layout: int = RT_BVH_SAH):
    """rt_debug_brute_layout (include/rt_debug.h): the brute-force box array rt_set_scene would upload,
    on the host alone.  Returns ``(slots, nbox, nbrute)``: slots is a float32 array of 8 floats per slot,
    padding slots included (columns 6 and 7 hold the int bits of the slot's records)."""
    vp, vn, face, mat, b = f32(V_p), f32(V_n), i32(faceData), f32(materialData), f32(bvh)
    H = host_lib()
    info = np.zeros(3, np.int64)
    args = (ptr(vp), vp.size, ptr(vn), vn.size, ptr(face), face.size, ptr(mat), mat.size, ptr(b), b.size, int(layout))
    st = H.rt_debug_brute_layout(*args, None, 0, info.ctypes.data)
    if st != 0:
        raise NativeError(st, H.rt_scene_last_error().decode(errors="replace"))
    boxes = np.zeros(int(info[2]), np.float32)
    st = H.rt_debug_brute_layout(*args, boxes.ctypes.data, boxes.size, info.ctypes.data)
    if st != 0:
        raise NativeError(st, H.rt_scene_last_error().decode(errors="replace"))
    return boxes.reshape(-1, 8), int(info[0]), int(info[1])


def brute_clusters(V_p, V_n, faceData, materialData, bvh, cluster: int = -1, layout: int = RT_BVH_SAH):
    """rt_debug_brute_clusters (include/rt_debug.h): the clustered box array option "brute_cluster" = cluster
    uploads, on the host alone.  Returns ``(slots, rows, nsingle)``: slots as brute_layout's (the singles
    padded to a group of 4, then 8 slots per cluster), rows 8 floats per cluster (the union box, then the int
    bits of first slot and box count); both empty when the scene is not clustered."""
    vp, vn, face, mat, b = f32(V_p), f32(V_n), i32(faceData), f32(materialData), f32(bvh)
    H = host_lib()
    info = np.zeros(4, np.int64)
    args = (ptr(vp), vp.size, ptr(vn), vn.size, ptr(face), face.size, ptr(mat), mat.size, ptr(b), b.size, int(layout),
            int(cluster))
    st = H.rt_debug_brute_clusters(*args, None, 0, None, 0, info.ctypes.data)
    if st != 0:
        raise NativeError(st, H.rt_scene_last_error().decode(errors="replace"))
    slots, rows = np.zeros(int(info[2]), np.float32), np.zeros(int(info[3]), np.float32)
    st = H.rt_debug_brute_clusters(*args, slots.ctypes.data, slots.size, rows.ctypes.data, rows.size, info.ctypes.data)
    if st != 0:
        raise NativeError(st, H.rt_scene_last_error().decode(errors="replace"))
    return slots.reshape(-1, 8), rows.reshape(-1, 8), int(info[1])


SHELL_REC_FLOATS = 76   # rt_debug_brute_shell's record: the box, two counts, two records for each of six faces, seven rows of 8


def brute_shell(V_p, V_n, faceData, materialData, bvh, cluster: int = -1, shell: int = -1, layout: int = RT_BVH_SAH):
    """rt_debug_brute_shell (include/rt_debug.h): the shell option "brute_shell" = shell uploads for the scene
    clustered with "brute_cluster" = cluster, on the host alone.  Returns None when there is no shell, else a dict:
    ``box`` (float32 lo.x hi.x lo.y hi.y lo.z hi.z), ``faces`` (int32 [6, 2]: the two records of the faces -x +x
    -y +y -z +z, -1 -1 where absent), ``nfaces``, ``nrest`` and ``rest`` (the slots of the singles that are no
    face, as brute_layout's, padding included)."""
    vp, vn, face, mat, b = f32(V_p), f32(V_n), i32(faceData), f32(materialData), f32(bvh)
    H = host_lib()
    info = np.zeros(3, np.int64)
    args = (ptr(vp), vp.size, ptr(vn), vn.size, ptr(face), face.size, ptr(mat), mat.size, ptr(b), b.size, int(layout),
            int(cluster), int(shell))
    st = H.rt_debug_brute_shell(*args, None, 0, info.ctypes.data)
    if st != 0:
        raise NativeError(st, H.rt_scene_last_error().decode(errors="replace"))
    if int(info[0]) == 0:
        return None
    rec = np.zeros(int(info[2]), np.float32)
    st = H.rt_debug_brute_shell(*args, rec.ctypes.data, rec.size, info.ctypes.data)
    if st != 0:
        raise NativeError(st, H.rt_scene_last_error().decode(errors="replace"))
    ints = rec[:SHELL_REC_FLOATS].view(np.int32)
    # (the face count's word carries the number of split faces above bit 8, option "brute_quad")
    return dict(box=rec[:6].copy(), nrest=int(ints[6]), nfaces=int(ints[7]) & 0xff, faces=ints[8:20].reshape(6, 2).copy(),
                rest=rec[SHELL_REC_FLOATS:].reshape(-1, 8).copy())


NEAR_FLOOR = np.float32(0.0001) * (np.float32(1.0) - np.float32(2.0 ** -12))   # rt_layout.h kNearFloor


def brute_near(V_p, V_n, faceData, materialData, bvh, cluster: int = -1, shell: int = -1, layout: int = RT_BVH_SAH):
    """rt_debug_brute_near (include/rt_debug.h), on the host alone: ``(flags, floor, nfaces)`` -- flags[g] is True
    where box g of brute_layout's array is near-safe (option "brute_near"), floor is the lower clamp the face tests
    of the shell of brute_shell(cluster, shell) get (NEAR_FLOOR or 0.0) and nfaces that shell's faces (0: none)."""
    vp, vn, face, mat, b = f32(V_p), f32(V_n), i32(faceData), f32(materialData), f32(bvh)
    H = host_lib()
    info = np.zeros(2, np.int64)
    floor = np.zeros(1, np.float32)
    args = (ptr(vp), vp.size, ptr(vn), vn.size, ptr(face), face.size, ptr(mat), mat.size, ptr(b), b.size, int(layout),
            int(cluster), int(shell))
    st = H.rt_debug_brute_near(*args, None, 0, floor.ctypes.data, info.ctypes.data)
    if st != 0:
        raise NativeError(st, H.rt_scene_last_error().decode(errors="replace"))
    flags = np.zeros(int(info[0]), np.int32)
    st = H.rt_debug_brute_near(*args, flags.ctypes.data if flags.size else None, flags.size, floor.ctypes.data,
                               info.ctypes.data)
    if st != 0:
        raise NativeError(st, H.rt_scene_last_error().decode(errors="replace"))
    return flags.astype(bool), np.float32(floor[0]), int(info[1])


QUAD_BAND, QUAD_GRAZE, QUAD_DIR_MAX = np.float32(2.0 ** -8), np.float32(2.0 ** -6), np.float32(2.0)   # rt_layout.h


def brute_quad(V_p, V_n, faceData, materialData, bvh, cluster: int = -1, shell: int = -1, quad: int = -1,
               layout: int = RT_BVH_SAH):
    """rt_debug_brute_quad (include/rt_debug.h), on the host alone: a dict of ``split`` and ``side`` (bool [6], per
    face position -x +x -y +y -z +z), ``lines`` (float32 [6, 4]: A.xyz gamma), ``words`` (uint32 [6, 3]: the packed
    records both / sigma >= 0 / sigma < 0), ``recs`` (float32 [6, 2, 3, 3]: p0, e1, e2 of the two records), ``guard`` (kQuadBand, kQuadGraze, kQuadDirMax), ``nfaces``, ``nsplit``."""
    vp, vn, face, mat, b = f32(V_p), f32(V_n), i32(faceData), f32(materialData), f32(bvh)
    flags, lines, words = np.zeros(6, np.int32), np.zeros(24, np.float32), np.zeros(18, np.int32)
    recs, guard, info = np.zeros(108, np.float32), np.zeros(3, np.float32), np.zeros(2, np.int64)
    st = host_lib().rt_debug_brute_quad(ptr(vp), vp.size, ptr(vn), vn.size, ptr(face), face.size, ptr(mat), mat.size,
                                        ptr(b), b.size, int(layout), int(cluster), int(shell), int(quad),
                                        flags.ctypes.data, lines.ctypes.data, words.ctypes.data, recs.ctypes.data,
                                        guard.ctypes.data,
                                        info.ctypes.data)
    if st != 0:
        raise NativeError(st, host_lib().rt_scene_last_error().decode(errors="replace"))
    return dict(split=(flags & 1).astype(bool), side=((flags >> 1) & 1).astype(bool), lines=lines.reshape(6, 4),
                words=words.view(np.uint32).reshape(6, 3), recs=recs.reshape(6, 2, 3, 3), guard=guard, nfaces=int(info[0]), nsplit=int(info[1]))


SHELL_DIRECT = 1 << 16   # rt_layout.h kShellDirect: option "brute_direct" in the shell record's count word


def brute_direct(V_p, V_n, faceData, materialData, bvh, cluster: int = -1, shell: int = -1, direct: int = -1,
                 layout: int = RT_BVH_SAH):
    """rt_debug_brute_direct (include/rt_debug.h), on the host alone: ``(nfaces, on, word)`` -- the faces of the shell
    of brute_shell(cluster, shell) (0: none), whether its record carries option "brute_direct"'s bit, and the record's
    count word as the kernels load it (0 without a shell)."""
    vp, vn, face, mat, b = f32(V_p), f32(V_n), i32(faceData), f32(materialData), f32(bvh)
    H = host_lib()
    fn = H.rt_debug_brute_direct   # (bound here: a library from before the option still loads)
    fn.restype, fn.argtypes = _i32, [_c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _c_p, _i64, _i32, _i32, _i32, _i32, _c_p]
    info = np.zeros(3, np.int64)
    st = fn(ptr(vp), vp.size, ptr(vn), vn.size, ptr(face), face.size, ptr(mat), mat.size, ptr(b), b.size, int(layout),
            int(cluster), int(shell), int(direct), info.ctypes.data)
    if st != 0:
        raise NativeError(st, H.rt_scene_last_error().decode(errors="replace"))
    return int(info[0]), bool(info[1]), int(info[2])


def last_direct() -> bool:
    """rt_debug_last_direct: whether the last render launch's kernel walked a shell whose record enables the in-place
    test of a lane's first record (option "brute_direct")."""
    fn = lib().rt_debug_last_direct
    fn.restype, fn.argtypes = _i32, []
    return bool(fn())


def brute_slices(nloc: int, lanes: int, spp: int, option: int = -1, accum_base: int = -1):
    """rt_debug_brute_slices (include/rt_debug.h): ``(on, K, tail)`` of the sample-slice rule for brute-force
    scenes, evaluated on the host alone."""
    out = np.zeros(3, np.int32)
    st = lib().rt_debug_brute_slices(int(nloc), int(lanes), int(spp), int(option), int(accum_base), out.ctypes.data)
    if st != 0:
        raise NativeError(st, "rt_debug_brute_slices: bad arguments")
    return bool(out[0]), int(out[1]), int(out[2])


def last_slices() -> int:
    """rt_debug_last_slices: the slice word the last render launch's kernel got (0: unsliced)."""
    return int(lib().rt_debug_last_slices())


def brute_refill(nloc: int, lanes: int, option: int = -1) -> int:
    """rt_debug_brute_refill (include/rt_debug.h): the refill threshold R of the one-lane brute-force kernels
    (0: every free lane is refilled at once), from the host's rule alone."""
    out = np.zeros(1, np.int32)
    st = lib().rt_debug_brute_refill(int(nloc), int(lanes), int(option), out.ctypes.data)
    if st != 0:
        raise NativeError(st, "rt_debug_brute_refill: bad arguments")
    return int(out[0])


def brute_lean(materialData, env, spp: int = 4, max_bounce: int = 4, pass_: int = 0, pilot: int = 0,
               fixed_point: int = 1, sun_cache: int = 1, option: int = -1, loop: int = 3, team: int = 1,
               count: int = 0, log: int = 0, acc: int = 0, traversal: int = 0):
    """rt_debug_brute_lean (include/rt_debug.h), on the host alone: ``(diffuse_only, lean)`` -- whether every material
    of the table has type 0 or 1, and whether a launch of that kernel over such a frame runs the lean kernel."""
    mat, e = f32(materialData), f32(env)
    fn = lib().rt_debug_brute_lean   # (bound here: a library from before the option still loads)
    fn.restype, fn.argtypes = _i32, [_c_p, _i64, _c_p, _c_p, _c_p, _c_p]
    frame = np.array([spp, max_bounce, pass_, pilot, fixed_point, sun_cache, option], np.int32)
    kernel = np.array([loop, team, count, log, acc, traversal], np.int32)
    out = np.zeros(2, np.int32)
    st = fn(ptr(mat) if mat.size else None, mat.size, ptr(e), frame.ctypes.data, kernel.ctypes.data, out.ctypes.data)
    if st != 0:
        raise NativeError(st, "rt_debug_brute_lean: bad arguments")
    return bool(out[0]), bool(out[1])


def last_refill():
    """rt_debug_last_refill: ``(R, events, lanes)`` -- the threshold the last render launch's kernel got, and the
    refill counters of the last instrumented launch."""
    out = np.zeros(3, np.int64)
    st = lib().rt_debug_last_refill(out.ctypes.data)
    if st != 0:
        raise NativeError(st, "rt_debug_last_refill: bad arguments")
    return int(out[0]), int(out[1]), int(out[2])


LAUNCH_FIELDS = ("trav", "count", "log", "smem", "ovf", "resume", "step", "wide", "brute", "ts", "acc",
                 "team", "walk_team", "slices", "refill", "grid", "lds", "shell", "near", "quad", "primary")
BRUTE_SLICED = 4   # bits of the key's ``brute`` beside the loop (brute & 3: 1 lock-step, 2 teams, 3 clustered)
BRUTE_REFILL = 8
BRUTE_LEAN = 16    # the lean form of the one-lane kernels (option "brute_lean"; rt_debug_brute_lean has the rule)


def last_launch() -> dict:
    """rt_debug_last_launch (include/rt_debug.h): the kernel key of the last render launch and the team sizes,
    slice word, refill threshold, grid and LDS bytes its kernel got, whether it walked a shell and whether that
    shell's face tests had a non-zero floor (option "brute_near") and its record split walls (option "brute_quad"), and
    whether a pre-pass traced the launch's camera rays (option "brute_primary"), by name
    (``LAUNCH_FIELDS``)."""
    out = np.zeros(len(LAUNCH_FIELDS), np.int32)
    st = lib().rt_debug_last_launch(out.ctypes.data)
    if st != 0:
        raise NativeError(st, "rt_debug_last_launch: bad arguments")
    return {name: int(v) for name, v in zip(LAUNCH_FIELDS, out)}


def tile_rows(npix: int, width: int, row0: int, row_step: int) -> int:
    return int(lib().rt_tile_rows(int(npix), int(width), int(row0), int(row_step)))

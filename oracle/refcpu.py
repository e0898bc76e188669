"""Drive the reference's own kernels on the CPU.

TEST INFRASTRUCTURE ONLY.  ``oracle/_ref/librefcpu.so`` is the reference's kernel text
(``Raytracing.cl`` and what it includes) compiled for the host by ``make -C oracle ref``
where the reference tree exists, linked with ``oracle/ref_cl/cpu_shim.c``, which supplies
the OpenCL builtins from the numerics contract (``csrc/rtm.h``).  No OpenCL runtime, no
GPU: a kernel is a C function and :func:`_run` loops it over its work-items.

Shaped like :mod:`oracle.refcl`: :func:`render` takes ``launch_Raytracing``'s arguments and
the ``kat_*`` functions have ``refcl``'s signatures, plus :func:`kat_pixel_state` and
:func:`kat_gi_sample`.

The reference's code indexes its arrays unchecked, so a caller hands it only what
``launch_Raytracing`` would accept: no empty scene, no malformed BVH or face indices, a
camera whose width ``(int)cam[6]`` is positive.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
LIB_PATH = os.path.join(REF_DIR, "librefcpu.so")
_libs: dict = {}


class _Image(ctypes.Structure):
    _fields_ = [("w", ctypes.c_int32), ("h", ctypes.c_int32), ("rgba", ctypes.c_void_p)]


def available(path: str = LIB_PATH) -> bool:
    return os.path.exists(path)


def _L(path: str = LIB_PATH):
    lib = _libs.get(path)
    if lib is None:
        lib = ctypes.CDLL(path)
        lib.ref_run.restype = ctypes.c_int
        lib.ref_run.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_int64,
                                ctypes.c_int]
        _libs[path] = lib
    return lib


def _threads() -> int:
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))))


class _Launch:
    """Collects a kernel's arguments in order; keeps every array alive until the run is over."""

    def __init__(self, name: str, lib_path: str = LIB_PATH):
        self.lib = _L(lib_path)
        self.fn = ctypes.cast(getattr(self.lib, name), ctypes.c_void_p)
        self.args = []
        self._keep = []

    def buf(self, arr, dtype, out: bool = False):
        arr = np.array(arr, dtype=dtype, order="C", copy=True) if out else np.ascontiguousarray(arr, dtype=dtype)
        self._keep.append(arr)
        self.args.append(arr.ctypes.data)
        return arr

    def scalar(self, value: int):
        self.args.append(int(value) & 0xFFFFFFFF)

    def image(self, rgba):
        img = np.ascontiguousarray(rgba, dtype=np.uint8)
        assert img.ndim == 3 and img.shape[2] == 4 and img.shape[0] > 0 and img.shape[1] > 0, "IBL must be HxWx4"
        desc = _Image(img.shape[1], img.shape[0], img.ctypes.data)
        self._keep += [img, desc]
        self.args.append(ctypes.addressof(desc))

    def run(self, n: int):
        a = (ctypes.c_uint64 * len(self.args))(*self.args)
        if self.lib.ref_run(self.fn, a, len(self.args), int(n), _threads()) != 0:
            raise RuntimeError("refcpu: ref_run rejected its arguments")


def _pad(a, dtype):
    """The launcher hands an empty V_uv or lightData over as one element."""
    a = np.ascontiguousarray(a if a is not None else [], dtype=dtype).reshape(-1)
    return a if a.size else np.zeros(1, dtype)


def _scene_bufs(L: _Launch, vp, vn, vuv, face):
    L.buf(vp, np.float32)
    L.buf(vn, np.float32)
    L.buf(_pad(vuv, np.float32), np.float32)
    return L.buf(face, np.int32)


def render(vp, vn, vuv, face, light, mat, bvh, cam, env, imgDim: int, spp: int, max_bounce: int, ibl_rgba,
           lib_path: str = LIB_PATH):
    """The reference's ``Raytracing`` kernel over ``imgDim`` work-items; returns float32 [3*imgDim]."""
    L = _Launch("Raytracing", lib_path)
    out = L.buf(np.zeros(3 * imgDim, np.float32), np.float32, out=True)
    face = _scene_bufs(L, vp, vn, vuv, face)
    nlight = int(np.asarray(light if light is not None else []).size)
    L.buf(_pad(light, np.int32), np.int32)
    L.buf(mat, np.float32)
    L.buf(bvh, np.float32)
    L.buf(cam, np.float32)
    L.buf(env, np.float32)
    L.scalar(face.size // 10)
    L.scalar(nlight)
    L.scalar(imgDim)
    L.scalar(spp)
    L.scalar(max_bounce)
    L.image(ibl_rgba)
    L.run(imgDim)
    return out


def kat_pixel_state(vp, vn, vuv, face, mat, bvh, cam, env, imgDim: int, spp: int, max_bounce: int, ibl_rgba):
    """Per pixel, before the kernel's output stage: (sum float32 [n,3] unclamped, seeds uint32 [n,2]
    after the last sample, hit float32 [n,2] = camera hit's k and hit flag)."""
    L = _Launch("kat_pixel_state")
    face = _scene_bufs(L, vp, vn, vuv, face)
    L.buf(mat, np.float32)
    L.buf(bvh, np.float32)
    L.buf(cam, np.float32)
    L.buf(env, np.float32)
    L.scalar(face.size // 10)
    L.scalar(imgDim)
    L.scalar(spp)
    L.scalar(max_bounce)
    L.image(ibl_rgba)
    s = L.buf(np.zeros(3 * imgDim, np.float32), np.float32, out=True)
    sd = L.buf(np.zeros(2 * imgDim, np.uint32), np.uint32, out=True)
    hit = L.buf(np.zeros(2 * imgDim, np.float32), np.float32, out=True)
    L.run(imgDim)
    return s.reshape(-1, 3), sd.reshape(-1, 2), hit.reshape(-1, 2)


def kat_gi_sample(vp, vn, vuv, face, mat, bvh, cam, env, max_bounce: int, ibl_rgba, idx, seeds):
    """One ``naiveGI`` call per entry on the camera hit of pixel ``idx[t]`` from ``seeds[t]``;
    returns (colour float32 [n,3], seeds after uint32 [n,2])."""
    idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
    L = _Launch("kat_gi_sample")
    face = _scene_bufs(L, vp, vn, vuv, face)
    L.buf(mat, np.float32)
    L.buf(bvh, np.float32)
    L.buf(cam, np.float32)
    L.buf(env, np.float32)
    L.scalar(face.size // 10)
    L.scalar(max_bounce)
    L.image(ibl_rgba)
    L.buf(idx, np.int32)
    sd = L.buf(np.asarray(seeds, np.uint32).reshape(-1), np.uint32, out=True)
    assert sd.size == 2 * idx.size
    out = L.buf(np.zeros(3 * idx.size, np.float32), np.float32, out=True)
    L.run(idx.size)
    return out.reshape(-1, 3), sd.reshape(-1, 2)


# ---------------- known-answer tests of single reference functions (refcl's signatures) ----------------

def kat_rand(seeds: np.ndarray, nd: int):
    seeds = np.ascontiguousarray(seeds, np.uint32).reshape(-1, 2)
    n = seeds.shape[0]
    L = _Launch("kat_rand")
    L.buf(seeds.reshape(-1), np.uint32)
    L.scalar(nd)
    out = L.buf(np.zeros(n * nd, np.float32), np.float32, out=True)
    st = L.buf(np.zeros(2 * n, np.uint32), np.uint32, out=True)
    L.run(n)
    return out.reshape(n, nd), st.reshape(n, 2)


def kat_camera(cam, idx):
    idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
    L = _Launch("kat_camera")
    L.buf(cam, np.float32)
    L.buf(idx, np.int32)
    out = L.buf(np.zeros(6 * idx.size, np.float32), np.float32, out=True)
    L.run(idx.size)
    return out.reshape(-1, 6)


def _simple(name, inp, width_in, width_out, out_dtype=np.float32):
    inp = np.ascontiguousarray(inp, np.float32).reshape(-1, width_in)
    n = inp.shape[0]
    L = _Launch(name)
    L.buf(inp.reshape(-1), np.float32)
    out = L.buf(np.zeros(n * width_out, out_dtype), out_dtype, out=True)
    L.run(n)
    return out.reshape(n, width_out)


def kat_rotate(inp7):
    return _simple("kat_rotate", inp7, 7, 3)


def kat_intersect(inp15):
    return _simple("kat_intersect", inp15, 15, 2)


def kat_box(inp12):
    return _simple("kat_box", inp12, 12, 1, np.int32)[:, 0]


def kat_ggx(inp15):
    return _simple("kat_ggx", inp15, 15, 3)


def kat_sphmap(dirs):
    return _simple("kat_sphmap", dirs, 3, 2)


def kat_trace(vp, vn, vuv, face, bvh, rays):
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    L = _Launch("kat_trace")
    face = _scene_bufs(L, vp, vn, vuv, face)
    L.buf(bvh, np.float32)
    L.scalar(face.size // 10)
    L.buf(rays.reshape(-1), np.float32)
    out = L.buf(np.zeros(8 * n, np.float32), np.float32, out=True)
    L.run(n)
    return out.reshape(n, 8)


def kat_ibl(ibl_rgba, dirs):
    """Completeness only: the fetch is the shim's, so this pins ``SampleSphericalMap`` and the
    coordinate conversion, nothing about image hardware."""
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    n = dirs.shape[0]
    L = _Launch("kat_ibl")
    L.image(ibl_rgba)
    L.buf(dirs.reshape(-1), np.float32)
    out = L.buf(np.zeros(5 * n, np.float32), np.float32, out=True)
    L.run(n)
    return out.reshape(n, 5)


def kat_texel(ibl_rgba, xy):
    """Completeness only: returns the shim's own definition of the fetch."""
    xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    n = xy.shape[0]
    L = _Launch("kat_texel")
    L.image(ibl_rgba)
    L.buf(xy.reshape(-1), np.int32)
    out = L.buf(np.zeros(4 * n, np.float32), np.float32, out=True)
    L.run(n)
    return out.reshape(n, 4)


def kat_hemi(kind: int, normals, seeds):
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    n = normals.shape[0]
    L = _Launch("kat_hemi")
    L.scalar(kind)
    L.buf(normals.reshape(-1), np.float32)
    sd = L.buf(np.asarray(seeds, np.uint32).reshape(-1), np.uint32, out=True)
    out = L.buf(np.zeros(4 * n, np.float32), np.float32, out=True)
    L.run(n)
    return out.reshape(n, 4), sd.reshape(n, 2)


def kat_math(fn: int, x, y=None):
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    y = np.ascontiguousarray(np.zeros_like(x) if y is None else y, np.float32).reshape(-1)
    L = _Launch("kat_math")
    L.scalar(fn)
    L.buf(x, np.float32)
    L.buf(y, np.float32)
    out = L.buf(np.zeros_like(x), np.float32, out=True)
    L.run(x.size)
    return out


def build_info() -> dict:
    """The compiler and flags the library was built with, as the recipe recorded them beside it."""
    try:
        with open(os.path.join(REF_DIR, "librefcpu.txt")) as f:
            lines = [ln.strip() for ln in f.read().splitlines() if ln.strip()]
    except OSError:
        return {"compiler": "unknown"}
    info = {"compiler": lines[0] if lines else "unknown"}
    for ln in lines[1:]:
        k, _, v = ln.partition(":")
        info[k.strip() + "_flags"] = " ".join(v.split())
    return info


# ---------------- the golden fixture (tests/golden/ref_cpu_frames.npz; tools/gen_golden.py --cpu) ----------------

# proto and furnace hold the pixels the frame clamps to 1 (9 % and 1 % of theirs), whose sums only the state shows
GOLDEN_STATE_CASES = ("cornell_64_s4", "serre_96x54_s4", "proto_64_s4", "furnace_64_s4")


def golden_frames() -> dict:
    """What the library renders now, as the fixture stores it: ``frame_<case>`` of every parity case and
    ``sum_ / seeds_ / hit_<case>`` (:func:`kat_pixel_state`) of ``GOLDEN_STATE_CASES``."""
    from ensem3a_openclraytracer_amd import workloads as W
    res = {}
    for name, wl in W.PARITY_CASES.items():
        sc, cam, env, npix, spp, mb, ibl = wl.inputs()
        res["frame_" + name] = render(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.lightData, sc.materialData,
                                      sc.BVH.exportArray, cam, env, npix, spp, mb, ibl)
        if name in GOLDEN_STATE_CASES:
            s, sd, hit = kat_pixel_state(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray,
                                         cam, env, npix, spp, mb, ibl)
            res["sum_" + name], res["seeds_" + name], res["hit_" + name] = s, sd, hit
    return res

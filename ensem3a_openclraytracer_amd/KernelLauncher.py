"""Drop-in replacement of the reference's ``KernelLauncher`` (KernelLauncher.py:6-103).

Same constructor and method signatures, same argument meaning, same in-place
output contract; the pyopencl program build / buffer uploads / enqueue /
blocking read-back are replaced by ctypes calls into the HIP C-ABI
(include/rt_api.h).  Errors raise :class:`~._native.NativeError`
(a ``RuntimeError``), as pyopencl raises its own ``RuntimeError`` subclasses.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np

from . import _native

try:  # xxhash is in the image; hashlib is the portable fallback for the upload cache key
    import xxhash

    def _digest(a: np.ndarray) -> bytes:
        return xxhash.xxh3_128_digest(memoryview(np.ascontiguousarray(a)).cast("B"))
except ImportError:  # pragma: no cover
    import hashlib

    def _digest(a: np.ndarray) -> bytes:
        return hashlib.blake2b(memoryview(np.ascontiguousarray(a)).cast("B"), digest_size=16).digest()


def _ibl_rgba(h_IBL) -> np.ndarray:
    """RGBA8 texels of the IBL: a PIL image (as ``main.py:68`` passes) or an HxWx4 uint8 array."""
    if isinstance(h_IBL, np.ndarray):
        img = h_IBL
    elif hasattr(h_IBL, "tobytes") and hasattr(h_IBL, "size"):
        mode = getattr(h_IBL, "mode", "RGBA")
        if mode != "RGBA":
            h_IBL = h_IBL.convert("RGBA")
        w, h = h_IBL.size
        img = np.frombuffer(h_IBL.tobytes(), dtype=np.uint8).reshape(h, w, 4)
    else:
        raise TypeError("h_IBL must be a PIL.Image or an HxWx4 uint8 array")
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 4:
        raise ValueError(f"IBL must be RGBA8 (HxWx4 uint8), got {img.dtype} {img.shape}")
    return np.ascontiguousarray(img)


class History(object):
    """What a frame knew when the camera moved (``Progressive.history``): the frame ``rgb`` float32 ``[3*imgDim]``,
    its guides ``[imgDim, 12]`` -- whose ``f`` word is the history's length in samples -- and the camera ``cam``
    they were made with; ``width`` is ``int(cam[6])``.  ``Progressive.reprojected`` of the next view takes it."""

    def __init__(self, rgb: np.ndarray, guides: np.ndarray, cam: np.ndarray, imgDim: int):
        self.rgb = rgb
        self.guides = guides
        self.cam = cam
        self.imgDim = int(imgDim)
        self.width = int(cam[6])


class Progressive(object):
    """A frame that takes more samples (``KernelLauncher.begin_progressive``; rt_accum_* of rt_api.h).

    Every ``add`` returns a finished frame at the samples done so far -- the frame ``launch_Raytracing``
    renders at that ``spp``, bit for bit -- and costs only the samples it adds.  Opened by
    ``begin_progressive_lens`` it is a lens frame instead: read ``lens_frame`` for ``launch_Raytracing`` below.
    """

    def __init__(self, ctx: "_native.Context", imgDim: int, cam=None):
        self._ctx = ctx
        self._n = int(imgDim)
        self._open = True
        self._cam = None if cam is None else np.array(cam, dtype=np.float32).reshape(-1)[:10]

    def _out(self, out, dtype):
        if not self._open:
            raise RuntimeError("the progressive render is closed (or was replaced by a later begin_progressive)")
        if out is None:
            return np.zeros(3 * self._n, dtype)
        if not isinstance(out, np.ndarray) or out.dtype != dtype or not out.flags.c_contiguous:
            raise TypeError(f"out must be a C-contiguous {np.dtype(dtype).name} numpy array")
        if out.size < 3 * self._n:
            raise ValueError(f"out has {out.size} elements, needs 3*imgDim = {3 * self._n}")
        return out

    def add(self, spp: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """``spp`` (>= 1) more samples of every pixel; the frame (float32 ``[3*imgDim]``, into ``out`` if given)."""
        out = self._out(out, np.float32)
        self._ctx.accum_add(int(spp), out=out.reshape(-1))
        return out

    def add_rgb8(self, spp: int, gamma: bool = False, out: Optional[np.ndarray] = None) -> np.ndarray:
        """``add`` with the 8-bit output stage of ``launch_Raytracing_rgb8`` on the device (a preview)."""
        out = self._out(out, np.uint8)
        self._ctx.accum_add_rgb8(int(spp), gamma=gamma, out=out.reshape(-1))
        return out

    def image(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The frame at the samples done; nothing is rendered."""
        out = self._out(out, np.float32)
        self._ctx.accum_read(out=out.reshape(-1))
        return out

    # -- adaptive sampling: refine only the pixels that need it.  A pixel that has received n samples holds the
    # value of ``launch_Raytracing`` at ``spp = n``, bit for bit, whatever the other pixels received. --
    def _live(self) -> None:
        if not self._open:
            raise RuntimeError("the progressive render is closed (or was replaced by a later begin_progressive)")

    def mark(self) -> None:
        """Snapshot every pixel's sum and sample count: what ``select`` measures the frame's change against."""
        self._live()
        self._ctx.accum_mark()

    def select(self, threshold: float) -> int:
        """Select the pixels that got samples since ``mark`` and whose colour moved by more than ``threshold``
        (|change| summed over r, g, b, over sqrt(r + g + b + 0.01) of the new colour; rt_api.h).  Returns how
        many are selected."""
        self._live()
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold must not be NaN")
        return self._ctx.accum_select(threshold)

    def select_mask(self, mask) -> None:
        """Select the pixels where ``mask`` (``imgDim`` elements, any shape) is non-zero."""
        self._live()
        m = np.asarray(mask)
        if m.size != self._n:
            raise ValueError(f"mask has {m.size} elements, needs imgDim = {self._n}")
        self._ctx.accum_select_mask(m)

    def select_all(self) -> None:
        self._live()
        self._ctx.accum_select_all()

    def selection(self) -> np.ndarray:
        """The current selection, a 0/1 uint8 mask of ``imgDim`` pixels."""
        self._live()
        return self._ctx.accum_selection()

    def sample_map(self) -> np.ndarray:
        """Samples done, pixel by pixel (int32 ``[imgDim]``)."""
        self._live()
        return self._ctx.accum_sample_map()

    def add_selected(self, spp: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """``spp`` (>= 1) more samples of every selected pixel, each from its own count; the whole frame."""
        out = self._out(out, np.float32)
        self._ctx.accum_add_selected(int(spp), out=out.reshape(-1))
        return out

    def refine(self, threshold: float, min_spp: int, max_spp: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """On a fresh accumulation: ``2 * min_spp`` samples of every pixel, then doublings of only the pixels
        whose colour still moved by more than ``threshold`` between the first half of their samples and all of
        them (the half-buffer estimate), until none is left or they hold ``max_spp``.  A pixel ends with
        ``2 * min_spp * 2**k`` samples (capped at ``max_spp``); returns the frame."""
        min_spp, max_spp = int(min_spp), int(max_spp)
        if min_spp < 1:
            raise ValueError("min_spp must be >= 1")
        if max_spp < 2 * min_spp:
            raise ValueError("max_spp must be at least 2 * min_spp")
        out = self._out(out, np.float32)
        self.add(min_spp, out)
        self.mark()
        self.add(min_spp, out)
        c = 2 * min_spp   # the samples every selected pixel holds
        n = self.select(threshold)
        while n > 0 and c < max_spp:
            step = min(c, max_spp - c)
            self.mark()
            self.add_selected(step, out)
            c += step
            n = self.select(threshold)
        return out

    # -- denoised previews: presentable frames from the first few samples.  Nothing is rendered and the
    # accumulation is untouched: ``image()`` stays the exact frame. --
    def guides(self) -> dict:
        """The first-hit guide buffers (rt_accum_guides), as views of one ``[imgDim, 12]`` array: ``normal``
        ``[n, 3]`` and ``depth`` ``[n]`` (0, 0, 0 and -1 on a miss), ``position`` ``[n, 3]``, ``albedo`` ``[n, 3]``
        (1, 1, 1 where the pixel is not filterable), ``material`` int32 ``[n]`` (-1 on a miss) and
        ``filterable_samples`` int32 ``[n]``: the pixel's sample count where its first hit is diffuse or glossy,
        else 0."""
        self._live()
        g = self._ctx.accum_guides()
        return {"normal": g[:, 0:3], "depth": g[:, 3], "position": g[:, 4:7], "albedo": g[:, 8:11],
                "material": g[:, 11].view(np.int32), "filterable_samples": g[:, 7].view(np.int32)}

    def denoised(self, passes: int = 5, normal_squarings: int = 5, sigma_c: float = 1.5, sigma_p: float = 0.02,
                 out: Optional[np.ndarray] = None) -> np.ndarray:
        """The frame at the samples done, through the edge-aware filter of rt_api.h (rt_accum_denoise): a
        preview for display.  Pixels whose first hit is not diffuse or glossy are ``image()``'s, bit for bit."""
        passes, normal_squarings = int(passes), int(normal_squarings)
        sigma_c, sigma_p = float(sigma_c), float(sigma_p)
        if not 1 <= passes <= 8:
            raise ValueError("passes must be 1..8")
        if not 0 <= normal_squarings <= 8:
            raise ValueError("normal_squarings must be 0..8")
        for name, v in (("sigma_c", sigma_c), ("sigma_p", sigma_p)):
            if not (v > 0.0 and v != float("inf")):
                raise ValueError(f"{name} must be finite and > 0")
        out = self._out(out, np.float32)
        self._ctx.accum_denoise(_native.DenoiseParams(passes, normal_squarings, sigma_c, sigma_p), out=out.reshape(-1))
        return out

    # -- temporal reprojection: carry the frame's history across a camera move.  Nothing is rendered and the
    # accumulation is untouched: ``image()`` stays the exact frame. --
    def history(self) -> History:
        """The frame and the guides at the samples done, with the camera: what ``reprojected`` of the next view
        takes.  Read it before the ``begin_progressive*`` that replaces this accumulation."""
        self._live()
        if self._cam is None:
            raise RuntimeError("this progressive render was opened without its camera")
        return History(self.image(), self._ctx.accum_guides(), self._cam.copy(), self._n)

    def reprojected(self, history: History, sigma_p: float = 0.02, normal_min: float = 0.9, max_history: float = 64.0,
                    min_weight: float = 0.25, denoise: bool = False, out: Optional[np.ndarray] = None,
                    return_history: bool = False):
        """The frame at the samples done, blended with ``history`` -- the frame of another camera on the same scene
        and environment -- gathered into this view (rt_accum_reproject of rt_api.h): a pixel whose first hit the
        previous view saw too keeps that view's samples, up to ``max_history`` of them.  With ``denoise`` the result
        goes through the edge-aware filter, whose colour bandwidth follows the blended counts (``sigma_p`` is shared,
        the other filter parameters are the defaults).  Pixels without history are ``image()``'s, bit for bit.  With
        ``return_history`` returns ``(frame, History)``: the blended, unfiltered frame and its guides under this
        camera, the history of the next move."""
        self._live()
        if not isinstance(history, History):
            raise TypeError("history must be a History (Progressive.history)")
        if history.imgDim != self._n:
            raise ValueError(f"the history has {history.imgDim} pixels, this frame {self._n}")
        sigma_p, normal_min = float(sigma_p), float(normal_min)
        max_history, min_weight = float(max_history), float(min_weight)
        for name, v in (("sigma_p", sigma_p), ("max_history", max_history)):
            if not (v > 0.0 and v != float("inf")):
                raise ValueError(f"{name} must be finite and > 0")
        for name, v in (("normal_min", normal_min), ("min_weight", min_weight)):
            if not (v == v and abs(v) != float("inf")):
                raise ValueError(f"{name} must be finite")
        if return_history and self._cam is None:
            raise RuntimeError("this progressive render was opened without its camera")
        out = self._out(out, np.float32)
        rgb, guides = self._ctx.accum_reproject(history.rgb, history.guides, history.cam,
                                                _native.ReprojectParams(sigma_p, normal_min, max_history, min_weight))
        if denoise:
            self._ctx.denoise(rgb, guides, self._n, history.width, _native.DenoiseParams(sigma_p=sigma_p),
                              out=out.reshape(-1))
        else:
            out.reshape(-1)[:3 * self._n] = rgb
        return (out, History(rgb, guides, self._cam.copy(), self._n)) if return_history else out

    @property
    def samples(self) -> int:
        """Samples done per pixel -- the most a pixel holds once ``add_selected`` made them differ (-1 once closed)."""
        return self._ctx.accum_samples() if self._open else -1

    def close(self) -> None:
        if self._open:
            self._open = False
            self._ctx.accum_end()


class KernelLauncher(object):
    """``KernelLauncher(context, platform, device, queue)``.

    ``context``, ``platform`` and ``queue`` exist for signature compatibility
    and are not used (there is no OpenCL context).  ``device`` selects the
    GPU(s): ``None`` = device 0, an ``int`` = that device, a sequence of ints =
    render on all of them (rows interleaved).  Keyword ``traversal`` picks the
    BVH traversal: ``"fast"`` (default) or ``"ref"`` (the reference's own DFS);
    ``bvh`` the tree the fast traversal walks: ``"sah"`` (default) or
    ``"reference"`` (the exported BVH.py tree) -- both give identical hits.
    """

    def __init__(self, context=None, platform=None, device: Union[None, int, Sequence[int]] = None, queue=None,
                 traversal: str = "fast", bvh: str = "sah"):
        self.platform = platform
        self.device = device
        self.context = context
        self.queue = queue
        if device is None or not isinstance(device, (int, list, tuple)):
            ids = [0]
        elif isinstance(device, int):
            ids = [device]
        else:
            ids = list(device)
        self._ctx = _native.Context(device_ids=ids)
        self.set_traversal(traversal)
        self.set_bvh(bvh)
        self._scene_key: Optional[tuple] = None
        self._env_key: Optional[tuple] = None
        self._face_material: Optional[np.ndarray] = None
        self._face_material_dev: dict = {}

    def set_traversal(self, traversal: str) -> None:
        mode = {"fast": _native.RT_TRAVERSAL_FAST, "ref": _native.RT_TRAVERSAL_REF}.get(traversal)
        if mode is None:
            raise ValueError("traversal must be 'fast' or 'ref'")
        self._ctx.set_option("traversal", mode)
        self.traversal = traversal

    def set_bvh(self, bvh: str) -> None:
        mode = {"reference": _native.RT_BVH_REFERENCE, "sah": _native.RT_BVH_SAH}.get(bvh)
        if mode is None:
            raise ValueError("bvh must be 'sah' or 'reference'")
        self._ctx.set_option("bvh", mode)
        self.bvh = bvh

    @property
    def native(self) -> _native.Context:
        return self._ctx

    # ------------------------------------------------------------------
    def _upload_scene(self, vp, vn, vuv, face, mat, bvh) -> None:
        arrays = (_native.f32(vp), _native.f32(vn), _native.f32(vuv), _native.i32(face), _native.f32(mat),
                  _native.f32(bvh))
        key = tuple((a.size, _digest(a)) for a in arrays)
        if key != self._scene_key:
            self._ctx.set_scene(*arrays)
            self._scene_key = key
            self._face_material = arrays[3].reshape(-1, 10)[:, 0].copy()   # trace_rays: a hit's material
            self._face_material_dev = {}

    def _upload_env(self, h_IBL) -> None:
        img = _ibl_rgba(h_IBL)
        key = (img.shape, _digest(img))
        if key != self._env_key:
            self._ctx.set_env(img)
            self._env_key = key

    def launch_Raytracing(self, h_img_out, h_vertex_p, h_vertex_n, h_vertex_uv, h_face_data, h_material_data,
                          h_light_data, h_BVH, h_cam, h_envData, imgDim, spp, maxBounce, h_IBL):
        """Render ``imgDim`` pixels into ``h_img_out`` (float32 ``[3*imgDim]``, written in place).

        Argument meaning as ``KernelLauncher.py:33-87``: the row width is
        ``int(h_cam[6])``; ``h_light_data`` is accepted and, as in the
        reference kernel, unused.  Blocking; returns ``None``.
        """
        if not isinstance(h_img_out, np.ndarray) or h_img_out.dtype != np.float32 or \
                not h_img_out.flags.c_contiguous:
            raise TypeError("h_img_out must be a C-contiguous float32 numpy array")
        imgDim = int(imgDim)
        if h_img_out.size < 3 * imgDim:
            raise ValueError(f"h_img_out has {h_img_out.size} floats, needs 3*imgDim = {3 * imgDim}")
        cam = _native.f32(h_cam).reshape(-1)
        env = _native.f32(h_envData).reshape(-1)
        if cam.size < 10 or env.size < 5:
            raise ValueError("h_cam needs 10 floats and h_envData 5")
        if h_light_data is not None:
            np.asarray(h_light_data)  # accepted for signature compatibility (unused by the kernel)
        self._upload_scene(h_vertex_p, h_vertex_n, h_vertex_uv, h_face_data, h_material_data, h_BVH)
        self._upload_env(h_IBL)
        out = h_img_out.reshape(-1)
        self._ctx.render(cam[:10], env[:5], imgDim, int(spp), int(maxBounce), out=out)

    def launch_Raytracing_rgb8(self, h_img_out, h_vertex_p, h_vertex_n, h_vertex_uv, h_face_data,
                               h_material_data, h_light_data, h_BVH, h_cam, h_envData, imgDim, spp, maxBounce,
                               h_IBL, gamma: bool = False):
        """``launch_Raytracing`` fused with the output stage: ``h_img_out`` is uint8 ``[3*imgDim]`` and
        receives ``(frame*255).astype('uint8')`` (FileManager.saveImg, FileManager.py:334-336),
        after the ImgProcessing gamma when ``gamma`` -- quantized on the device, so a quarter of
        the bytes cross PCIe."""
        if not isinstance(h_img_out, np.ndarray) or h_img_out.dtype != np.uint8 or \
                not h_img_out.flags.c_contiguous:
            raise TypeError("h_img_out must be a C-contiguous uint8 numpy array")
        imgDim = int(imgDim)
        if h_img_out.size < 3 * imgDim:
            raise ValueError(f"h_img_out has {h_img_out.size} bytes, needs 3*imgDim = {3 * imgDim}")
        cam = _native.f32(h_cam).reshape(-1)
        env = _native.f32(h_envData).reshape(-1)
        if cam.size < 10 or env.size < 5:
            raise ValueError("h_cam needs 10 floats and h_envData 5")
        self._upload_scene(h_vertex_p, h_vertex_n, h_vertex_uv, h_face_data, h_material_data, h_BVH)
        self._upload_env(h_IBL)
        self._ctx.render_rgb8(cam[:10], env[:5], imgDim, int(spp), int(maxBounce), gamma=gamma,
                              out=h_img_out.reshape(-1))

    def begin_progressive(self, h_vertex_p, h_vertex_n, h_vertex_uv, h_face_data, h_material_data, h_light_data,
                          h_BVH, h_cam, h_envData, imgDim, maxBounce, h_IBL) -> "Progressive":
        """Open a progressive render of the frame ``launch_Raytracing`` would render from these arguments
        (its order, without ``h_img_out`` and ``spp``): the returned :class:`Progressive` adds samples to
        the frame, and after adds of ``a`` and ``b`` samples the frame is, bit for bit, ``launch_Raytracing``
        at ``spp = a + b``.  One per launcher at a time: a second call replaces the first.  Uploading another
        scene or IBL (a ``launch_Raytracing`` with other arrays) invalidates it: its next ``add`` raises
        :class:`~._native.NativeError`; a call with the same arrays (an upload-cache hit) does not."""
        imgDim = int(imgDim)
        cam = _native.f32(h_cam).reshape(-1)
        env = _native.f32(h_envData).reshape(-1)
        if cam.size < 10 or env.size < 5:
            raise ValueError("h_cam needs 10 floats and h_envData 5")
        if h_light_data is not None:
            np.asarray(h_light_data)  # accepted for signature compatibility (unused by the kernel)
        self._upload_scene(h_vertex_p, h_vertex_n, h_vertex_uv, h_face_data, h_material_data, h_BVH)
        self._upload_env(h_IBL)
        if getattr(self, "_progressive", None) is not None:
            self._progressive._open = False   # replaced: the context holds one accumulation
        self._ctx.accum_begin(cam[:10], env[:5], imgDim, int(maxBounce))
        self._progressive = Progressive(self._ctx, imgDim, cam[:10])
        return self._progressive

    def begin_progressive_lens(self, h_vertex_p, h_vertex_n, h_vertex_uv, h_face_data, h_material_data, h_light_data,
                               h_BVH, h_cam, h_envData, imgDim, maxBounce, h_IBL, jitter: float = 1.0,
                               aperture: float = 0.0, focus: float = 1.0, seed: int = 0) -> "Progressive":
        """``begin_progressive`` for a lens frame (rt_accum_begin_lens of rt_api.h): every sample goes down a camera
        ray of its own -- ``jitter``, ``aperture``, ``focus`` and ``seed`` as ``lens_frame`` takes them -- so the
        frames that ``add``, ``refine`` and ``denoised`` return have anti-aliased edges and depth of field.  A pixel
        that has received ``n`` samples holds ``lens_frame``'s value at ``spp = n``, bit for bit; ``jitter = 0,
        aperture = 0`` is ``begin_progressive``.  The guides describe the pixel-centre pinhole ray's first hit,
        whatever the lens: with ``aperture > 0`` the filter under-smooths edges that are out of focus."""
        imgDim = int(imgDim)
        cam = _native.f32(h_cam).reshape(-1)
        env = _native.f32(h_envData).reshape(-1)
        if cam.size < 10 or env.size < 5:
            raise ValueError("h_cam needs 10 floats and h_envData 5")
        if imgDim < 1:
            raise ValueError("imgDim must be >= 1")
        _, lens, _, _, _ = self._lens_args(cam, imgDim, jitter, aperture, focus, seed, 0, None)
        if h_light_data is not None:
            np.asarray(h_light_data)  # accepted for signature compatibility (unused by the kernel)
        self._upload_scene(h_vertex_p, h_vertex_n, h_vertex_uv, h_face_data, h_material_data, h_BVH)
        self._upload_env(h_IBL)
        if getattr(self, "_progressive", None) is not None:
            self._progressive._open = False   # replaced: the context holds one accumulation
        self._ctx.accum_begin_lens(cam[:10], env[:5], lens, imgDim, int(maxBounce))
        self._progressive = Progressive(self._ctx, imgDim, cam[:10])
        return self._progressive

    def upload_scene(self, h_vertex_p, h_vertex_n, h_vertex_uv, h_face_data, h_material_data, h_BVH) -> None:
        """Upload the scene alone (what ``launch_Raytracing`` does with these arguments): ``trace_rays`` needs
        no environment and no frame."""
        self._upload_scene(h_vertex_p, h_vertex_n, h_vertex_uv, h_face_data, h_material_data, h_BVH)

    def trace_rays(self, origins, directions, tmax=None, any_hit: bool = False) -> dict:
        """Trace rays of the caller's own through the uploaded scene (rt_trace of rt_api.h): the hits a frame
        would see, under the launcher's traversal.  ``origins`` and ``directions`` are ``[n, 3]`` (directions are
        used as given, not normalised), ``tmax`` a scalar or ``[n]`` (None: the horizon, 1000; a hit has
        ``k < min(tmax, 1000)``).  Returns ``k`` (1000 on a miss), ``tri`` (the row of faceData, -1 on a miss),
        ``u``, ``v`` (barycentrics, 0 on a miss), ``hit`` and ``material`` (``faceData[tri, 0]``, -1 on a miss).
        With ``any_hit`` the flag is the closest-hit query's, and a hit describes some triangle the ray really
        hits within ``tmax``, not necessarily the closest.

        numpy arrays are traced blocking, split over the launcher's devices.  Objects with ``data_ptr()`` (torch
        tensors on the launcher's first device) go through the device form on torch's current stream: nothing
        is copied to the host and the call does not wait; the results are tensors on that device."""
        if getattr(self, "_face_material", None) is None:
            raise RuntimeError("trace_rays needs a scene: call upload_scene or launch_Raytracing first")
        mode = _native.RT_QUERY_ANY if any_hit else _native.RT_QUERY_CLOSEST
        if hasattr(origins, "data_ptr") or hasattr(directions, "data_ptr"):
            return self._trace_rays_torch(origins, directions, tmax, mode)
        hits = self._ctx.trace(_native.pack_rays(origins, directions, tmax), mode)
        hit = hits["tri"] >= 0
        material = np.full(len(hits), -1, np.int32)
        material[hit] = self._face_material[hits["tri"][hit]]
        return {"k": hits["k"].copy(), "tri": hits["tri"].copy(), "u": hits["u"].copy(), "v": hits["v"].copy(),
                "hit": hit, "material": material}

    def _trace_rays_torch(self, origins, directions, tmax, mode: int) -> dict:
        import torch
        dev = origins.device if hasattr(origins, "data_ptr") else directions.device
        o = torch.as_tensor(origins, dtype=torch.float32, device=dev).reshape(-1, 3)
        d = torch.as_tensor(directions, dtype=torch.float32, device=dev).reshape(-1, 3)
        if o.shape[0] != d.shape[0]:
            raise ValueError(f"{o.shape[0]} origins but {d.shape[0]} directions")
        n = o.shape[0]
        rays = torch.zeros((n, _native.RAY_FLOATS), dtype=torch.float32, device=dev)
        rays[:, 0:3] = d
        rays[:, 3:6] = o
        rays[:, 6] = _native.QUERY_HORIZON if tmax is None else torch.as_tensor(tmax, dtype=torch.float32, device=dev)
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        if n:
            self._ctx.trace_device(0, rays.data_ptr(), n, mode, out.data_ptr(),
                                   torch.cuda.current_stream(dev).cuda_stream)
        tri = out[:, 1].view(torch.int32)
        hit = tri >= 0
        table = self._face_material_dev.get(dev)
        if table is None:
            table = torch.as_tensor(self._face_material, dtype=torch.int32, device=dev)
            self._face_material_dev[dev] = table
        material = torch.where(hit, table[tri.clamp(min=0).long()] if len(table) else tri, torch.full_like(tri, -1))
        return {"k": out[:, 0], "tri": tri, "u": out[:, 2], "v": out[:, 3], "hit": hit, "material": material}

    def upload_env(self, h_IBL) -> None:
        """Upload the environment map alone (what ``launch_Raytracing`` does with ``h_IBL``): ``radiance`` needs a
        scene and an environment, and no frame."""
        self._upload_env(h_IBL)

    def camera_rays(self, cam, npix) -> tuple:
        """The rays ``launch_Raytracing`` gives the ``npix`` pixels of ``cam``'s frame (rt_camera_rays of rt_api.h):
        ``(origins [n, 3], directions [n, 3], seeds uint32 [n, 2])`` -- ``radiance`` of them is that frame."""
        cam = _native.f32(cam).reshape(-1)
        if cam.size < 10:
            raise ValueError("cam needs 10 floats")
        rays = self._ctx.camera_rays(cam[:10], int(npix))
        return rays[:, 3:6].copy(), rays[:, 0:3].copy(), rays[:, 6:8].copy().view(np.uint32)

    def radiance(self, origins, directions, spp, max_bounce, env, seeds=None, state=None) -> dict:
        """Path-trace rays of the caller's own (rt_radiance of rt_api.h): ``spp`` samples of the frame's integrator
        along each ray, under the launcher's traversal, with ``env`` and ``max_bounce`` as ``launch_Raytracing``
        takes ``h_envData`` and ``maxBounce``.  ``origins`` and ``directions`` are ``[n, 3]`` (directions are used
        as given, not normalised); ``seeds`` is uint32 ``[n, 2]``, the RNG state each ray starts from (None:
        ``(ray index, 0)``, the decorrelation a frame gives its pixels).  The camera rays of a frame with that
        frame's seeds (``camera_rays``) give that frame, bit for bit.

        Returns ``rgb`` (``sum / float32(n)``, not clamped: a baker keeps values above 1), ``sum``, ``n`` (samples
        done), ``k``, ``tri``, ``hit`` (the first hit, as ``trace_rays`` reports it) and ``state``.  Passing the
        returned ``state`` back as ``state`` adds ``spp`` more samples to every ray -- after calls of ``a`` and
        ``b`` samples the result is that of one call of ``a + b`` -- and ``seeds`` is then ignored; keeping a ray's
        total at or below ``2**24`` samples is the caller's job.

        numpy arrays go through the blocking host form, split over the launcher's devices.  Objects with
        ``data_ptr()`` (torch tensors on the launcher's first device) go through the device form on torch's current
        stream: nothing is copied to the host and the call does not wait; the results are tensors on that device
        (``state`` an int32 ``[n, 8]`` tensor of the records' words, updated in place when passed back)."""
        spp = int(spp)
        if spp < 1:
            raise ValueError("spp must be >= 1")
        e = _native.f32(env).reshape(-1)
        if e.size < 5:
            raise ValueError("env needs 5 floats")
        if hasattr(origins, "data_ptr") or hasattr(directions, "data_ptr"):
            return self._radiance_torch(origins, directions, spp, int(max_bounce), e[:5], seeds, state)
        o = np.asarray(origins, dtype=np.float32)
        d = np.asarray(directions, dtype=np.float32)
        for name, a in (("origins", o), ("directions", d)):
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError(f"{name} must be [n, 3], got {list(a.shape)}")
        rays = _native.pack_radiance_rays(o, d, seeds)   # (counts that differ, the seeds' shape and type)
        if state is not None:
            if not isinstance(state, np.ndarray) or state.dtype != _native.RADIANCE_STATE_DTYPE:
                raise TypeError("state must be the 'state' array an earlier call returned")
            if state.shape != (len(rays),):
                raise ValueError(f"state holds {state.size} records, needs {len(rays)}")
            state = np.ascontiguousarray(state)
        st = self._ctx.radiance(rays, e[:5], spp, int(max_bounce), state=state)
        n = st["n"].copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            rgb = st["sum"] / n.astype(np.float32)[:, None]
        return {"rgb": rgb, "sum": st["sum"].copy(), "n": n, "k": st["k"].copy(), "tri": st["tri"].copy(),
                "hit": st["tri"] >= 0, "state": st}

    def _radiance_torch(self, origins, directions, spp, max_bounce, env, seeds, state) -> dict:
        import torch
        dev = origins.device if hasattr(origins, "data_ptr") else directions.device
        o = torch.as_tensor(origins, dtype=torch.float32, device=dev)
        d = torch.as_tensor(directions, dtype=torch.float32, device=dev)
        for name, a in (("origins", o), ("directions", d)):
            if a.dim() != 2 or a.shape[1] != 3:
                raise ValueError(f"{name} must be [n, 3], got {list(a.shape)}")
        if o.shape[0] != d.shape[0]:
            raise ValueError(f"{o.shape[0]} origins but {d.shape[0]} directions")
        n = o.shape[0]
        rays = torch.zeros((n, _native.RAY_FLOATS), dtype=torch.float32, device=dev)
        rays[:, 0:3] = d
        rays[:, 3:6] = o
        words = rays.view(torch.int32)
        if seeds is None:
            words[:, 6] = torch.arange(n, dtype=torch.int32, device=dev)
        else:
            sd = torch.as_tensor(seeds, device=dev)
            if sd.dtype.is_floating_point or sd.dtype == torch.bool:
                raise TypeError(f"seeds must be integers, got {sd.dtype}")
            if tuple(sd.shape) != (n, 2):
                raise ValueError(f"seeds must be [{n}, 2], got {list(sd.shape)}")
            words[:, 6:8] = sd.to(torch.int64).to(torch.int32)   # (the low 32 bits: uint32 seeds keep theirs)
        flags = 0
        if state is not None:
            if not hasattr(state, "data_ptr") or state.dtype != torch.int32 or not state.is_contiguous():
                raise TypeError("state must be the contiguous int32 'state' tensor an earlier call returned")
            if tuple(state.shape) != (n, 8) or state.device != rays.device:
                raise ValueError(f"state must be [{n}, 8] on {rays.device}, got {list(state.shape)} on {state.device}")
            flags = _native.RT_RADIANCE_RESUME
        else:
            state = torch.empty((n, 8), dtype=torch.int32, device=dev)
        if n:
            self._ctx.radiance_device(0, rays.data_ptr(), n, env, spp, max_bounce, flags, state.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream)
        total = state[:, 0:3].view(torch.float32)
        count = state[:, 7]
        tri = state[:, 6]
        return {"rgb": total / count.to(torch.float32)[:, None], "sum": total, "n": count,
                "k": state[:, 3].view(torch.float32), "tri": tri, "hit": tri >= 0, "state": state}

    @staticmethod
    def _lens_args(cam, npix, jitter, aperture, focus, seed, first, count):
        """The checked camera, lens and pixel range of ``lens_frame`` / ``lens_rays`` (rt_api.h's argument rules)."""
        cam = _native.f32(cam).reshape(-1)
        if cam.size < 10:
            raise ValueError("cam needs 10 floats")
        npix, first = int(npix), int(first)
        count = npix - first if count is None else int(count)
        if npix < 1 or first < 0 or count < 0 or first + count > npix:
            raise ValueError(f"pixels {first} .. +{count} outside the frame of {npix}")
        jitter, aperture, focus = float(jitter), float(aperture), float(focus)
        if not (np.isfinite(jitter) and jitter >= 0.0):
            raise ValueError("jitter must be finite and >= 0")
        if not (np.isfinite(aperture) and aperture >= 0.0):
            raise ValueError("aperture must be finite and >= 0")
        if not (np.isfinite(focus) and focus > 0.0):
            raise ValueError("focus must be finite and > 0")
        seed = int(seed)
        if not 0 <= seed < 2 ** 32:
            raise ValueError("seed must be a uint32")
        return cam[:10], _native.Lens(jitter, aperture, focus, seed), npix, first, count

    def lens_rays(self, cam, npix, jitter, aperture, focus, seed, first=0, count=None, sample0=0, nsamples=1):
        """The sample rays of a lens frame (rt_lens_rays of rt_api.h): float32 ``[count, nsamples, 8]``, ray
        ``[t, q]`` that of pixel ``first + t`` and sample ``sample0 + q`` -- direction, origin, then the pixel's
        frame seeds as uint bits.  Needs no scene."""
        cam, lens, npix, first, count = self._lens_args(cam, npix, jitter, aperture, focus, seed, first, count)
        sample0, nsamples = int(sample0), int(nsamples)
        if sample0 < 0 or nsamples < 1:
            raise ValueError("sample0 must be >= 0 and nsamples >= 1")
        return self._ctx.lens_rays(cam, lens, npix, first, count, sample0, nsamples)

    def lens_frame(self, cam, env, npix, spp, max_bounce, jitter=1.0, aperture=0.0, focus=1.0, seed=0, first=0,
                   count=None, state=None) -> dict:
        """A frame whose every sample goes down a camera ray of its own (rt_lens_radiance of rt_api.h): ``jitter``
        is the width in pixels of the box filter the samples are spread over (anti-aliasing), ``aperture`` the
        radius of a thin lens and ``focus`` the distance of the plane in focus along the view axis (depth of
        field); ``seed`` selects the rays' uniforms.  ``jitter = 0, aperture = 0`` is ``launch_Raytracing``'s
        frame, bit for bit.  Pixels ``first .. first + count - 1`` of ``cam``'s frame of ``npix`` are rendered.

        Returns ``rgb`` (the clamped frame ``[count, 3]``), ``sum``, ``n`` and ``state``.  Passing the returned
        ``state`` back adds ``spp`` more samples to every pixel: after calls of ``a`` and ``b`` samples the result
        is that of one call of ``a + b``.  A numpy state (or none) goes through the blocking host form, split over
        the launcher's devices; a torch int32 ``[count, 8]`` tensor on the launcher's first device goes through
        the device form on torch's current stream, is updated in place, and the results are tensors there (nothing
        is copied to the host and the call does not wait); ``lens_state`` makes the tensor a frame starts from."""
        spp = int(spp)
        if spp < 1:
            raise ValueError("spp must be >= 1")
        e = _native.f32(env).reshape(-1)
        if e.size < 5:
            raise ValueError("env needs 5 floats")
        cam, lens, npix, first, count = self._lens_args(cam, npix, jitter, aperture, focus, seed, first, count)
        if state is not None and hasattr(state, "data_ptr"):
            import torch
            if state.dtype != torch.int32 or not state.is_contiguous():
                raise TypeError("state must be a contiguous int32 tensor")
            if tuple(state.shape) != (count, 8) or not state.is_cuda:
                raise ValueError(f"state must be [{count}, 8] on the launcher's device, got {list(state.shape)}")
            stream = torch.cuda.current_stream(state.device).cuda_stream
            if count:
                self._ctx.lens_radiance_device(0, cam, e[:5], lens, npix, first, count, spp, int(max_bounce),
                                               _native.RT_RADIANCE_RESUME, state.data_ptr(), stream)
            rgb = torch.empty((count, 3), dtype=torch.float32, device=state.device)
            if count:
                self._ctx.radiance_resolve_device(0, state.data_ptr(), count, rgb.data_ptr(), stream)
            return {"rgb": rgb, "sum": state[:, 0:3].view(torch.float32), "n": state[:, 7], "state": state}
        if state is not None:
            if not isinstance(state, np.ndarray) or state.dtype != _native.RADIANCE_STATE_DTYPE:
                raise TypeError("state must be the 'state' array an earlier call returned")
            if state.shape != (count,):
                raise ValueError(f"state holds {state.size} records, needs {count}")
            state = np.ascontiguousarray(state)
        st = self._ctx.lens_radiance(cam, e[:5], lens, npix, first, count, spp, int(max_bounce), state=state)
        n = st["n"].copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = st["sum"] / n.astype(np.float32)[:, None]
        rgb = np.fmax(np.fmin(mean, np.float32(1.0)), np.float32(0.0))   # Raytracing.cl:211-220: NaN goes to 1
        return {"rgb": rgb, "sum": st["sum"].copy(), "n": n, "state": st}

    @staticmethod
    def lens_state(npix, first=0, count=None, device="cuda"):
        """The records a lens frame starts from, as a torch int32 ``[count, 8]`` tensor for ``lens_frame``'s device
        form: ``sum = 0``, ``n = 0`` and the frame's seeds ``(i % npix, i / npix)``.  Resuming these is the fresh
        call, bit for bit, so a device-resident loop passes this tensor to its first ``lens_frame`` and the same
        tensor to every later one."""
        import torch
        npix, first = int(npix), int(first)
        count = npix - first if count is None else int(count)
        if npix < 1 or first < 0 or count < 0 or first + count > npix:
            raise ValueError(f"pixels {first} .. +{count} outside the frame of {npix}")
        state = torch.zeros((count, 8), dtype=torch.int32, device=device)
        i = torch.arange(first, first + count, dtype=torch.int64, device=device)
        state[:, 4] = (i % npix).to(torch.int32)
        state[:, 5] = (i // npix).to(torch.int32)
        state[:, 3] = torch.tensor(1000.0, dtype=torch.float32).view(torch.int32).item()   # k of a miss
        state[:, 6] = -1
        return state

    def launch_ImgProcessing(self, h_src, h_out, SIZE):
        """Gamma 2.2 of ``ImgProcessing.cl``: ``h_out[k] = min(h_src[k], 1) ** 2.2`` for ``k < 3*SIZE*SIZE``."""
        src = _native.f32(h_src).reshape(-1)
        if not isinstance(h_out, np.ndarray) or h_out.dtype != np.float32 or not h_out.flags.c_contiguous:
            raise TypeError("h_out must be a C-contiguous float32 numpy array")
        n = min(int(SIZE) * int(SIZE) * 3, src.size, h_out.size)
        if n > 0:
            res = self._ctx.gamma(src[:n])
            h_out.reshape(-1)[:n] = res

    def close(self) -> None:
        self._ctx.close()

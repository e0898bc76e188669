"""Denoised previews without a GPU: the entry points are declared, exported and bound with the signatures of
rt_api.h, the params struct has the C layout, a NULL context is refused before any device call, the Python
layer checks its arguments -- and the numpy restatement of the filter (tests/denoise_ref.py), which is the GPU
tests' oracle, has the properties the definition promises."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from tests import denoise_ref as R
from ensem3a_openclraytracer_amd.KernelLauncher import Progressive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {
    "rt_accum_guides": "(rt_ctx* ctx, float* out)",
    "rt_accum_guides_device": "(rt_ctx* ctx, int device_index, float* d_guides, void* stream)",
    "rt_denoise_device": "(rt_ctx* ctx, int device_index, const float* d_rgb, const float* d_guides, int64_t npix, "
                         "int width, const rt_denoise_params* params, float* d_out, void* stream)",
    "rt_accum_denoise": "(rt_ctx* ctx, const rt_denoise_params* params, float* out_rgb)",
}


def test_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rt_api.h")).read())
    lib = _native.lib()
    c_p, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    kinds = {"rt_ctx*": c_p, "void*": c_p, "float*": c_p, "const float*": c_p, "int": i32, "int64_t": i64,
             "const rt_denoise_params*": ctypes.POINTER(_native.DenoiseParams)}
    for name, args in NEW.items():
        assert "int %s%s;" % (name, args) in header, name
        assert name in _native.EXPORTED
        fn = getattr(lib, name)
        want = [kinds[a.rsplit(" ", 1)[0]] for a in args.strip("()").split(", ")]
        assert fn.restype is i32 and list(fn.argtypes) == want, name


def test_params_struct_has_the_c_layout_and_the_defaults():
    header = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} rt_denoise_params;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["int passes", "int normal_squarings",
                                                                 "float sigma_c, sigma_p"]
    P = _native.DenoiseParams
    assert ctypes.sizeof(P) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("passes", 0), ("normal_squarings", 4),
                                                                  ("sigma_c", 8), ("sigma_p", 12)]
    p = P()
    assert (p.passes, p.normal_squarings, p.sigma_c, p.sigma_p) == (5, 5, 1.5, np.float32(0.02))
    assert R.DEFAULTS == dict(passes=5, normal_squarings=5, sigma_c=1.5, sigma_p=0.02)
    sig = inspect.signature(Progressive.denoised).parameters
    assert {k: sig[k].default for k in R.DEFAULTS} == R.DEFAULTS and sig["out"].default is None
    assert list(inspect.signature(Progressive.guides).parameters) == ["self"]


def test_a_null_context_is_an_argument_error():
    lib = _native.lib()
    buf = np.zeros(12, np.float32)
    assert lib.rt_accum_guides(None, buf.ctypes.data) == _native.RT_ERR_ARG
    assert lib.rt_accum_guides_device(None, 0, buf.ctypes.data, None) == _native.RT_ERR_ARG
    assert lib.rt_denoise_device(None, 0, buf.ctypes.data, buf.ctypes.data, 1, 1, None, buf.ctypes.data,
                                 None) == _native.RT_ERR_ARG
    assert lib.rt_accum_denoise(None, None, buf.ctypes.data) == _native.RT_ERR_ARG
    assert not buf.any()


class _Recorder:
    def __init__(self, npix):
        self.calls = []
        self.g = np.arange(12 * npix, dtype=np.float32).reshape(npix, 12)

    def accum_guides(self):
        self.calls.append(("guides",))
        return self.g

    def accum_denoise(self, params, out=None):
        self.calls.append(("denoise", params.passes, params.normal_squarings, params.sigma_c, params.sigma_p, out.size))


def test_python_layer():
    ctx = _Recorder(16)
    p = Progressive(ctx, 16)
    g = p.guides()
    assert sorted(g) == ["albedo", "depth", "filterable_samples", "material", "normal", "position"]
    assert g["normal"].shape == g["position"].shape == g["albedo"].shape == (16, 3) and g["depth"].shape == (16,)
    assert g["material"].dtype == g["filterable_samples"].dtype == np.int32
    for key, col in (("normal", 0), ("depth", 3), ("position", 4), ("albedo", 8)):
        assert np.shares_memory(g[key], ctx.g) and g[key].reshape(16, -1)[2, 0] == ctx.g[2, col]
    np.testing.assert_array_equal(g["filterable_samples"].view(np.float32), ctx.g[:, 7])
    np.testing.assert_array_equal(g["material"].view(np.float32), ctx.g[:, 11])
    out = p.denoised()
    assert out.dtype == np.float32 and out.size == 48
    p.denoised(2, 0, 0.5, 0.25, out=out)
    assert ctx.calls[1:] == [("denoise", 5, 5, 1.5, np.float32(0.02), 48), ("denoise", 2, 0, 0.5, 0.25, 48)]
    n = len(ctx.calls)
    for bad in (dict(passes=0), dict(passes=9), dict(normal_squarings=-1), dict(normal_squarings=9), dict(sigma_c=0.0),
                dict(sigma_c=-1.0), dict(sigma_p=float("nan")), dict(sigma_p=float("inf")), dict(sigma_c=float("nan"))):
        with pytest.raises(ValueError):
            p.denoised(**bad)
    with pytest.raises((TypeError, ValueError)):
        p.denoised(out=np.zeros(48, np.float64))
    with pytest.raises(ValueError):
        p.denoised(out=np.zeros(47, np.float32))
    assert len(ctx.calls) == n
    p._open = False
    for call in (p.guides, p.denoised):
        with pytest.raises(RuntimeError):
            call()


# ---- the restatement's own invariants ----
def _plane(w, h, rng, s=4, split_normals=False):
    """A wall facing the camera at depth 2: albedo (0.8, 0.5, 0.2), noisy radiance around 0.5 albedo."""
    n = w * h
    g = np.zeros((n, 12), np.float32)
    x = (np.arange(n) % w).astype(np.float32)
    y = (np.arange(n) // w).astype(np.float32)
    g[:, 0:3] = (0, 0, 1)
    if split_normals:
        g[x >= w // 2, 0:3] = (1, 0, 0)
    g[:, 3] = 2.0
    g[:, 4], g[:, 5], g[:, 6] = x * 0.01, y * 0.01, 2.0
    g[:, 7] = np.full(n, s, np.int32).view(np.float32)
    g[:, 8:11] = (0.8, 0.5, 0.2)
    g[:, 11] = np.zeros(n, np.int32).view(np.float32)
    rgb = (g[:, 8:11] * (0.5 + 0.2 * rng.standard_normal((n, 1)))).astype(np.float32).clip(0, 1)
    return rgb, g


def test_restatement_smooths_a_flat_wall_and_stays_in_range():
    rgb, g = _plane(40, 30, np.random.default_rng(1))
    out = R.denoise(rgb, g, 1200, 40)
    assert out.dtype == np.float32 and out.shape == (1200, 3)
    assert out.min() >= 0 and out.max() <= 1
    assert out[:, 0].std() < 0.5 * rgb[:, 0].std()
    assert abs(float(out[:, 0].mean()) - float(rgb[:, 0].mean())) < 0.02


def test_restatement_passes_unfilterable_pixels_through_and_never_reads_them():
    rng = np.random.default_rng(2)
    rgb, g = _plane(33, 20, rng)
    off = rng.random(660) < 0.3
    g[off, 7] = 0
    out = R.denoise(rgb, g, 660, 33)
    np.testing.assert_array_equal(out[off].view(np.uint32), rgb[off].view(np.uint32))
    assert (out[~off] != rgb[~off]).any()
    rgb2 = rgb.copy()
    rgb2[off] = 1.0 - rgb2[off]
    out2 = R.denoise(rgb2, g, 660, 33)
    np.testing.assert_array_equal(out2[~off].view(np.uint32), out[~off].view(np.uint32))


def test_restatement_does_not_mix_across_a_normal_edge():
    rng = np.random.default_rng(3)
    rgb, g = _plane(32, 16, rng, split_normals=True)
    left = (np.arange(512) % 32) < 16
    out = R.denoise(rgb, g, 512, 32)
    rgb2 = rgb.copy()
    rgb2[~left] = rgb2[~left][::-1]
    out2 = R.denoise(rgb2, g, 512, 32)
    np.testing.assert_array_equal(out2[left].view(np.uint32), out[left].view(np.uint32))
    assert (out2[~left] != out[~left]).any()


@pytest.mark.parametrize("w,h,npix", [(1, 1, 1), (3, 2, 6), (7, 5, 31)])
def test_restatement_on_frames_smaller_than_the_stencil(w, h, npix):
    """Taps that leave the frame, or land past npix, have no weight: no pixel past npix is ever read."""
    rgb, g = _plane(w, h, np.random.default_rng(4))
    out = R.denoise(rgb[:npix], g[:npix], npix, w)
    rgb2 = rgb.copy()
    rgb2[npix:] = 0.9
    out2 = R.denoise(rgb2, g, npix, w)
    np.testing.assert_array_equal(out.view(np.uint32), out2.view(np.uint32))
    if npix == 1:   # the centre tap alone: x' = (h x) / h, then remodulated
        x = rgb[0] / g[0, 8:11]
        h9 = np.float32(0.375) * np.float32(0.375)
        want = np.maximum(np.minimum(((h9 * x) / h9) * g[0, 8:11], np.float32(1)), np.float32(0))
        np.testing.assert_array_equal(out[0].view(np.uint32), want.astype(np.float32).view(np.uint32))


def test_restatement_colour_bandwidth_narrows_with_the_sample_count():
    rng = np.random.default_rng(5)
    rgb, g4 = _plane(40, 30, rng, s=4)
    g64 = g4.copy()
    g64[:, 7] = np.full(1200, 1024, np.int32).view(np.float32)
    d4 = np.abs(R.denoise(rgb, g4, 1200, 40) - rgb).mean()
    d64 = np.abs(R.denoise(rgb, g64, 1200, 40) - rgb).mean()
    assert d64 < d4

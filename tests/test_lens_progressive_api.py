"""Progressive lens frames, host side (no GPU): rt_accum_begin_lens and rt_accum_begin_lens_device are declared in
rt_api.h, exported and bound with the header's argument types; rt_debug_accum_state is declared in rt_debug.h (not in
rt_api.h) and bound; KernelLauncher.begin_progressive_lens refuses a bad lens before anything native is touched and
takes begin_progressive's arguments plus the lens; begin_progressive keeps its signature."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher, Progressive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "rt_accum_begin_lens": "(rt_ctx* ctx, const float cam[10], const float env[5], const rt_lens* lens, int64_t npix, "
                           "int max_bounce)",
    "rt_accum_begin_lens_device": "(rt_ctx* ctx, int device_index, const float cam[10], const float env[5], "
                                  "const rt_lens* lens, int64_t npix, int max_bounce, int row0, int row_step)",
}
BEGIN_PROGRESSIVE = ["self", "h_vertex_p", "h_vertex_n", "h_vertex_uv", "h_face_data", "h_material_data",
                     "h_light_data", "h_BVH", "h_cam", "h_envData", "imgDim", "maxBounce", "h_IBL"]


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"\s+", " ", f.read())


def _kind(arg):
    c_p, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    return c_p if "*" in arg or "[" in arg else {"int": i32, "int64_t": i64}[arg.rsplit(" ", 1)[0]]


def test_begin_lens_is_declared_exported_and_bound():
    header = _header("rt_api.h")
    lib = _native.lib()
    for name, args in NEW.items():
        assert "int %s%s;" % (name, args) in header, name
        assert name in _native.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int, name
        assert list(fn.argtypes) == [_kind(a) for a in args.strip("()").split(", ")], name
    # the begin of a lens accumulation is the plain begin's arguments with the lens behind env
    plain = list(_native.lib().rt_accum_begin.argtypes)
    assert list(lib.rt_accum_begin_lens.argtypes) == plain[:3] + [ctypes.c_void_p] + plain[3:]
    plain = list(_native.lib().rt_accum_begin_device.argtypes)
    assert list(lib.rt_accum_begin_lens_device.argtypes) == plain[:4] + [ctypes.c_void_p] + plain[4:]


def test_the_state_read_out_is_a_debug_entry_point():
    assert "int rt_debug_accum_state(rt_ctx* ctx, rt_radiance_state* out" in _header("rt_debug.h")
    assert "rt_debug_accum_state" not in _header("rt_api.h")
    assert "rt_debug_accum_state" in _native.EXPORTED
    fn = _native.lib().rt_debug_accum_state
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_void_p]
    assert callable(_native.Context.debug_accum_state) and callable(_native.Context.accum_begin_lens)
    assert _native.RADIANCE_STATE_DTYPE.itemsize == 32


def test_the_header_says_which_options_apply():
    header = _header("rt_api.h")
    block = header[header.index("Progressive lens frames"):header.index("int rt_accum_begin_lens(")]
    for contract in ("E1", "E2", "E3"):
        assert contract in block
    for option in ('"block"', '"radiance_grid"', '"slices"', '"pilot"', '"spec"', '"team"', '"walk_team"',
                   '"bvh_width"'):
        assert option in block, option
    assert "do not" in block and "8 bytes per pixel" in block


class _NoNative:
    """Stands where the launcher keeps its context: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the native layer was touched ({name}) before the lens was checked")


def test_begin_progressive_lens_refuses_a_bad_lens_before_anything_native(monkeypatch):
    kl = KernelLauncher.__new__(KernelLauncher)   # no context: there is no GPU here
    kl._ctx = _NoNative()
    monkeypatch.setattr(_native, "_lib", _NoNative())   # ... and the library handle itself is a stub
    cam = np.array([0, -3.5, 0, 0, 0, 0, 5, 4, 1, 0.785], np.float32)
    env = np.zeros(5, np.float32)
    inf, nan = float("inf"), float("nan")
    bad = [dict(jitter=-0.5), dict(jitter=nan), dict(jitter=inf), dict(jitter=-inf),
           dict(aperture=-1e-3), dict(aperture=nan), dict(aperture=inf),
           dict(focus=0.0), dict(focus=-1.0), dict(focus=nan), dict(focus=inf),
           dict(seed=-1), dict(seed=2 ** 32)]
    for change in bad:
        lens = dict(jitter=1.0, aperture=0.0, focus=1.0, seed=0)
        lens.update(change)
        with pytest.raises(ValueError):
            kl.begin_progressive_lens(None, None, None, None, None, None, None, cam, env, 20, 4, None, **lens)
    with pytest.raises(ValueError):   # begin_progressive's own checks come first as well
        kl.begin_progressive_lens(None, None, None, None, None, None, None, cam[:9], env, 20, 4, None)
    # a good lens goes on to the native layer: the stub is what stops it
    kl._scene_key = None
    f, i = np.zeros(9, np.float32), np.zeros(10, np.int32)
    with pytest.raises(AssertionError, match="native layer was touched"):
        kl.begin_progressive_lens(f, f, f[:2], i, f[:6], None, f, cam, env, 20, 4, None, jitter=0.0)


def test_signatures():
    plain = inspect.signature(KernelLauncher.begin_progressive)
    assert list(plain.parameters) == BEGIN_PROGRESSIVE
    assert all(p.default is inspect.Parameter.empty for p in plain.parameters.values())
    lens = inspect.signature(KernelLauncher.begin_progressive_lens)
    assert list(lens.parameters) == BEGIN_PROGRESSIVE + ["jitter", "aperture", "focus", "seed"]
    got = {k: lens.parameters[k].default for k in ("jitter", "aperture", "focus", "seed")}
    assert got == dict(jitter=1.0, aperture=0.0, focus=1.0, seed=0)
    # it returns the existing class, which gained no method for it
    assert lens.return_annotation == plain.return_annotation
    assert str(lens.return_annotation).strip("'\"") == "Progressive" or lens.return_annotation is Progressive
    assert not [m for m in vars(Progressive) if "lens" in m.lower()]

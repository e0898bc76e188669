"""Radiance queries, host side (no GPU): the entry points are declared, exported and bound; rt_radiance_state is the
32-byte record of the header and _native's dtype matches it field by field; the ray packing carries the seeds' bits;
KernelLauncher.radiance refuses bad inputs before anything native is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "rt_radiance": "(rt_ctx* ctx, const float* rays, int64_t n, const float env[5], int spp, int max_bounce, int flags, "
                   "rt_radiance_state* state)",
    "rt_radiance_device": "(rt_ctx* ctx, int device_index, const float* d_rays, int64_t n, const float env[5], int spp, "
                          "int max_bounce, int flags, rt_radiance_state* d_state, void* stream)",
    "rt_camera_rays": "(rt_ctx* ctx, const float cam[10], int64_t npix, int64_t first, int64_t count, float* rays)",
    "rt_camera_rays_device": "(rt_ctx* ctx, int device_index, const float cam[10], int64_t npix, int64_t first, "
                             "int64_t count, float* d_rays, void* stream)",
}


def _header():
    with open(os.path.join(ROOT, "include", "rt_api.h")) as f:
        return f.read()


def test_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"\s+", " ", _header())
    lib = _native.lib()
    c_p, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64

    def kind(arg):
        return c_p if "*" in arg or "[" in arg else {"int": i32, "int64_t": i64}[arg.rsplit(" ", 1)[0]]

    for name, args in NEW.items():
        assert "int %s%s;" % (name, args) in header, name
        assert name in _native.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is i32 and list(fn.argtypes) == [kind(a) for a in args.strip("()").split(", ")], name
    assert re.search(r"enum \{ RT_RADIANCE_RESUME = 1 \};", header) and _native.RT_RADIANCE_RESUME == 1
    m = re.search(r"#define RT_ACCUM_MAX_SAMPLES \(1 << (\d+)\)", header)
    assert m and _native.RT_ACCUM_MAX_SAMPLES == 1 << int(m.group(1))


def test_state_dtype_is_the_headers_record(tmp_path):
    m = re.search(r"typedef struct \{([^}]*)\} rt_radiance_state;", _header())
    assert m, "rt_radiance_state is not declared"
    fields = []   # (C type, name, count)
    for t, names in re.findall(r"(float|uint32_t|int32_t)\s+([^;]+);", m.group(1)):
        for n in names.split(","):
            a = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", n)
            fields.append((t, a.group(1), int(a.group(2) or 1)))
    assert fields == [("float", "sum", 3), ("float", "k", 1), ("uint32_t", "seed0", 1), ("uint32_t", "seed1", 1),
                      ("int32_t", "tri", 1), ("int32_t", "n", 1)]
    dt = _native.RADIANCE_STATE_DTYPE
    want = {"float": np.float32, "uint32_t": np.uint32, "int32_t": np.int32}
    assert dt.itemsize == 32 and list(dt.names) == [n for _, n, _ in fields]
    off = 0
    for t, n, count in fields:
        assert dt.fields[n][0].base == want[t] and dt.fields[n][0].shape == ((count,) if count > 1 else ()), n
        assert dt.fields[n][1] == off, n
        off += 4 * count
    assert off == 32
    # ... and the C compiler lays the header's struct out the same way
    tu = tmp_path / "state.c"
    checks = "\n".join(f"_Static_assert(offsetof(rt_radiance_state, {n}) == {dt.fields[n][1]}, \"{n}\");" for n in dt.names)
    tu.write_text('#include <stddef.h>\n#include "rt_api.h"\n_Static_assert(sizeof(rt_radiance_state) == 32, "size");\n'
                  f"{checks}\nint main(void) {{ return 0; }}\n")
    r = subprocess.run(["gcc", "-x", "c", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_ray_packing_carries_the_seed_bits():
    o = np.arange(9, dtype=np.float64).reshape(3, 3)
    d = -np.arange(9, dtype=np.float64).reshape(3, 3) - 1
    seeds = np.array([[0, 1], [0xffffffff, 0x7fc00000], [0x3f800000, 0x80000000]], np.uint32)
    r = _native.pack_radiance_rays(o, d, seeds)
    assert r.dtype == np.float32 and r.shape == (3, 8) and r.flags.c_contiguous
    np.testing.assert_array_equal(r[:, 0:3], d.astype(np.float32))
    np.testing.assert_array_equal(r[:, 3:6], o.astype(np.float32))
    np.testing.assert_array_equal(r.view(np.uint32)[:, 6:8], seeds)   # words 6 and 7: the bits, NaN patterns included
    # the default: (ray index, 0), the frame's decorrelation
    r = _native.pack_radiance_rays(np.zeros((300, 3)), np.ones((300, 3)))
    np.testing.assert_array_equal(r.view(np.uint32)[:, 6], np.arange(300, dtype=np.uint32))
    assert (r.view(np.uint32)[:, 7] == 0).all()
    # signed integers keep their low 32 bits
    r = _native.pack_radiance_rays(o, d, np.array([[-1, 2], [3, 4], [5, 6]], np.int64))
    assert r.view(np.uint32)[0, 6] == 0xffffffff and r.view(np.uint32)[2, 7] == 6
    assert _native.pack_radiance_rays(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 8)
    with pytest.raises(ValueError):
        _native.pack_radiance_rays(o, d[:2])
    with pytest.raises(ValueError):
        _native.pack_radiance_rays(o, d, seeds[:2])
    with pytest.raises(ValueError):
        _native.pack_radiance_rays(o, d, seeds[:, :1])
    with pytest.raises(TypeError):
        _native.pack_radiance_rays(o, d, seeds.astype(np.float32))


class _NoNative:
    """Stands where the launcher keeps its context: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the native layer was touched ({name}) before the inputs were checked")


def test_launcher_refuses_bad_inputs_before_anything_native():
    kl = KernelLauncher.__new__(KernelLauncher)   # no context: there is no GPU here
    kl._ctx = _NoNative()
    o, d, env = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32), np.zeros(5, np.float32)
    state = np.zeros(4, _native.RADIANCE_STATE_DTYPE)
    bad = [
        (ValueError, dict(origins=np.zeros((4, 2)))),                       # shapes
        (ValueError, dict(directions=np.zeros(12))),
        (ValueError, dict(origins=np.zeros((2, 2, 3)))),
        (ValueError, dict(directions=np.ones((3, 3)))),                     # counts that differ
        (ValueError, dict(spp=0)),
        (ValueError, dict(spp=-1)),
        (ValueError, dict(env=np.zeros(4))),
        (ValueError, dict(seeds=np.zeros((3, 2), np.uint32))),
        (ValueError, dict(seeds=np.zeros(4, np.uint32))),
        (TypeError, dict(seeds=np.zeros((4, 2), np.float32))),
        (ValueError, dict(state=state[:3])),                                # a state of the wrong length
        (TypeError, dict(state=np.zeros((4, 8), np.float32))),              # ... or dtype
        (TypeError, dict(state=[0] * 4)),
    ]
    for exc, change in bad:
        args = dict(origins=o, directions=d, spp=2, max_bounce=4, env=env, seeds=None, state=None)
        args.update(change)
        with pytest.raises(exc):
            kl.radiance(**args)
    with pytest.raises(ValueError):
        kl.camera_rays(np.zeros(9), 16)

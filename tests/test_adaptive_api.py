"""Adaptive sampling without a GPU: the entry points are declared, exported and bound with the signatures of
rt_api.h, and the Python layer checks its arguments and runs ``refine`` as documented (against a recording
stand-in for the native context)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd.KernelLauncher import Progressive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {
    "rt_accum_mark": "(rt_ctx* ctx)",
    "rt_accum_select": "(rt_ctx* ctx, float threshold, int64_t* n_selected)",
    "rt_accum_select_mask": "(rt_ctx* ctx, const uint8_t* mask)",
    "rt_accum_select_all": "(rt_ctx* ctx)",
    "rt_accum_selection": "(rt_ctx* ctx, uint8_t* mask_out)",
    "rt_accum_sample_map": "(rt_ctx* ctx, int32_t* out)",
    "rt_accum_add_selected": "(rt_ctx* ctx, int spp, float* out_rgb)",
    "rt_accum_mark_device": "(rt_ctx* ctx, int device_index, void* stream)",
    "rt_accum_select_device": "(rt_ctx* ctx, int device_index, float threshold, void* stream)",
    "rt_accum_select_mask_device": "(rt_ctx* ctx, int device_index, const uint8_t* d_mask, void* stream)",
    "rt_accum_select_all_device": "(rt_ctx* ctx, int device_index, void* stream)",
    "rt_accum_add_selected_device": "(rt_ctx* ctx, int device_index, int spp, float* d_out, void* stream)",
}


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    lib = _native.lib()
    c_p, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    kinds = {"rt_ctx*": c_p, "void*": c_p, "float*": c_p, "int32_t*": c_p, "uint8_t*": c_p, "const uint8_t*": c_p,
             "int": i32, "float": f32, "int64_t*": ctypes.POINTER(ctypes.c_int64)}
    for name, args in NEW.items():
        assert re.search(r"\bint %s%s;" % (name, re.escape(args)), header), name
        assert name in _native.EXPORTED
        fn = getattr(lib, name)
        want = [kinds[a.rsplit(" ", 1)[0]] for a in args.strip("()").split(", ")]
        assert fn.restype is i32 and list(fn.argtypes) == want, name


def test_python_signatures():
    sig = {n: list(inspect.signature(getattr(Progressive, n)).parameters)[1:]
           for n in ("mark", "select", "select_mask", "select_all", "selection", "sample_map", "add_selected", "refine")}
    assert sig == {"mark": [], "select": ["threshold"], "select_mask": ["mask"], "select_all": [], "selection": [],
                   "sample_map": [], "add_selected": ["spp", "out"], "refine": ["threshold", "min_spp", "max_spp", "out"]}
    assert inspect.signature(Progressive.refine).parameters["out"].default is None
    for n in ("accum_mark", "accum_select", "accum_select_mask", "accum_select_all", "accum_selection",
              "accum_sample_map", "accum_add_selected", "accum_mark_device", "accum_select_device",
              "accum_select_mask_device", "accum_select_all_device", "accum_add_selected_device"):
        assert callable(getattr(_native.Context, n)), n


class _Recorder:
    """Stands in for _native.Context: records the calls, and answers select from a list."""

    def __init__(self, selected):
        self.calls = []
        self.selected = list(selected)

    def accum_add(self, spp, out=None):
        self.calls.append(("add", spp))

    def accum_add_selected(self, spp, out=None):
        self.calls.append(("add_selected", spp))

    def accum_mark(self):
        self.calls.append(("mark",))

    def accum_select(self, threshold):
        self.calls.append(("select", threshold))
        return self.selected.pop(0)

    def accum_select_mask(self, mask):
        self.calls.append(("select_mask", np.asarray(mask).shape))


def test_refine_is_the_documented_sequence():
    ctx = _Recorder([10, 7, 3, 1])
    p = Progressive(ctx, 16)
    out = p.refine(0.02, 4, 32)
    assert out.dtype == np.float32 and out.size == 48
    assert ctx.calls == [("add", 4), ("mark",), ("add", 4), ("select", 0.02),
                         ("mark",), ("add_selected", 8), ("select", 0.02),
                         ("mark",), ("add_selected", 16), ("select", 0.02)]
    # an empty selection ends it; the last step is cut at max_spp
    ctx = _Recorder([5, 0])
    Progressive(ctx, 16).refine(0.5, 2, 64)
    assert ctx.calls[4:] == [("mark",), ("add_selected", 4), ("select", 0.5)]
    ctx = _Recorder([5, 5, 5])
    Progressive(ctx, 16).refine(0.5, 4, 20)
    assert [c for c in ctx.calls if c[0] == "add_selected"] == [("add_selected", 8), ("add_selected", 4)]
    ctx = _Recorder([5])
    Progressive(ctx, 16).refine(0.5, 4, 8)   # already at max_spp after the two full adds
    assert ctx.calls == [("add", 4), ("mark",), ("add", 4), ("select", 0.5)]


def test_python_argument_checks():
    ctx = _Recorder([1])
    p = Progressive(ctx, 16)
    with pytest.raises(ValueError):
        p.refine(0.02, 0, 32)
    with pytest.raises(ValueError):
        p.refine(0.02, 4, 7)
    with pytest.raises(ValueError):
        p.select(float("nan"))
    with pytest.raises(ValueError):
        p.select_mask(np.zeros(15, np.uint8))
    with pytest.raises((TypeError, ValueError)):
        p.add_selected(1, out=np.zeros(48, np.float64))
    with pytest.raises(ValueError):
        p.add_selected(1, out=np.zeros(47, np.float32))
    with pytest.raises((TypeError, ValueError)):
        p.refine(0.02, 4, 32, out=np.zeros(48, np.float64))
    assert ctx.calls == []
    p.select_mask(np.zeros((4, 4), bool))
    assert ctx.calls == [("select_mask", (4, 4))]
    p._open = False   # closed, or replaced by a later begin_progressive
    for call in (p.mark, p.select_all, p.selection, p.sample_map, lambda: p.select(0.1), lambda: p.add_selected(1),
                 lambda: p.select_mask(np.zeros(16)), lambda: p.refine(0.02, 4, 32)):
        with pytest.raises(RuntimeError):
            call()

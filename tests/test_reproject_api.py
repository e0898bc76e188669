"""Temporal reprojection without a GPU: the entry points are declared, exported and bound with the signatures of
rt_api.h, the params struct has the C layout, rt_reproject_basis inverts the CPU oracle's camera ray, a NULL
context is refused before any device call, the Python layer checks its arguments -- and the numpy restatement of
the definition (tests/reproject_ref.py), which is the GPU tests' oracle, has the properties the definition promises."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd.KernelLauncher import History, Progressive
from tests import reproject_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

NEW = {
    "rt_reproject_basis": "(const float cam[10], float basis[16])",
    "rt_reproject_device": "(rt_ctx* ctx, int device_index, const float* d_prev_rgb, const float* d_prev_guides, "
                           "const float prev_cam[10], const float* d_cur_rgb, const float* d_cur_guides, int64_t npix, "
                           "int width, const rt_reproject_params* params, float* d_out_rgb, float* d_out_guides, "
                           "void* stream)",
    "rt_accum_reproject": "(rt_ctx* ctx, const float* prev_rgb, const float* prev_guides, const float prev_cam[10], "
                          "const rt_reproject_params* params, float* out_rgb, float* out_guides)",
    "rt_denoise": "(rt_ctx* ctx, const float* rgb, const float* guides, int64_t npix, int width, "
                  "const rt_denoise_params* params, float* out_rgb)",
}


def test_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rt_api.h")).read())
    lib = _native.lib()
    c_p, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    kinds = {"rt_ctx*": c_p, "void*": c_p, "float*": c_p, "const float*": c_p, "const float": c_p, "float": c_p,
             "int": i32, "int64_t": i64, "const rt_reproject_params*": ctypes.POINTER(_native.ReprojectParams),
             "const rt_denoise_params*": ctypes.POINTER(_native.DenoiseParams)}
    for name, args in NEW.items():
        assert "int %s%s;" % (name, args) in header, name
        assert name in _native.EXPORTED
        fn = getattr(lib, name)
        want = [kinds[a.rsplit(" ", 1)[0]] for a in args.strip("()").split(", ")]   # (an array argument: a pointer)
        assert fn.restype is i32 and list(fn.argtypes) == want, name
    assert "rt_reproject_basis" in _native.HOST_ONLY


def test_params_struct_has_the_c_layout_and_the_defaults():
    header = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} rt_reproject_params;", header).group(1)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["float sigma_p, normal_min, max_history, min_weight"]
    P = _native.ReprojectParams
    assert ctypes.sizeof(P) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("sigma_p", 0), ("normal_min", 4),
                                                                  ("max_history", 8), ("min_weight", 12)]
    p = P()
    assert (p.sigma_p, p.normal_min, p.max_history, p.min_weight) == (F(0.02), F(0.9), 64.0, 0.25)
    assert R.DEFAULTS == dict(sigma_p=0.02, normal_min=0.9, max_history=64.0, min_weight=0.25)
    sig = inspect.signature(Progressive.reprojected).parameters
    assert {k: sig[k].default for k in R.DEFAULTS} == R.DEFAULTS
    assert (sig["denoise"].default, sig["out"].default, sig["return_history"].default) == (False, None, False)
    assert list(inspect.signature(Progressive.history).parameters) == ["self"]


# ---- rt_reproject_basis against the CPU oracle's camera ray ----
CAMS = [(64, [0.0, -3.5, 1.0, 0.0, 0.0, 0.0, 64, 64, 1, 0.6]),
        (37, [0.4, -2.0, 0.7, 12.0, -7.0, 31.0, 37, 20, 1, 0.9]),
        (5, [-1.5, 0.3, 2.0, -40.0, 25.0, 170.0, 5, 7, 1, 1.2])]


def _pixels(W, npix):
    spread = np.linspace(0, npix - 1, 23).astype(np.int64)
    always = [0, 1, W - 2, W - 1, W, npix - 1]
    return sorted(set(int(i) for i in list(spread) + always if 0 <= i < npix))


@pytest.mark.parametrize("W,cam", CAMS, ids=["w64", "w37_rotated", "w5_rotated"])
def test_basis_inverts_the_oracles_camera_ray(W, cam):
    cam = np.asarray(cam, F)
    npix = W * int(cam[7])
    basis = _native.reproject_basis(cam)
    assert basis.dtype == F and basis.shape == (16,)
    np.testing.assert_array_equal(basis[9:12], cam[0:3])
    assert basis[13] == cam[6] and basis[14] == 0 and basis[15] == 0
    M = basis[:9].reshape(3, 3).astype(np.float64)
    np.testing.assert_allclose(M @ M.T, np.eye(3), atol=1e-5)
    for j in range(3):   # column j: e_j through the three rotations undone, z first
        e = np.eye(3, dtype=F)[j]
        e = O.rotate(-(cam[5] * F(F(3.14) / F(180.0))), [0, 0, 1], e)
        e = O.rotate(-(cam[4] * F(F(3.14) / F(180.0))), [0, 1, 0], e)
        e = O.rotate(-(cam[3] * F(F(3.14) / F(180.0))), [1, 0, 0], e)
        np.testing.assert_array_equal(basis[j:9:3].view(np.uint32), e.view(np.uint32), err_msg=f"column {j}")
    pix = _pixels(W, npix)
    pts = np.zeros((len(pix), 3), F)
    for n, i in enumerate(pix):
        ray = O.camera_ray(cam, i)
        pts[n] = ray[3:6] + ray[0:3] * F(2.7)
    ly, u, vv = R.project(basis, pts)
    assert (ly > 0).all()
    worst = 0.0
    for n, i in enumerate(pix):
        cu, cv = int(round(float(u[n]))), int(round(float(vv[n])))
        worst = max(worst, abs(float(u[n]) - cu), abs(float(vv[n]) - cv))
        assert abs(float(u[n]) - cu) < 0.05 and abs(float(vv[n]) - cv) < 0.05, (i, u[n], vv[n])
        assert (cv + 1) * W + cu - 1 == (i if i >= W - 1 else i + W), (i, cu, cv)
    print("W = %d: worst distance of (u, vv) from an integer %.2e" % (W, worst))


def test_basis_refuses_null_and_non_finite_cameras():
    H = _native.host_lib()
    out = np.zeros(16, F)
    cam = np.asarray(CAMS[0][1], F)
    assert H.rt_reproject_basis(None, out.ctypes.data) == _native.RT_ERR_ARG
    assert H.rt_reproject_basis(cam.ctypes.data, None) == _native.RT_ERR_ARG
    for k in (0, 5, 9):
        bad = cam.copy()
        bad[k] = np.nan if k else np.inf
        with pytest.raises(_native.NativeError):
            _native.reproject_basis(bad)
    assert not out.any()


def test_a_null_context_is_an_argument_error():
    lib = _native.lib()
    buf = np.zeros(16, F)
    cam = np.asarray(CAMS[0][1], F)
    p = buf.ctypes.data
    assert lib.rt_reproject_device(None, 0, p, p, cam.ctypes.data, p, p, 1, 64, None, p, p, None) == _native.RT_ERR_ARG
    assert lib.rt_reproject_device(None, 0, None, None, None, None, None, 0, 0, None, None, None,
                                   None) == _native.RT_ERR_ARG
    assert lib.rt_accum_reproject(None, p, p, cam.ctypes.data, None, p, p) == _native.RT_ERR_ARG
    assert lib.rt_denoise(None, p, p, 1, 1, None, p) == _native.RT_ERR_ARG
    assert not buf.any()


# ---- the Python layer ----
class _Recorder:
    def __init__(self, npix):
        self.calls = []
        self.n = npix
        self.g = np.arange(12 * npix, dtype=F).reshape(npix, 12)

    def accum_read(self, out=None):
        self.calls.append(("read",))
        out[:] = 0.25
        return out

    def accum_guides(self):
        self.calls.append(("guides",))
        return self.g

    def accum_reproject(self, rgb, guides, cam, params, out=None):
        self.calls.append(("reproject", params.sigma_p, params.normal_min, params.max_history, params.min_weight,
                           rgb.size, guides.size, float(cam[6])))
        return np.full(3 * self.n, 0.5, F), self.g + 1

    def denoise(self, rgb, guides, npix, width, params, out=None):
        self.calls.append(("denoise", npix, width, params.passes, params.sigma_p, float(rgb[0])))
        out[:] = 0.75
        return out


def test_python_layer():
    ctx = _Recorder(16)
    cam = np.arange(10, dtype=np.float64)
    cam[6] = 4
    p = Progressive(ctx, 16, cam)
    cam[0] = 99   # (the Progressive keeps its own copy)
    h = p.history()
    assert isinstance(h, History) and (h.imgDim, h.width) == (16, 4)
    assert h.rgb.dtype == F and h.rgb.size == 48 and h.guides.shape == (16, 12)
    assert h.cam.dtype == F and h.cam[0] == 0 and h.cam[6] == 4
    assert ctx.calls == [("read",), ("guides",)]
    out = p.reprojected(h)
    assert out.dtype == F and out.size == 48 and (out == 0.5).all()
    assert ctx.calls[2:] == [("reproject", F(0.02), F(0.9), 64.0, 0.25, 48, 192, 4.0)]
    buf = np.zeros(48, F)
    got, h2 = p.reprojected(h, sigma_p=0.05, normal_min=0.5, max_history=8, min_weight=0.0, denoise=True, out=buf,
                            return_history=True)
    assert got is buf and (buf == 0.75).all()
    assert isinstance(h2, History) and (h2.rgb == 0.5).all() and (h2.guides == ctx.g + 1).all() and h2.cam[6] == 4
    assert ctx.calls[3:] == [("reproject", F(0.05), 0.5, 8.0, 0.0, 48, 192, 4.0), ("denoise", 16, 4, 5, F(0.05), 0.5)]
    n = len(ctx.calls)
    for bad in (dict(sigma_p=0.0), dict(sigma_p=float("nan")), dict(max_history=0.0), dict(max_history=float("inf")),
                dict(normal_min=float("nan")), dict(min_weight=float("inf"))):
        with pytest.raises(ValueError):
            p.reprojected(h, **bad)
    with pytest.raises(TypeError):
        p.reprojected((h.rgb, h.guides))
    with pytest.raises(ValueError):
        p.reprojected(History(h.rgb[:45], h.guides[:15], h.cam, 15))
    with pytest.raises((TypeError, ValueError)):
        p.reprojected(h, out=np.zeros(48, np.float64))
    with pytest.raises(RuntimeError):
        Progressive(ctx, 16).history()
    assert len(ctx.calls) == n
    p._open = False
    for call in (p.history, lambda: p.reprojected(h)):
        with pytest.raises(RuntimeError):
            call()


# ---- the restatement's own invariants, on synthetic guides ----
def _wall(W, H, cam, f=4, depth=2.0, material=3):
    """A wall facing the camera `cam` (unrotated: it looks along +y) at `depth`: the guides of W x H pixels whose
    first hits are the camera rays' own points on it, albedo (0.8, 0.5, 0.2), and a smooth radiance."""
    cam = np.asarray(cam, F)
    n = W * H
    g = np.zeros((n, 12), F)
    gi = g.view(np.int32)
    for i in range(n):
        ray = O.camera_ray(cam, i)
        k = F(depth) / ray[1]
        g[i, 3] = k
        g[i, 4:7] = ray[3:6] + ray[0:3] * k
    g[:, 0:3] = (0, -1, 0)
    gi[:, 7] = f
    g[:, 8:11] = (0.8, 0.5, 0.2)
    gi[:, 11] = material
    rgb = (g[:, 8:11] * (F(0.3) + F(0.1) * g[:, 4:5])).astype(F)
    return rgb, g


CAM0 = np.asarray([0.0, -3.5, 1.0, 0.0, 0.0, 0.0, 12, 9, 1, 0.6], F)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_restatement_a_previous_camera_looking_away_gives_the_inputs_back():
    rgb, g = _wall(12, 9, CAM0)
    away = CAM0.copy()
    away[5] = 180.0
    out, og = R.reproject(rgb * F(0.5), g, _native.reproject_basis(away), rgb, g, 108, 12)
    np.testing.assert_array_equal(_bits(out), _bits(rgb))
    np.testing.assert_array_equal(_bits(og), _bits(g))


def test_restatement_static_camera_takes_the_pixels_own_history():
    rgb, g = _wall(12, 9, CAM0)
    prev = (rgb * F(0.5)).astype(F)
    out, og = R.reproject(prev, g, _native.reproject_basis(CAM0), rgb, g, 108, 12)
    f = og[:, 7].view(np.int32)
    assert (f[11:] >= 5).all() and (f[11:] <= 8).all()
    want = (prev * F(4) + rgb * F(4)) / F(8)
    np.testing.assert_allclose(out[11:], want[11:], rtol=2e-2)   # (neighbours at 1e-6 of a pixel: a smooth wall)
    keep = np.ones(12, bool)
    keep[7] = False
    np.testing.assert_array_equal(_bits(og)[:, keep], _bits(g)[:, keep])


@pytest.mark.parametrize("what", ["material", "normal", "plane"])
def test_restatement_rejects_taps_on_another_surface(what):
    rgb, g = _wall(12, 9, CAM0)
    basis = _native.reproject_basis(CAM0)
    pg = g.copy()
    if what == "material":
        pg.view(np.int32)[:, 11] = 4
    elif what == "normal":
        pg[:, 0:3] = (F(0.6), F(-0.8), 0)      # n_p . n_q = 0.8 < normal_min
    else:
        pg[:, 5] += F(0.02 * 3.5 * 1.5)        # |n_p . (P_q - P_p)| above sigma_p * k for every k here (k < 3.5)
        assert (g[:, 3] < 3.5).all()
    out, og = R.reproject(rgb * F(0.5), pg, basis, rgb, g, 108, 12)
    np.testing.assert_array_equal(_bits(out), _bits(rgb))
    np.testing.assert_array_equal(_bits(og), _bits(g))
    # ... and each is accepted once the threshold allows it
    loose = dict(normal=dict(normal_min=0.75), plane=dict(sigma_p=0.2)).get(what)
    if loose:
        out, og = R.reproject(rgb * F(0.5), pg, basis, rgb, g, 108, 12, **loose)
        assert (og[11:, 7].view(np.int32) > 4).all() and (_bits(out)[11:] != _bits(rgb)[11:]).any()


def test_restatement_caps_the_history():
    rgb, g = _wall(12, 9, CAM0, f=3)
    pg = g.copy()
    pg.view(np.int32)[:, 7] = 1000
    for mh in (64.0, 10.5):
        out, og = R.reproject(rgb, pg, _native.reproject_basis(CAM0), rgb, g, 108, 12, max_history=mh)
        np.testing.assert_array_equal(og[11:, 7].view(np.int32), int(F(mh) + F(3)))


def test_restatement_never_reads_past_npix_and_leaves_unfilterable_pixels():
    rgb, g = _wall(12, 9, CAM0)
    npix = 12 * 6 + 5
    off = np.arange(108) % 7 == 3
    g.view(np.int32)[off, 7] = 0
    basis = _native.reproject_basis(CAM0)
    prev = (rgb * F(0.5)).astype(F)
    out, og = R.reproject(prev[:npix], g[:npix], basis, rgb[:npix], g[:npix], npix, 12)
    prev2, g2 = prev.copy(), g.copy()
    prev2[npix:] = np.nan
    g2[npix:] = np.nan
    out2, og2 = R.reproject(prev2, g2, basis, rgb, g2, npix, 12)
    np.testing.assert_array_equal(_bits(out), _bits(out2))
    np.testing.assert_array_equal(_bits(og), _bits(og2))
    np.testing.assert_array_equal(_bits(out)[off[:npix]], _bits(rgb)[:npix][off[:npix]])
    np.testing.assert_array_equal(_bits(og)[off[:npix]], _bits(g)[:npix][off[:npix]])
    assert (og[:, 7].view(np.int32) > 4).any()

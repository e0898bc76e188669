"""Temporal reprojection (rt_reproject_device / rt_accum_reproject, Progressive.history / reprojected): the kernel is
its definition in rt_api.h bit for bit (tests/reproject_ref.py restates it in numpy float32), pixels without
history pass through, the outputs chain into the filter and into the next move, the host form is the device form,
and the result is closer to the converged frame than the frame it started from.

Every comparison but the last is exact: arrays are compared as their 32-bit words.
"""

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from tests import denoise_ref as D
from tests import reproject_ref as R
from tests.test_gpu_denoise import _bits, _converged, _inputs, _launcher, _same   # (and its cache of converged frames)

pytestmark = pytest.mark.gpu

STATE, ARG = _native.RT_ERR_STATE, _native.RT_ERR_ARG
F = np.float32
CASES = ["cornell_64_s4", "monkey_c3_64_s4", "serre_96x54_s4"]
OTHER = dict(sigma_p=0.08, normal_min=0.5, max_history=5.5, min_weight=0.6)


@pytest.fixture()
def pl():
    k = _launcher()
    yield k
    k.close()


@pytest.fixture(scope="module")
def ref_kl():
    """The launcher of the shared inputs and the converged frame (it holds no accumulation between tests)."""
    k = _launcher()
    yield k
    k.close()


def _moved(cam, dx=0.1, rz=2.0):
    """The previous camera: the case's, moved by dx in x and turned rz degrees about z."""
    c = np.array(cam, F)
    c[0] += F(dx)
    c[5] += F(rz)
    return c


def _render(kl, case, cam, spp, npix=None, lens=None):
    """(frame [npix, 3], guides [npix, 12]) of `spp` samples at `cam`; the accumulation stays open."""
    sc, _, env, n, _, mb, ibl = _inputs(case)
    args = (sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.BVH.exportArray, cam, env,
            npix or n, mb, ibl)
    p = kl.begin_progressive_lens(*args, *lens) if lens else kl.begin_progressive(*args)
    rgb = p.add(spp).reshape(-1, 3).copy()
    return p, rgb, kl.native.accum_guides().copy()


_FRAMES = {}


def _frames(kl, case, prev_spp=8, cur_spp=2):
    """The shared inputs of a case: the previous camera, its frame and guides at prev_spp, and the current frame and
    guides at cur_spp at the case's own camera (rendered once, never written)."""
    key = (case, prev_spp, cur_spp)
    if key not in _FRAMES:
        cam = np.asarray(_inputs(case)[1], F)
        pcam = _moved(cam)
        p, prgb, pg = _render(kl, case, pcam, prev_spp)
        p, crgb, cg = _render(kl, case, cam, cur_spp)
        p.close()
        for a in (pcam, prgb, pg, crgb, cg):
            a.setflags(write=False)
        _FRAMES[key] = (pcam, prgb, pg, crgb, cg)
    return _FRAMES[key]


def _reproject(ctx, prgb, pg, pcam, crgb, cg, npix, width, stream=0, **kw):
    """rt_reproject_device on host arrays, through device tensors: (out_rgb [npix, 3], out_guides [npix, 12])."""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, F).reshape(-1).copy()).cuda()   # noqa: E731
    d_prgb, d_pg, d_crgb, d_cg = up(prgb), up(pg), up(crgb), up(cg)
    d_rgb = torch.full((3 * npix,), -1.0, dtype=torch.float32, device="cuda")
    d_g = torch.full((12 * npix,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.reproject_device(d_prgb.data_ptr(), d_pg.data_ptr(), pcam, d_crgb.data_ptr(), d_cg.data_ptr(), npix, width,
                         d_rgb.data_ptr(), d_g.data_ptr(), _native.ReprojectParams(**kw) if kw else None, stream)
    torch.cuda.synchronize()
    return d_rgb.cpu().numpy().reshape(-1, 3), d_g.cpu().numpy().reshape(-1, 12)


def _f(g):
    return np.ascontiguousarray(g, F).reshape(-1, 12)[:, 7].copy().view(np.int32)


def _check(got, want, msg=""):
    _same(got[0], want[0], msg + " out_rgb")
    _same(got[1], want[1], msg + " out_guides")


# ---- 1. the kernel is its definition, bit for bit (and 4b: a pixel with f = 0 passes through) ----
@pytest.mark.parametrize("kw", [{}, OTHER], ids=["defaults", "other"])
@pytest.mark.parametrize("case", CASES)
def test_reprojection_equals_its_definition(pl, ref_kl, case, kw):
    npix, W = _inputs(case)[3], int(_inputs(case)[1][6])
    pcam, prgb, pg, crgb, cg = _frames(ref_kl, case)
    want = R.reproject(prgb, pg, _native.reproject_basis(pcam), crgb, cg, npix, W, **kw)
    got = _reproject(pl.native, prgb, pg, pcam, crgb, cg, npix, W, **kw)
    _check(got, want, case)
    off = _f(cg) <= 0
    np.testing.assert_array_equal(_bits(got[0])[off], _bits(crgb)[off])
    np.testing.assert_array_equal(_bits(got[1])[off], _bits(cg)[off])
    hist = _f(got[1]) > _f(cg)
    assert hist.any() and (_bits(got[0])[hist] != _bits(crgb)[hist]).any()
    keep = np.ones(12, bool)
    keep[7] = False
    np.testing.assert_array_equal(_bits(got[1])[:, keep], _bits(cg)[:, keep])
    if kw:
        assert (_bits(want[0]) != _bits(R.reproject(prgb, pg, _native.reproject_basis(pcam), crgb, cg, npix, W)[0])).any()
    print(case, "filterable %.3f, with history %.3f of them" % ((~off).mean(), hist.sum() / max((~off).sum(), 1)))


# ---- 2. a partial last row ----
def test_partial_last_row(pl):
    case, npix = "cornell_64_s4", 64 * 40 + 23
    cam = np.asarray(_inputs(case)[1], F)
    pcam = _moved(cam)
    p, prgb, pg = _render(pl, case, pcam, 8, npix)
    p, crgb, cg = _render(pl, case, cam, 2, npix)
    assert cg.shape == (npix, 12)
    want = R.reproject(prgb, pg, _native.reproject_basis(pcam), crgb, cg, npix, 64)
    assert (_f(want[1])[-23:] > 2).any()
    # the pixels past npix are never read: poison behind the frames changes nothing
    pad = lambda a: np.concatenate([a, np.full((41, a.shape[1]), np.nan, F)])   # noqa: E731
    _check(_reproject(pl.native, pad(prgb), pad(pg), pcam, pad(crgb), pad(cg), npix, 64), want)
    out, h2 = p.reprojected(_history(prgb, pg, pcam, npix), return_history=True)
    _check((out, h2.guides), want, "host form")


def _history(rgb, g, cam, npix):
    from ensem3a_openclraytracer_amd.KernelLauncher import History
    return History(np.ascontiguousarray(rgb, F).reshape(-1), np.ascontiguousarray(g, F), np.array(cam, F), npix)


# ---- 3. frames smaller than the footprint ----
def _wall(ctx, cam, npix, f, depth=2.0):
    """Synthetic guides of a wall facing the (unrotated) camera at `depth`, from rt_camera_rays, and a smooth frame."""
    rays = ctx.camera_rays(cam, npix)
    g = np.zeros((npix, 12), F)
    k = (F(depth) / rays[:, 1]).astype(F)
    g[:, 0:3] = (0, -1, 0)
    g[:, 3] = k
    g[:, 4:7] = rays[:, 3:6] + rays[:, 0:3] * k[:, None]
    g.view(np.int32)[:, 7] = f
    g[:, 8:11] = (0.8, 0.5, 0.2)
    g.view(np.int32)[:, 11] = 3
    rgb = (g[:, 8:11] * (F(0.3) + F(0.1) * g[:, 4:5] + F(0.05) * g[:, 6:7])).astype(F)
    return rgb, g


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 3), (5, 5)])
def test_frames_smaller_than_the_footprint(pl, w, h):
    cam = np.asarray([0.0, -3.5, 1.0, 0.0, 0.0, 0.0, w, h, 1, 0.6], F)
    pcam = _moved(cam, dx=0.03, rz=0.5)
    npix = w * h
    crgb, cg = _wall(pl.native, cam, npix, 2)
    prgb, pg = _wall(pl.native, pcam, npix, 9)
    prgb = (prgb * F(0.5)).astype(F)
    want = R.reproject(prgb, pg, _native.reproject_basis(pcam), crgb, cg, npix, w)
    assert (_f(want[1]) > 2).any()
    _check(_reproject(pl.native, prgb, pg, pcam, crgb, cg, npix, w), want)


# ---- 4. a previous camera that looks away: everything passes through ----
def test_a_previous_camera_looking_away_passes_everything_through(pl, ref_kl):
    case = "cornell_64_s4"
    npix, W = _inputs(case)[3], 64
    _, prgb, pg, crgb, cg = _frames(ref_kl, case)
    away = np.array(_inputs(case)[1], F)
    away[5] += F(180.0)
    got = _reproject(pl.native, prgb, pg, away, crgb, cg, npix, W)
    _check(got, (crgb, cg))


# ---- 5. a static camera: a pixel finds itself ----
def test_static_camera(pl, ref_kl):
    case = "cornell_64_s4"
    npix, W = _inputs(case)[3], 64
    cam = np.asarray(_inputs(case)[1], F)
    _, _, _, crgb, cg = _frames(ref_kl, case)
    fp = _f(cg)
    there = (fp > 0) & (np.arange(npix) >= W - 1)
    assert there.any()
    got = _reproject(pl.native, crgb, cg, cam, crgb, cg, npix, W)
    _check(got, R.reproject(crgb, cg, _native.reproject_basis(cam), crgb, cg, npix, W))
    assert (_f(got[1])[there] >= fp[there] + 1).all()
    flat = (F(0.5) * cg[:, 8:11]).astype(F)
    got = _reproject(pl.native, flat, cg, cam, flat, cg, npix, W)
    assert (_f(got[1])[there] >= fp[there] + 1).all()
    ulp = np.abs(_bits(got[0]).astype(np.int64) - _bits(flat).astype(np.int64))
    print("static camera, flat frame: worst distance %d ulp" % ulp[there].max())
    assert ulp[there].max() <= 2


# ---- 6. the outputs chain: into the filter, and into the next move ----
def test_outputs_chain_into_the_filter_and_the_next_move(pl, ref_kl):
    import torch
    case = "monkey_c3_64_s4"
    npix, W = _inputs(case)[3], 64
    cam = np.asarray(_inputs(case)[1], F)
    pcam, prgb, pg, crgb, cg = _frames(ref_kl, case)
    one = R.reproject(prgb, pg, _native.reproject_basis(pcam), crgb, cg, npix, W)
    ctx = pl.native
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, F).reshape(-1).copy()).cuda()   # noqa: E731
    d_prgb, d_pg, d_crgb, d_cg = up(prgb), up(pg), up(crgb), up(cg)
    d_rgb, d_g = torch.zeros(3 * npix, device="cuda"), torch.zeros(12 * npix, device="cuda")
    d_den = torch.zeros(3 * npix, device="cuda")
    torch.cuda.synchronize()
    ctx.reproject_device(d_prgb.data_ptr(), d_pg.data_ptr(), pcam, d_crgb.data_ptr(), d_cg.data_ptr(), npix, W,
                         d_rgb.data_ptr(), d_g.data_ptr())
    ctx.denoise_device(d_rgb.data_ptr(), d_g.data_ptr(), npix, W, d_den.data_ptr())
    torch.cuda.synchronize()
    _check((d_rgb.cpu().numpy(), d_g.cpu().numpy()), one)
    _same(d_den.cpu().numpy(), D.denoise(one[0], one[1], npix, W), "rt_denoise_device of the outputs")
    assert (_bits(D.denoise(one[0], one[1], npix, W)) != _bits(D.denoise(one[0], cg, npix, W))).any()
    # the second move: back to the first camera, whose 8 spp frame is now the current one
    d_rgb2, d_g2 = torch.zeros(3 * npix, device="cuda"), torch.zeros(12 * npix, device="cuda")
    torch.cuda.synchronize()
    ctx.reproject_device(d_rgb.data_ptr(), d_g.data_ptr(), cam, d_prgb.data_ptr(), d_pg.data_ptr(), npix, W,
                         d_rgb2.data_ptr(), d_g2.data_ptr())
    torch.cuda.synchronize()
    two = R.reproject(one[0], one[1], _native.reproject_basis(cam), prgb, pg, npix, W)
    _check((d_rgb2.cpu().numpy(), d_g2.cpu().numpy()), two, "the second move")
    assert _f(two[1]).max() > 8 + 2


# ---- 7. the host form ----
@pytest.mark.parametrize("lens", [None, (1.0, 0.05, 3.0)], ids=["plain", "lens"])
def test_host_form_equals_the_device_form(pl, ref_kl, lens):
    case = "serre_96x54_s4"
    npix, W = _inputs(case)[3], 96
    cam = np.asarray(_inputs(case)[1], F)
    pcam, prgb, pg, _, _ = _frames(ref_kl, case)
    p, crgb, cg = _render(pl, case, cam, 2, lens=lens)
    before = p.image().copy()
    _same(before, crgb)
    want = R.reproject(prgb, pg, _native.reproject_basis(pcam), crgb, cg, npix, W)
    _check(_reproject(pl.native, prgb, pg, pcam, crgb, cg, npix, W), want, "device form")
    h = _history(prgb, pg, pcam, npix)
    out, h2 = p.reprojected(h, return_history=True)
    _check((out, h2.guides), want, "host form")
    _same(h2.rgb, want[0])
    np.testing.assert_array_equal(h2.cam, cam)
    _same(p.reprojected(h, **OTHER), R.reproject(prgb, pg, _native.reproject_basis(pcam), crgb, cg, npix, W, **OTHER)[0])
    _same(p.reprojected(h, denoise=True), D.denoise(want[0], want[1], npix, W), "through the filter")
    _same(p.image(), before, "rt_accum_read after a reprojection")
    np.testing.assert_array_equal(p.sample_map(), 2)
    _same(pl.native.accum_guides(), cg)
    hh = p.history()
    _same(hh.rgb, crgb)
    _same(hh.guides, cg)
    np.testing.assert_array_equal(hh.cam, cam)


def test_three_slots_of_one_device_give_the_one_slot_bits(pl, ref_kl):
    case = "serre_96x54_s4"
    npix, W = _inputs(case)[3], 96
    cam = np.asarray(_inputs(case)[1], F)
    pcam, prgb, pg, crgb, cg = _frames(ref_kl, case)
    want = R.reproject(prgb, pg, _native.reproject_basis(pcam), crgb, cg, npix, W)
    ml = _launcher([0, 0, 0])
    try:
        q, rgb3, g3 = _render(ml, case, cam, 2)
        _same(rgb3, crgb)
        _same(g3, cg)
        out, h2 = q.reprojected(_history(prgb, pg, pcam, npix), return_history=True)
        _check((out, h2.guides), want)
        _same(q.image(), rgb3, "rt_accum_read after a reprojection")
        _same(q.reprojected(_history(prgb, pg, pcam, npix), denoise=True), D.denoise(want[0], want[1], npix, W))
    finally:
        ml.close()


def test_tile_forms_on_one_stream_without_a_host_wait(pl, ref_kl):
    import torch
    case = "monkey_c3_64_s4"
    sc, cam, env, npix, _, mb, ibl = _inputs(case)
    pcam, prgb, pg, crgb, cg = _frames(ref_kl, case)
    want = R.reproject(prgb, pg, _native.reproject_basis(pcam), crgb, cg, npix, 64)
    p, _, _ = _render(pl, case, cam, 2)     # (the scene's upload)
    ctx = pl.native
    d_prgb = torch.from_numpy(prgb.reshape(-1).copy()).cuda()
    d_pg = torch.from_numpy(pg.reshape(-1).copy()).cuda()
    d_rgb, d_g = torch.zeros(3 * npix, device="cuda"), torch.zeros(12 * npix, device="cuda")
    d_out, d_og = torch.zeros(3 * npix, device="cuda"), torch.zeros(12 * npix, device="cuda")
    d_den = torch.zeros(3 * npix, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream
    ctx.accum_begin_device(cam, env, npix, mb, 0, 1)
    ctx.accum_add_device(2, d_rgb.data_ptr(), s)
    ctx.accum_guides_device(d_g.data_ptr(), s)
    ctx.reproject_device(d_prgb.data_ptr(), d_pg.data_ptr(), pcam, d_rgb.data_ptr(), d_g.data_ptr(), npix, 64,
                         d_out.data_ptr(), d_og.data_ptr(), None, s)
    ctx.denoise_device(d_out.data_ptr(), d_og.data_ptr(), npix, 64, d_den.data_ptr(), None, s)
    stream.synchronize()
    _same(d_rgb.cpu().numpy(), crgb)
    _same(d_g.cpu().numpy(), cg)
    _check((d_out.cpu().numpy(), d_og.cpu().numpy()), want)
    _same(d_den.cpu().numpy(), D.denoise(want[0], want[1], npix, 64))
    ctx.accum_end()


# ---- 8. it helps ----
def _rmse(a, b):
    d = np.asarray(a, np.float64).reshape(-1) - np.asarray(b, np.float64).reshape(-1)
    return float(np.sqrt(np.mean(d * d)))


def test_reprojected_is_closer_to_the_converged_frame(pl, ref_kl):
    """Cornell 64 x 64: a history of 64 spp at the moved camera, a current frame of 2 spp, the converged frame 2048
    spp at the current camera.  Measured on the MI355X: 99.7 % of the filterable pixels receive history, and
    over them the RMSE falls from 0.1267 (the 2-spp frame) to 0.0286 reprojected."""
    case = "cornell_64_s4"
    npix, W = _inputs(case)[3], 64
    ref = np.asarray(_converged(ref_kl, case)).reshape(-1, 3)
    pcam, prgb, pg, crgb, cg = _frames(ref_kl, case, prev_spp=64)
    p, rgb2, g2 = _render(pl, case, np.asarray(_inputs(case)[1], F), 2)
    _same(rgb2, crgb)
    out, h2 = p.reprojected(_history(prgb, pg, pcam, npix), return_history=True)
    out = out.reshape(-1, 3)
    hist = _f(h2.guides) > _f(cg)
    share = hist.sum() / (_f(cg) > 0).sum()
    e0, e1 = _rmse(crgb[hist], ref[hist]), _rmse(out[hist], ref[hist])
    print("cornell 64x64: history on %.3f of the filterable pixels, rmse 2 spp %.4f -> reprojected %.4f" % (share, e0, e1))
    assert share > 0.5, share
    assert e1 < e0, (e0, e1)


# ---- 9. errors ----
def _status(fn, *a, **kw):
    with pytest.raises(_native.NativeError) as ei:
        fn(*a, **kw)
    return ei.value.status


def test_errors_leave_the_accumulation_and_the_outputs_unchanged(pl, ref_kl):
    import torch
    case = "cornell_64_s4"
    npix, W = _inputs(case)[3], 64
    cam = np.asarray(_inputs(case)[1], F)
    pcam, prgb, pg, _, _ = _frames(ref_kl, case)
    ctx = pl.native
    P = _native.ReprojectParams
    hrgb, hg = prgb.reshape(-1), pg.reshape(-1)
    assert _status(ctx.accum_reproject, hrgb, hg, pcam) == STATE          # nothing open
    sc, _, env, _, _, mb, ibl = _inputs(case)
    p = pl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.BVH.exportArray,
                             cam, env, npix, mb, ibl)
    assert _status(ctx.accum_reproject, hrgb, hg, pcam) == STATE          # before the first add
    frame = p.add(2).copy()

    def unchanged():
        np.testing.assert_array_equal(p.sample_map(), 2)
        _same(p.image(), frame)

    buf = torch.zeros(12 * npix + 4, dtype=torch.float32, device="cuda")
    outs = torch.zeros(15 * npix, dtype=torch.float32, device="cuda")
    a, o_rgb, o_g = buf.data_ptr(), outs.data_ptr(), outs.data_ptr() + 12 * npix
    assert o_g % 16 == 0

    def dev(prev_rgb=a, prev_g=a, pc=pcam, cur_rgb=a, cur_g=a, n=npix, w=W, out_rgb=o_rgb, out_g=o_g, params=None, di=0):
        return _status(ctx.reproject_device, prev_rgb, prev_g, pc, cur_rgb, cur_g, n, w, out_rgb, out_g, params, 0, di)

    bad_params = (P(sigma_p=0.0), P(sigma_p=-1.0), P(sigma_p=float("nan")), P(sigma_p=float("inf")), P(max_history=0.0),
                  P(max_history=float("inf")), P(max_history=float("nan")), P(normal_min=float("nan")),
                  P(normal_min=float("inf")), P(min_weight=float("nan")), P(min_weight=-float("inf")))
    for bad in bad_params:
        assert dev(params=bad) == ARG
        assert _status(ctx.accum_reproject, hrgb, hg, pcam, bad) == ARG
    for k in ("prev_rgb", "prev_g", "cur_rgb", "cur_g", "out_rgb", "out_g"):
        assert dev(**{k: 0}) == ARG, k
    assert dev(n=0) == ARG and dev(w=0) == ARG and dev(n=-5) == ARG and dev(di=7) == ARG
    assert dev(w=32) == ARG                                              # not prev_cam's width
    for k, v in ((0, np.nan), (5, np.inf), (9, -np.inf)):
        c = pcam.copy()
        c[k] = v
        assert dev(pc=c) == ARG
        assert _status(ctx.accum_reproject, hrgb, hg, c) == ARG
    narrow = pcam.copy()
    narrow[6] = 32
    assert _status(ctx.accum_reproject, hrgb, hg, narrow) == ARG
    for k in ("prev_g", "cur_g", "out_g"):                                # misaligned guides
        assert dev(**{k: (o_g if k == "out_g" else a) + 4}) == ARG, k
    # outputs that overlap an input or each other
    assert dev(out_rgb=a) == ARG and dev(out_g=a) == ARG and dev(prev_rgb=o_rgb) == ARG and dev(cur_g=o_g) == ARG
    assert dev(out_rgb=o_g + 16) == ARG and dev(out_g=o_rgb + 16) == ARG
    lib = _native.lib()
    out = np.zeros(3 * npix, F)
    og = np.zeros(12 * npix, F)
    cp = pcam.ctypes.data
    for args in ((None, hg.ctypes.data, cp, None, out.ctypes.data, og.ctypes.data),
                 (hrgb.ctypes.data, None, cp, None, out.ctypes.data, og.ctypes.data),
                 (hrgb.ctypes.data, hg.ctypes.data, None, None, out.ctypes.data, og.ctypes.data),
                 (hrgb.ctypes.data, hg.ctypes.data, cp, None, None, og.ctypes.data),
                 (hrgb.ctypes.data, hg.ctypes.data, cp, None, out.ctypes.data, None)):
        assert lib.rt_accum_reproject(ctx.handle, *args) == ARG
    with pytest.raises(ValueError):
        ctx.accum_reproject(hrgb[:-3], hg, pcam)
    unchanged()
    torch.cuda.synchronize()
    assert not outs.any() and not buf.any() and not out.any() and not og.any()
    # an invalidation
    ctx.set_env(ibl)
    assert _status(ctx.accum_reproject, hrgb, hg, pcam) == STATE
    p.close()
    with pytest.raises(RuntimeError):
        p.reprojected(_history(prgb, pg, pcam, npix))
    assert _status(ctx.accum_reproject, hrgb, hg, pcam) == STATE

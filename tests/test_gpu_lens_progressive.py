"""Progressive lens frames on the GPU (rt_accum_begin_lens*, KernelLauncher.begin_progressive_lens): a camera ray per
sample inside rt_accum_*.  Under test, DESIGN.md 2.5's contracts, each bit for bit:

  E1  a pixel that has received n samples -- by any sequence of full and selected adds, on any engine, block, grid, tile
      or split over slots -- holds the record rt_lens_radiance returns for it at spp = n, in all 32 bytes, and the frame
      is the clamped mean of those records;
  E2  the degenerate lens (jitter 0, aperture 0) gives the plain accumulation's frames, sample map, selection and
      guides, and so rt_render's frame;
  E3  the guides are those of a plain accumulation whose pixels hold the same counts, whatever the lens: the first hit
      is the pixel-centre pinhole ray's; rt_accum_read gives the same bits before and after.

Scenes, cameras and helpers: tests/radiance_scenes.py (cornell and soup7: brute force; soup150: the BVH2 walk).  Frames
are 25 x 23 pixels (575: a partial last wave, a partial block at every block size), max_bounce 4, at most 8 samples per
pixel.  Records are read through rt_debug_accum_state and compared word for word: equal bits, or NaN on both sides.
"""
import functools

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests import denoise_ref as DR
from tests import radiance_scenes as RS
from tests.radiance_scenes import NPIX, WIDTH
from tests.test_gpu_lens import DEGENERATE, LENS, PINHOLE, SEED, differing_records
from tests.test_gpu_radiance import FAST, REF, render, using

pytestmark = pytest.mark.gpu

MB = 4
SCENES = ("cornell", "soup7", "soup150")
STATE, ARG = _native.RT_ERR_STATE, _native.RT_ERR_ARG
NPIX_PARTIAL = 568   # 22 rows of 25 and one of 18


def _launcher(device=0):
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    k = KernelLauncher(None, None, device, None)
    k.upload_env(W.ibl_preview())
    return k


@pytest.fixture(scope="module")
def kl():
    k = _launcher()
    yield k
    k.close()


def begin_lens(kl, sc, lens, npix=NPIX):
    return kl.begin_progressive_lens(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.bvh, sc.cam,
                                     sc.env, npix, MB, W.ibl_preview(), jitter=lens[0], aperture=lens[1],
                                     focus=lens[2], seed=SEED)


def begin_plain(kl, sc, npix=NPIX):
    return kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.bvh, sc.cam,
                                sc.env, npix, MB, W.ibl_preview())


def lens_frame(kl, sc, spp, lens, npix=NPIX):
    """The definition of E1: rt_lens_radiance's records and frame of the whole frame at spp."""
    return kl.lens_frame(sc.cam, sc.env, npix, spp, MB, jitter=lens[0], aperture=lens[1], focus=lens[2], seed=SEED)


def records(kl):
    return kl.native.debug_accum_state()


def same(got, want, msg=""):
    np.testing.assert_array_equal(RS.bits(got).reshape(-1), RS.bits(want).reshape(-1), err_msg=str(msg))


def assert_records(kl, want_state, msg=""):
    bad = differing_records(records(kl), want_state)
    assert not len(bad), (msg, bad[:8])


def the_mask(npix=NPIX):
    """Pixel 0, pixels 60-70 (across a wave boundary) and the last real pixel."""
    m = np.zeros(npix, np.uint8)
    m[0] = m[npix - 1] = 1
    m[60:71] = 1
    return m


# ---- 1. E1: full adds ----

@pytest.mark.parametrize("traversal", [FAST, REF])
@pytest.mark.parametrize("lens", [PINHOLE, LENS])
@pytest.mark.parametrize("name", SCENES)
def test_adds_leave_the_lens_frames_records(kl, name, lens, traversal):
    sc = RS.scene(name)
    with using(kl, name, traversal):
        want = {n: lens_frame(kl, sc, n, lens) for n in (1, 3, 6)}
        p = begin_lens(kl, sc, lens)
        total = 0
        for a in (1, 2, 3):
            frame = p.add(a).copy()
            total += a
            assert p.samples == total
            assert_records(kl, want[total]["state"], (name, lens, traversal, total))
            same(frame, want[total]["rgb"], (name, total))
            same(p.image(), frame)
            np.testing.assert_array_equal(p.sample_map(), total)
        p.close()


# ---- 2. E2: the degenerate lens is the plain accumulation ----

def _plain_sequence(p, threshold):
    out = {}
    out[1] = p.add(1).copy()
    p.mark()
    out[3] = p.add(2).copy()
    out["n"] = p.select(threshold)
    out["selection"] = p.selection().copy()
    out["map"] = p.sample_map().copy()
    out["guides"] = p._ctx.accum_guides().copy()
    out[5] = p.add_selected(2).copy()
    out["map5"] = p.sample_map().copy()
    out["guides5"] = p._ctx.accum_guides().copy()
    return out


@pytest.mark.parametrize("traversal", [FAST, REF])
@pytest.mark.parametrize("name", SCENES)
def test_degenerate_lens_is_the_plain_accumulation(kl, name, traversal):
    sc = RS.scene(name)
    threshold = 0.02
    with using(kl, name, traversal):
        plain = _plain_sequence(begin_plain(kl, sc), threshold)
        lens = _plain_sequence(begin_lens(kl, sc, DEGENERATE), threshold)
        one_shot = {n: render(kl, sc, sc.cam, sc.env, NPIX, n, MB) for n in (1, 3)}
        for n in (1, 3):
            same(lens[n], plain[n], (name, n))
            same(lens[n], one_shot[n], (name, n, "launch_Raytracing"))
        assert lens["n"] == plain["n"]
        np.testing.assert_array_equal(lens["selection"], plain["selection"])
        np.testing.assert_array_equal(lens["map"], plain["map"])
        np.testing.assert_array_equal(lens["map5"], plain["map5"])
        same(lens["guides"], plain["guides"], name)
        same(lens["guides5"], plain["guides5"], name)
        same(lens[5], plain[5], name)
        kl.native.accum_end()


# ---- 3. E1: selected adds ----

@pytest.mark.parametrize("traversal", [FAST, REF])
@pytest.mark.parametrize("lens", [PINHOLE, LENS])
@pytest.mark.parametrize("name", SCENES)
def test_selected_adds_leave_each_pixel_its_own_counts_record(kl, name, lens, traversal):
    sc = RS.scene(name)
    mask = the_mask()
    on = mask != 0

    def expect(p, lo, hi, want, msg):
        """counts hi on the mask and lo elsewhere; every pixel's record and colour are lens_frame's at its count"""
        np.testing.assert_array_equal(p.sample_map(), np.where(on, hi, lo), err_msg=str(msg))
        state = np.where(on, want[hi]["state"], want[lo]["state"])
        assert_records(kl, state, msg)
        same(p.image().reshape(-1, 3), np.where(on[:, None], want[hi]["rgb"], want[lo]["rgb"]), msg)

    with using(kl, name, traversal):
        want = {n: lens_frame(kl, sc, n, lens) for n in (2, 3, 5, 6, 8)}
        p = begin_lens(kl, sc, lens)
        p.add(2)
        p.select_mask(mask)
        np.testing.assert_array_equal(p.selection(), mask)
        p.add_selected(3)
        expect(p, 2, 5, want, (name, "add_selected(3)"))
        frame = p.add(1).copy()                      # a full add once the counts differ
        expect(p, 3, 6, want, (name, "add(1)"))
        same(frame, p.image())
        # an empty selection adds nothing
        p.select_mask(np.zeros(NPIX, np.uint8))
        same(p.add_selected(1), frame)
        expect(p, 3, 6, want, (name, "empty selection"))
        # select_all + add_selected is a full add
        p.select_all()
        p.add_selected(2)
        expect(p, 5, 8, want, (name, "select_all"))
        p.close()


# ---- 4. a partial last row; tiles; several slots ----

def _partial_sequence(p, threshold):
    """begin .. guides of the tile test, through the host forms: what every tile must reproduce in its rows."""
    p.add(2)
    p.mark()
    p.add(1)
    n = p.select(threshold)
    frame = p.add_selected(2).copy()
    return dict(n=n, frame=frame.reshape(-1, 3), map=p.sample_map().copy(), selection=p.selection().copy(),
                guides=p._ctx.accum_guides().copy())


@functools.lru_cache(maxsize=None)
def _partial_whole(lens):
    """The one-slot whole-frame answer of the partial-row tests (cornell, FAST); computed once, never written."""
    k = _launcher()
    try:
        sc = RS.scene("cornell")
        with using(k, "cornell", FAST):
            p = begin_lens(k, sc, lens, NPIX_PARTIAL)
            out = _partial_sequence(p, 0.05)
            out["state"] = records(k).copy()
            out["want"] = {n: lens_frame(k, sc, n, lens, NPIX_PARTIAL) for n in (3, 5)}
            p.close()
    finally:
        k.close()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_partial_last_row_is_the_lens_frames(kl):
    whole = _partial_whole(LENS)
    assert 0 < whole["n"] < NPIX_PARTIAL, whole["n"]      # the threshold splits the frame
    assert whole["n"] == int(whole["selection"].sum())
    five = whole["selection"] != 0
    np.testing.assert_array_equal(whole["map"], np.where(five, 5, 3))
    want = whole["want"]
    bad = differing_records(whole["state"], np.where(five, want[5]["state"], want[3]["state"]))
    assert not len(bad), bad[:8]
    same(whole["frame"], np.where(five[:, None], want[5]["rgb"], want[3]["rgb"]))


@pytest.mark.parametrize("row0,row_step", [(0, 1), (1, 2), (2, 3)])
def test_device_tile_forms_on_one_stream_without_a_host_wait(kl, row0, row_step):
    import torch
    whole = _partial_whole(LENS)
    sc = RS.scene("cornell")
    npix = NPIX_PARTIAL
    rows = np.arange(row0, -(-npix // WIDTH), row_step)
    nloc = len(rows) * WIDTH
    assert nloc == _native.tile_rows(npix, WIDTH, row0, row_step) * WIDTH
    pix = (rows[:, None] * WIDTH + np.arange(WIDTH)[None, :]).reshape(-1)   # the tile's pixels, padding included
    real = pix < npix
    with using(kl, "cornell", FAST):
        ctx = kl.native
        d_rgb = torch.full((3 * nloc,), -1.0, dtype=torch.float32, device="cuda")
        d_g = torch.full((12 * nloc,), -1.0, dtype=torch.float32, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        s = stream.cuda_stream
        ctx.accum_begin_lens_device(sc.cam, sc.env, _native.Lens(LENS[0], LENS[1], LENS[2], SEED), npix, MB, row0,
                                    row_step)
        ctx.accum_add_device(2, d_rgb.data_ptr(), s)
        ctx.accum_mark_device(s)
        ctx.accum_add_device(1, d_rgb.data_ptr(), s)
        ctx.accum_select_device(0.05, s)
        ctx.accum_add_selected_device(2, d_rgb.data_ptr(), s)
        ctx.accum_guides_device(d_g.data_ptr(), s)
        stream.synchronize()
        rgb = d_rgb.cpu().numpy().reshape(-1, 3)
        g = d_g.cpu().numpy().reshape(-1, 12)
        same(rgb[real], whole["frame"][pix[real]], (row0, row_step))
        same(g[real], whole["guides"][pix[real]], (row0, row_step))
        # padding pixels of the partial last row: the miss pattern, no sample
        miss = np.array([0, 0, 0, -1, 0, 0, 0, 0, 1, 1, 1, 0], np.float32)
        miss.view(np.int32)[11] = -1
        for row in g[~real]:
            same(row, miss)
        # a second guides call traces nothing and gives the same bits
        d_g.fill_(-1.0)
        torch.cuda.synchronize()
        ctx.accum_guides_device(d_g.data_ptr(), s)
        stream.synchronize()
        same(d_g.cpu().numpy().reshape(-1, 12), g)
        ctx.accum_end()


def test_host_form_over_three_slots_of_one_device():
    whole = _partial_whole(LENS)
    sc = RS.scene("cornell")
    ml = _launcher([0, 0, 0])
    try:
        with using(ml, "cornell", FAST):
            p = begin_lens(ml, sc, LENS, NPIX_PARTIAL)
            got = _partial_sequence(p, 0.05)
            assert got["n"] == whole["n"]
            same(got["frame"], whole["frame"])
            np.testing.assert_array_equal(got["map"], whole["map"])
            np.testing.assert_array_equal(got["selection"], whole["selection"])
            same(got["guides"], whole["guides"])
            bad = differing_records(records(ml), whole["state"])
            assert not len(bad), bad[:8]
            p.close()
    finally:
        ml.close()


# ---- 5. E3: the guides are the plain accumulation's at the same counts ----

@pytest.mark.parametrize("traversal", [FAST, REF])
@pytest.mark.parametrize("name", SCENES)
def test_guides_are_the_plain_accumulations_whatever_the_lens(kl, name, traversal):
    sc = RS.scene(name)
    mask = the_mask()
    with using(kl, name, traversal):
        q = begin_plain(kl, sc)
        q.add(2)
        plain2 = q._ctx.accum_guides().copy()
        q.select_mask(mask)
        q.add_selected(3)
        plain5 = q._ctx.accum_guides().copy()
        assert (plain2 != plain5).any()                  # f follows the counts
        for lens in (LENS, PINHOLE):
            p = begin_lens(kl, sc, lens)
            frame = p.add(2).copy()
            same(p._ctx.accum_guides(), plain2, (name, lens, "after add(2)"))      # the call that traces
            same(p.image(), frame, "rt_accum_read after the first guides call")
            same(p._ctx.accum_guides(), plain2, (name, lens, "a later call"))
            p.select_mask(mask)
            frame = p.add_selected(3).copy()
            g = p._ctx.accum_guides().copy()
            same(g, plain5, (name, lens, "after the selected add"))
            same(p.image(), frame)
            same(p.denoised().reshape(-1, 3), DR.denoise(frame, g, NPIX, WIDTH), (name, lens, "denoised"))
            same(p.image(), frame, "rt_accum_read after a denoise")
            p.close()


# ---- 6. neutrality ----

def test_block_grid_and_engine_may_change_between_adds(kl):
    sc = RS.scene("soup7")
    with using(kl, "soup7", FAST):
        want = {n: lens_frame(kl, sc, n, LENS) for n in (2, 5, 6, 7, 8)}
        ctx = kl.native
        try:
            p = begin_lens(kl, sc, LENS)
            ctx.set_option("block", 64)
            p.add(2)
            assert_records(kl, want[2]["state"], "block 64")
            ctx.set_option("block", 256)
            p.add(3)
            assert_records(kl, want[5]["state"], "block 256")
            ctx.set_option("radiance_grid", 1)
            p.add(1)
            assert_records(kl, want[6]["state"], "one block")
            ctx.set_option("radiance_grid", 0)
            ctx.set_option("brute_max", 0)               # the BVH2 walk in place of the brute force
            p.add(1)
            assert_records(kl, want[7]["state"], "the tree walk")
            g_walk = p._ctx.accum_guides().copy()
            ctx.set_option("brute_max", 64)
            p.select_all()
            same(p.add_selected(1), want[8]["rgb"])
            assert_records(kl, want[8]["state"], "brute force again, a listed add")
            g = p._ctx.accum_guides().copy()
            g_walk[:, 7].view(np.int32)[g_walk[:, 7].view(np.int32) > 0] = 8
            same(g, g_walk)
            p.close()
        finally:
            for k, v in (("block", 128), ("radiance_grid", 0), ("brute_max", 64)):
                ctx.set_option(k, v)


def test_other_calls_between_select_and_add_selected_leave_the_accumulation_alone(kl):
    name = "soup150"
    sc = RS.scene(name)
    with using(kl, name, FAST):
        want = {n: lens_frame(kl, sc, n, LENS) for n in (3, 5)}
        p = begin_lens(kl, sc, LENS)
        p.add(1)
        p.mark()
        p.add(2)
        n = p.select(0.0)
        sel = p.selection().copy()
        assert 0 < n == int(sel.sum())
        # an rt_render, an rt_trace, a lens frame and an rt_radiance in between
        assert render(kl, sc, sc.cam, sc.env, NPIX, 2, MB).mean() > 0.0
        o, d, seeds = kl.camera_rays(sc.cam, NPIX)
        assert len(kl.trace_rays(o, d)["k"]) == NPIX
        lens_frame(kl, sc, 2, PINHOLE)
        kl.radiance(o, d, 2, MB, sc.env, seeds=seeds)
        np.testing.assert_array_equal(p.selection(), sel)
        np.testing.assert_array_equal(p.sample_map(), 3)
        assert_records(kl, want[3]["state"], "after the other calls")
        assert p.select(0.0) == n                        # the mark is still the one taken after the first add
        np.testing.assert_array_equal(p.selection(), sel)
        p.add_selected(2)
        on = sel != 0
        np.testing.assert_array_equal(p.sample_map(), np.where(on, 5, 3))
        assert_records(kl, np.where(on, want[5]["state"], want[3]["state"]), "the selected add")
        p.close()


# ---- 7. errors ----

def _error(fn, *a, **kw):
    with pytest.raises(_native.NativeError) as ei:
        fn(*a, **kw)
    return ei.value.status, str(ei.value)


def test_errors_leave_the_accumulation_unchanged(kl):
    sc = RS.scene("cornell")
    nan = float("nan")
    with using(kl, "cornell", FAST):
        ctx = kl.native
        p = begin_lens(kl, sc, LENS)
        # a selected add needs a selection, and a full add first
        assert _error(p.add_selected, 1)[0] == STATE
        frame = p.add(2).copy()

        def unchanged():
            np.testing.assert_array_equal(p.sample_map(), 2)
            same(p.image(), frame)
            assert p.samples == 2

        # a failing begin leaves the open accumulation as it was
        L = _native.Lens
        for lens, text in ((None, "lens must not be NULL"),
                           (L(-0.5, 0.0, 1.0, 0), "lens jitter must be finite and >= 0"),
                           (L(nan, 0.0, 1.0, 0), "lens jitter must be finite and >= 0"),
                           (L(1.0, -1e-3, 1.0, 0), "lens aperture must be finite and >= 0"),
                           (L(1.0, nan, 1.0, 0), "lens aperture must be finite and >= 0"),
                           (L(1.0, 0.0, 0.0, 0), "lens focus must be finite and > 0")):
            status, msg = _error(ctx.accum_begin_lens, sc.cam, sc.env, lens, NPIX, MB)
            assert status == ARG and text in msg, (status, msg)
            status, msg = _error(ctx.accum_begin_lens_device, sc.cam, sc.env, lens, NPIX, MB, 0, 1)
            assert status == ARG and text in msg, (status, msg)
        unchanged()
        assert _error(p.add, 0)[0] == ARG
        assert _error(p.add_selected, 1)[0] == STATE           # still no selection
        p.select_all()
        assert _error(p.add_selected, 0)[0] == ARG
        assert _error(p.add, _native.RT_ACCUM_MAX_SAMPLES)[0] == ARG
        unchanged()
        # a fresh accumulation: a selection needs samples, a selected add a full add
        p = begin_lens(kl, sc, LENS)
        assert _error(p.select_all)[0] == STATE
        assert _error(p.add_selected, 1)[0] == STATE
        assert _error(p.guides)[0] == STATE
        frame = p.add(2).copy()
        unchanged()
        # rt_set_scene invalidates: add and guides refuse, the count stays readable
        ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.bvh)
        assert _error(p.add, 1)[0] == STATE
        assert _error(p.guides)[0] == STATE
        assert _error(p.add_selected, 1)[0] == STATE
        assert p.samples == 2
        # ... and a new begin starts over
        p = begin_lens(kl, sc, LENS)
        same(p.add(2), frame)
        p.guides()
        p.close()
        with pytest.raises(RuntimeError):
            p.add(1)

"""Option "brute_refill" (FrameParams::refill): a wave of the one-lane brute-force kernels hands out jobs only once
R of its lanes are free -- or none of its lanes traces, or its hand-out is near its end.  Which lane renders a
pixel never affects the pixel (its seeds come from its index), so every frame is the frame of R = 1, bit for bit.

R = 64 on a launch of fewer than 64 pixels is a threshold no wave can meet: those launches end through the rule
"no lane of the wave traces".  Every GPU step runs under a time limit of its own (_limit): a launch that waits for
a threshold it cannot meet ends the test process instead of hanging it."""
import contextlib
import faulthandler
import functools

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W

pytestmark = pytest.mark.gpu

RS = (2, 4, 64)
DEFAULTS = {"brute_refill": -1, "slices": -1, "brute_cluster": -1, "team": 0}
STEP_SECONDS = 60


@contextlib.contextmanager
def _limit(seconds=STEP_SECONDS):
    """One GPU step: past the limit the process prints its stacks and exits (a blocked HIP call takes no signal)."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def kl():
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    k = KernelLauncher(None, None, 0, None)
    yield k
    for key, v in DEFAULTS.items():
        k.native.set_option(key, v)
    k.close()


@pytest.fixture(autouse=True)
def _defaults(kl):
    yield
    for key, v in DEFAULTS.items():
        kl.native.set_option(key, v)


@functools.lru_cache(maxsize=None)
def _soup():
    from tests.test_brute_clusters import GPU_SOUPS
    from tests.test_gpu_parity import _random_scene
    return _random_scene(*GPU_SOUPS[0])


def _inputs(scene, w, h, spp):
    """(scene, cam, env, npix, spp, max_bounce, ibl) of Cornell or of a random triangle soup under a lit sun."""
    if scene == "cornell":
        return W.PARITY_CASES["cornell_64_s4"].with_size(w, h, spp).inputs()
    from tests.test_gpu_nonfinite import SOUP_CAM, SOUP_ENV
    cam = SOUP_CAM.copy()
    cam[6], cam[7] = w, h
    return _soup(), cam, SOUP_ENV, w * h, spp, 4, W.ibl_preview()


def _set(kl, opts):
    for key, v in dict(DEFAULTS, **opts).items():
        kl.native.set_option(key, v)


def _frame(kl, inp, **opts):
    sc, cam, env, n, s, m, ibl = inp
    _set(kl, opts)
    out = np.zeros(3 * n, np.float32)
    with _limit():
        kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                             sc.BVH.exportArray, cam, env, n, s, m, ibl)
    assert kl.native.scene_info()["brute_records"] > 0
    return out


def _all_rs(kl, inp, want_r=True, **opts):
    """The launch with every lane refilled at once, then with each R: the same frame."""
    base = _frame(kl, inp, brute_refill=1, **opts)
    assert _native.last_refill()[0] == 0
    for r in RS:
        got = _frame(kl, inp, brute_refill=r, **opts)
        if want_r:
            assert _native.last_refill()[0] == r, (r, opts)
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (r, opts)
    return base


SCENES = ("cornell", "soup")


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("size", ((1, 1, 3), (63, 1, 5), (65, 1, 5), (130, 3, 5)), ids=str)
def test_partial_waves(kl, scene, size):
    """A single pixel, a wave short of one lane, a wave and one lane, and three rows that end in a partial wave:
    with R = 64 the first two can never have 64 lanes free."""
    base = _all_rs(kl, _inputs(scene, *size), team=1)
    assert np.isfinite(base).all()


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("cluster", (0, 1))
@pytest.mark.parametrize("slices", (0, 4))
def test_sliced_and_clustered(kl, scene, cluster, slices):
    """96 x 96 at 8 spp: slices forced (K = 4, every pixel) and off, clusters forced and off."""
    inp = _inputs(scene, 96, 96, 8)
    _all_rs(kl, inp, team=1, slices=slices, brute_cluster=cluster)
    assert _native.last_slices() == ((4 | 256 << 8) if slices else 0)


@pytest.mark.parametrize("scene", SCENES)
def test_row_tile(kl, scene):
    """Rows 1::3 of 96 x 96."""
    import torch
    inp = _inputs(scene, 96, 96, 8)
    sc, cam, env, npix, spp, mb, ibl = inp
    whole = _frame(kl, inp, brute_refill=1, team=1)
    tile = whole.reshape(-1, 3 * 96)[1::3].ravel()
    n = 3 * 96 * _native.tile_rows(npix, 96, 1, 3)
    assert n == tile.size
    for r in (1,) + RS:
        _set(kl, dict(brute_refill=r, team=1))
        t = torch.zeros(n, dtype=torch.float32, device="cuda")
        with _limit():
            kl.native.render_device(cam, env, npix, spp, mb, 1, 3, t.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        assert _native.last_refill()[0] == (r if r > 1 else 0)
        assert np.array_equal(t.cpu().numpy().view(np.uint32), tile.view(np.uint32)), r


@pytest.mark.parametrize("scene", SCENES)
def test_progressive_and_listed_adds(kl, scene):
    """rt_accum_*: an add of 4 + 4 samples, then a listed add of 4 on a mask that covers every column."""
    inp = _inputs(scene, 96, 96, 8)
    sc, cam, env, npix, spp, mb, ibl = inp
    mask = ((np.arange(npix) // 96 + np.arange(npix) % 96) % 3 == 0).astype(np.uint8)
    assert mask.reshape(96, 96).any(axis=0).all()
    frames = {}
    for r in (1,) + RS:
        _set(kl, dict(brute_refill=r, team=1))
        with _limit():
            p = kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                     sc.BVH.exportArray, cam, env, npix, mb, ibl)
            a = p.add(4).copy()
            b = p.add(4).copy()
            p.select_mask(mask)
            c = p.add_selected(4).copy()
            p.close()
        assert _native.last_refill()[0] == (r if r > 1 else 0)
        frames[r] = (a, b, c)
    one_shot = _frame(kl, inp, brute_refill=1, team=1)
    assert np.array_equal(frames[1][1].view(np.uint32), one_shot.view(np.uint32))
    for r in RS:
        for got, want in zip(frames[r], frames[1]):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), r


@pytest.mark.parametrize("scene", SCENES)
def test_more_pixels_than_resident_lanes(kl, scene):
    """1024 x 512 at 1 spp: more pixels than the device keeps lanes, so the hand-out turns over and the launch ends
    through "the group is near its end".  Auto takes the threshold on a tile this large."""
    inp = _inputs(scene, 1024, 512, 1)
    base = _all_rs(kl, inp)
    auto = _frame(kl, inp)
    assert _native.last_refill()[0] == _native.brute_refill(1024 * 512, 5 * 4 * 256 * 64) > 0
    assert np.array_equal(auto.view(np.uint32), base.view(np.uint32))


def test_auto_rule_of_the_launches(kl):
    """Auto: off on 96 x 96 (as launched), on for the 1024 x 1024 headline frame (the rule alone: nothing rendered)."""
    _frame(kl, _inputs("cornell", 96, 96, 8))
    assert _native.last_refill()[0] == 0
    _frame(kl, _inputs("cornell", 96, 96, 8), team=1)
    assert _native.last_refill()[0] == 0
    assert _native.brute_refill(1024 * 1024, 5 * 4 * 256 * 64) == 4
    assert _native.brute_refill(96 * 96, 5 * 4 * 256 * 64) == 0


def test_counters(kl):
    """The instrumented launch takes the threshold too: the same rays and samples, fewer refill events."""
    inp = _inputs("cornell", 96, 96, 8)
    sc, cam, env, npix, spp, mb, ibl = inp
    _frame(kl, inp, brute_refill=1, team=1)
    got = {}
    for r in (1, 4):
        _set(kl, dict(brute_refill=r, team=1))
        with _limit():
            c = kl.native.count_work_detail(cam, env, npix, spp, mb)
        rr, ev, lanes = _native.last_refill()
        assert rr == (r if r > 1 else 0) and ev == c["refill_events"] > 0 and lanes >= npix
        got[r] = c
    for key in ("rays", "samples", "ev_diffuse", "sun_terms"):
        assert got[4][key] == got[1][key], key
    assert got[4]["refill_events"] < got[1]["refill_events"]


def test_option_range(kl):
    for bad in (-2, 65):
        with pytest.raises(_native.NativeError, match="brute_refill"):
            kl.native.set_option("brute_refill", bad)
    kl.native.set_option("brute_refill", 64)

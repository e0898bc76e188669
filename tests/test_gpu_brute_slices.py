"""Option "slices" on brute-force scenes: the one-lane brute-force kernels (rt_kernels.hip render_kernel, the
lock-step and the clustered loop) hand out each pixel's samples as K jobs, slice-major, and pass the pixel's
state -- with the cached first-bounce shadow ray -- from job to job.  Every pixel's samples still run in order,
so the frame is the unsliced frame, bit for bit.

The frames here are small on purpose: with fewer jobs than resident lanes, slice k + 1 of a pixel is taken while
its slice k runs, so nearly every job goes through the wait for its predecessor.  A set slice count keeps such a
tile on single lanes (auto would take teams of 4, and auto slices stay off below 1.5 pixels per resident lane)
and slices every pixel; auto slices only the tile's last pixels (test_auto_on_a_large_tile)."""
import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W

pytestmark = pytest.mark.gpu

KS = (2, 3, 5, 8, 16)
DEFAULTS = {"slices": -1, "brute_cluster": -1, "handout": -1, "team": 0}


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


def _cornell(w, h, spp, **params):
    wl = W.PARITY_CASES["cornell_64_s4"].with_size(w, h, spp)
    wl.params.update({k: str(v) for k, v in params.items()})
    return wl.inputs()


def _frame(kl, inp, spp=None, mb=None, npix=None, **opts):
    sc, cam, env, n, s, m, ibl = inp
    n = n if npix is None else npix
    for key, v in dict(DEFAULTS, **opts).items():
        kl.native.set_option(key, v)
    out = np.zeros(3 * n, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                         sc.BVH.exportArray, cam, env, n, s if spp is None else spp, m if mb is None else mb, ibl)
    assert kl.native.scene_info()["brute_records"] > 0
    return out


def _same(a, b, msg):
    assert a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes(), msg


@pytest.fixture(scope="module")
def cornell32():
    """Cornell 32x32, 16 spp, maxBounce 4 (its own sun is lit: sun_Power 0.5) and the oracle's frame."""
    inp = _cornell(32, 32, 16)
    sc, cam, env, npix, spp, mb, ibl = inp
    assert env[3] > 0
    return inp, O.render(O.OracleScene.from_scene(sc, ibl), cam, env, npix, spp, mb, nthreads=16)


@pytest.mark.parametrize("cluster", (0, 1))
@pytest.mark.parametrize("size", ((32, 32), (48, 20)), ids=str)
def test_frames_equal_unsliced_and_the_oracle(kl, cornell32, size, cluster):
    if size == (32, 32):
        inp, want = cornell32
    else:
        inp = _cornell(*size, 16)
        sc, cam, env, npix, spp, mb, ibl = inp
        want = O.render(O.OracleScene.from_scene(sc, ibl), cam, env, npix, spp, mb, nthreads=16)
    off = _frame(kl, inp, slices=0, brute_cluster=cluster, team=1)
    np.testing.assert_array_equal(off, want)
    for handout in (0, 1):
        for k in KS:
            _same(_frame(kl, inp, slices=k, brute_cluster=cluster, handout=handout), off, (k, handout))
    # an explicit team of one lane, and the auto slice count (off on a tile this small)
    _same(_frame(kl, inp, slices=8, brute_cluster=cluster, team=1), off, "team 1")
    _same(_frame(kl, inp, brute_cluster=cluster), off, "auto")


@pytest.mark.parametrize("cluster", (0, 1))
def test_row_tiles(kl, cornell32, cluster):
    import torch
    inp, want = cornell32
    sc, cam, env, npix, spp, mb, ibl = inp
    _frame(kl, inp, slices=0)   # (uploads the scene)
    w = int(cam[6])
    for r0 in range(3):
        tile = want.reshape(-1, 3 * w)[r0::3].ravel()
        n = 3 * w * _native.tile_rows(npix, w, r0, 3)
        assert n == tile.size
        for k in (0,) + KS:
            kl.native.set_option("slices", k)
            kl.native.set_option("brute_cluster", cluster)
            t = torch.zeros(n, dtype=torch.float32, device="cuda")
            kl.native.render_device(cam, env, npix, spp, mb, r0, 3, t.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(t.cpu(), torch.from_numpy(tile.copy())), (r0, k)


@pytest.mark.parametrize("cluster", (0, 1))
def test_odd_sample_counts(kl, cornell32, cluster):
    inp, _ = cornell32
    # (spp, K): 13 over 5 slices of 2 or 3 samples; 3 samples cap to one slice (every slice at least two);
    # a single sample; none (the reference's 0 / 0 frame)
    for spp, k in ((13, 5), (13, 16), (3, 8), (1, 8), (0, 8)):
        off = _frame(kl, inp, spp=spp, slices=0, brute_cluster=cluster, team=1)
        _same(_frame(kl, inp, spp=spp, slices=k, brute_cluster=cluster), off, (spp, k))
    # a partial last row, and maxBounce 0
    npix = 32 * 31 + 7
    _same(_frame(kl, inp, npix=npix, slices=5, brute_cluster=cluster),
          _frame(kl, inp, npix=npix, slices=0, brute_cluster=cluster, team=1), "partial row")
    _same(_frame(kl, inp, mb=0, slices=8, brute_cluster=cluster),
          _frame(kl, inp, mb=0, slices=0, brute_cluster=cluster, team=1), "maxBounce 0")


@pytest.mark.parametrize("cluster", (0, 1))
def test_early_finishers(kl, cluster):
    """From well outside the open front most camera rays miss the box and some end on the emitter: those
    pixels draw no random number, so slice 0 finishes all their samples (fixed_point), and their later
    slices find nothing to do and retire."""
    inp = _cornell(32, 32, 16, cam_y=-12)
    sc, cam, env, npix, spp, mb, ibl = inp
    off = _frame(kl, inp, slices=0, brute_cluster=cluster, team=1)
    np.testing.assert_array_equal(off, O.render(O.OracleScene.from_scene(sc, ibl), cam, env, npix, spp, mb, nthreads=16))
    c = kl.native.count_work_detail(cam, env, npix, spp, mb)
    assert c["samples"] == npix * spp and c["rays"] < npix * spp // 2   # most pixels: one ray for all samples
    for k in (2, 8, 16):
        _same(_frame(kl, inp, slices=k, brute_cluster=cluster), off, k)


def test_triangle_soups_with_a_lit_sun(kl):
    """Other brute-force scenes (no other bundled scene is small enough for the path): random soups under a
    lit sun and IBL, so the shadow-ray hit carried from slice to slice is used."""
    from tests.test_brute_clusters import GPU_SOUPS
    from tests.test_gpu_nonfinite import SOUP_CAM, SOUP_ENV
    from tests.test_gpu_parity import _random_scene
    assert SOUP_ENV[3] > 0
    for which in GPU_SOUPS[:2]:
        sc = _random_scene(*which)
        inp = (sc, SOUP_CAM, SOUP_ENV, 32 * 32, 16, 4, W.ibl_preview())
        for cluster in (0, 1):
            off = _frame(kl, inp, slices=0, brute_cluster=cluster, team=1)
            for k in (3, 8):
                _same(_frame(kl, inp, slices=k, brute_cluster=cluster), off, (which, cluster, k))


def test_counters(kl, cornell32):
    """The instrumented launch takes the slices too (rt_debug_last_slices: the slice word its kernel got), and the
    first bounce's shadow ray travels with the pixel: the sliced frame traces exactly the unsliced frame's rays."""
    inp, _ = cornell32
    sc, cam, env, npix, spp, mb, ibl = inp
    _frame(kl, inp, slices=0)
    got, word = {}, {}
    for k in (0, 8):
        kl.native.set_option("slices", k)
        kl.native.set_option("team", 1)
        got[k] = kl.native.count_work_detail(cam, env, npix, spp, mb)
        word[k] = _native.last_slices()
    assert word == {0: 0, 8: 8 | 256 << 8}
    for key in ("rays", "samples", "ev_diffuse", "sun_terms"):
        assert got[8][key] == got[0][key], key
    assert got[0]["samples"] == npix * spp


def test_launches_are_sliced(kl, cornell32):
    """What the product launches of this file run: a set slice count reaches the kernel with every pixel sliced,
    also on a tile the team rule would take; slices 0, auto on a small tile and a set team do not."""
    inp, _ = cornell32
    for opts, want in ((dict(slices=5), 5 | 256 << 8), (dict(slices=16, brute_cluster=1), 8 | 256 << 8),
                       (dict(slices=0), 0), (dict(), 0), (dict(slices=8, team=2), 0), (dict(slices=8, team=1), 8 | 256 << 8)):
        _frame(kl, inp, **opts)
        assert _native.last_slices() == want, opts
    _frame(kl, inp, spp=3, slices=8)
    assert _native.last_slices() == 0


@pytest.mark.parametrize("cluster", (0, 1))
def test_progressive_adds(kl, cornell32, cluster):
    """Adds of 16 samples, each cut into slices, against the one-shot frames (tests/test_gpu_progressive.py)."""
    inp, _ = cornell32
    sc, cam, env, npix, spp, mb, ibl = inp
    want = {n: _frame(kl, inp, spp=n, slices=0, brute_cluster=cluster, team=1) for n in (16, 32, 48)}
    for k in (4, 8):
        kl.native.set_option("slices", k)
        kl.native.set_option("brute_cluster", cluster)
        p = kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                 sc.BVH.exportArray, cam, env, npix, mb, ibl)
        for n in (16, 32, 48):
            _same(p.add(16), want[n], (k, n))
        p.close()


BIG = (1024, 704)   # more than two pixels per resident lane of an MI355X (327,680 lanes)


@pytest.fixture(scope="module")
def big_frames(kl):
    """The unsliced frames the large-tile tests compare against: (spp, npix) -> frame."""
    frames = {}

    def get(spp, npix=None):
        if (spp, npix) not in frames:
            frames[spp, npix] = _frame(kl, _cornell(*BIG, spp), npix=npix, slices=0)
            assert _native.last_slices() == 0
        return frames[spp, npix]
    return get


@pytest.mark.parametrize("handout", (0, 1))
@pytest.mark.parametrize("cluster", (0, 1))
def test_auto_on_a_large_tile(kl, big_frames, cluster, handout):
    """The product path: auto slices only the tile's last pixels, so each hand-out group's counter deals whole
    pixels first and then the slices of the rest (take_job with whole jobs).  Both loops, both hand-out orders,
    K = 4 (8 spp), a partial last row, and K = 2 (4 spp)."""
    for spp, k, npix in ((8, 4, None), (8, 4, BIG[0] * (BIG[1] - 1) + 333), (4, 2, None)):
        got = _frame(kl, _cornell(*BIG, spp), npix=npix, brute_cluster=cluster, handout=handout)
        word = _native.last_slices()
        assert word & 0xff == k and 1 <= word >> 8 < 256, (spp, word)   # sliced, and not every pixel
        _same(got, big_frames(spp, npix), (spp, npix))


def test_large_tile_every_pixel_sliced(kl, big_frames):
    _same(_frame(kl, _cornell(*BIG, 4), slices=2), big_frames(4), "every pixel sliced")
    assert _native.last_slices() == 2 | 256 << 8


def test_option_range(kl):
    with pytest.raises(_native.NativeError, match="slices"):
        kl.native.set_option("slices", 17)
    kl.native.set_option("slices", 16)

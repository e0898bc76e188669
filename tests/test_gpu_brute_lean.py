"""Option "brute_lean" on the GPU (rt_kernels.hip render_kernel LEAN; rt_internal.h brute_lean_frame has the rule,
tests/test_brute_lean.py checks it on the host): an all-diffuse one-shot frame runs a one-lane brute-force kernel
without the glossy, glass, IBL and pilot code.  Every frame it renders is the frame of "brute_lean" = 0, byte for
byte; rt_debug_last_launch says which kernel ran (16 in its key's ``brute``).

Frames are Cornell at 4 spp, maxBounce 4 unless a case says otherwise.  128 x 128 with one lane per pixel is the
lock-step kernel; 1024 x 480 is the smallest frame of 1024 columns at which launch_pick takes the clustered, sliced
kernel with a refill threshold on an MI355X (1.5 pixels per resident lane, rt_slices.h brute_auto_slices)."""
import copy

import numpy as np
import pytest
import torch

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests import test_gpu_brute_shell as S

pytestmark = pytest.mark.gpu

DEFAULTS = dict(S.DEFAULTS, brute_lean=-1, fixed_point=1, sun_cache=1, sun_skip=1)
SPP, MB = S.SPP, S.MB
SMALL, LARGE = (128, 128), (1024, 480)
LEAN, SLICED, REFILL = _native.BRUTE_LEAN, _native.BRUTE_SLICED, _native.BRUTE_REFILL


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


def _scene(retype=None, power=None):
    """Cornell; retype = (material, type) gives one material another type, power lights the emitter (its file has 0)."""
    sc, cam, env = S._cornell()
    if retype is not None or power is not None:
        sc = copy.copy(sc)
        m = np.array(sc.materialData, np.float32).reshape(-1, 6).copy()
        if retype is not None:
            m[retype[0], 0] = retype[1]
        if power is not None:
            m[m[:, 0] == 0, 4] = power
        sc.materialData = m.reshape(-1)
    return sc, cam.copy(), env.copy()


def _frame(kl, sc, cam, env, size, spp=SPP, mb=MB, npix=None, tile=None, **opts):
    """One frame (tile = (row0, row_step): that tile of it, rendered on the device as the N-GPU path does)."""
    for key, v in dict(DEFAULTS, **opts).items():
        kl.native.set_option(key, v)
    npix = size[0] * size[1] if npix is None else npix
    cam = S._sized(cam, size)
    out = np.zeros(3 * npix, np.float32)
    args = (sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.BVH.exportArray, cam, env, npix)
    if tile is None:
        kl.launch_Raytracing(out, *args, spp, mb, W.ibl_preview())
        return out, _native.last_launch()
    kl.launch_Raytracing(out, *args, 1, 0, W.ibl_preview())                    # (uploads the scene and the IBL)
    rows = _native.tile_rows(npix, size[0], *tile)
    t = torch.zeros(3 * size[0] * rows, dtype=torch.float32, device="cuda")
    kl.native.render_device(cam, env, npix, spp, mb, tile[0], tile[1], t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return t.cpu().numpy(), _native.last_launch()


def _pair(kl, *args, loop=None, bits=None, **kw):
    """The frame with the option on auto and off: the first ran a lean kernel, the second the same kernel's general
    form, and the two are equal to the byte."""
    on, ll = _frame(kl, *args, **kw)
    assert ll["brute"] & LEAN and ll["team"] == 1 and ll["acc"] == 0 and ll["count"] == 0, ll
    off, l0 = _frame(kl, *args, brute_lean=0, **kw)
    assert l0["brute"] == ll["brute"] & ~LEAN and (l0["grid"], l0["lds"], l0["slices"], l0["refill"]) == \
        (ll["grid"], ll["lds"], ll["slices"], ll["refill"]), (ll, l0)
    assert loop is None or ll["brute"] & 3 == loop, ll
    assert bits is None or ll["brute"] & (SLICED | REFILL) == bits, ll
    assert torch.equal(torch.from_numpy(on).view(torch.int32), torch.from_numpy(off).view(torch.int32))
    return on, ll


def test_the_lock_step_kernel_at_128(kl):
    one, _ = _pair(kl, *_scene(), SMALL, loop=1, bits=0, team=1)
    assert np.isfinite(one).all() and one.max() > 0.0
    again, _ = _frame(kl, *_scene(), SMALL, team=1, brute_lean=1)             # 1 means auto
    S._same(again, one, "brute_lean 1")


def test_the_clustered_sliced_refill_kernel_at_its_smallest_frame(kl):
    _pair(kl, *_scene(), LARGE, loop=3, bits=SLICED | REFILL)


@pytest.mark.parametrize("size,team", [(SMALL, 1), (LARGE, 0)])
def test_one_sample_and_no_bounce(kl, size, team):
    _pair(kl, *_scene(), size, spp=1, team=team)
    _pair(kl, *_scene(), size, mb=0, team=team)
    _pair(kl, *_scene(), size, spp=1, mb=0, team=team)


def test_a_pixel_count_that_is_no_multiple_of_the_width(kl):
    _pair(kl, *_scene(), (128, 101), npix=128 * 100 + 37, loop=1, team=1)
    _pair(kl, *_scene(), (1024, 481), npix=1024 * 480 + 517, loop=3)


@pytest.mark.parametrize("tile", [(0, 2), (1, 8)])
def test_row_tiles_as_the_multi_gpu_path_launches_them(kl, tile):
    _pair(kl, *_scene(), LARGE, tile=tile, team=1)
    _pair(kl, *_scene(), (128, 101), npix=128 * 100 + 37, tile=tile, team=1)


def test_a_camera_that_looks_straight_at_the_light(kl):
    """From under the lit emitter, looking up: the camera ray ends on it, the sample draws nothing and the rest of the
    pixel's samples are summed at bounce 0 (fixed_point).  Against the CPU oracle as well: 64 x 64 at 8 spp."""
    sc, cam, env = _scene(power=3.0)
    cam[0:3] = [0.01, 0.1, 0.0]
    cam[3:6] = [90.0, 0.0, 0.0]
    size = (64, 64)
    got, _ = _pair(kl, sc, cam, env, size, spp=8, loop=1, team=1)
    px = got.reshape(-1, 3)
    assert (px[32 * 64 + 32] == 1.0).all() and (px >= 1.0).all(1).sum() > 400
    want = O.render(O.OracleScene.from_scene(sc, W.ibl_preview()), S._sized(cam, size), env, 64 * 64, 8, MB, nthreads=16)
    S._same(got, want, "the oracle")
    _pair(kl, sc, cam, env, LARGE, loop=3)


@pytest.mark.parametrize("sun", [0.0, 0.5, -0.0])
def test_sun_skip_on_and_off(kl, sun):
    sc, cam, env = _scene()
    env[3] = sun
    for size, team in ((SMALL, 1), (LARGE, 0)):
        _pair(kl, sc, cam, env, size, team=team)
        _pair(kl, sc, cam, env, size, team=team, sun_skip=0)


def _general(kl, *args, **kw):
    """An ineligible launch: the general kernel with the option on auto and off, and the same frame."""
    on, ll = _frame(kl, *args, **kw)
    off, l0 = _frame(kl, *args, brute_lean=0, **kw)
    for n in (ll, l0):
        assert n["brute"] & 3 in (1, 3) and not n["brute"] & LEAN, n
    assert ll == l0
    assert torch.equal(torch.from_numpy(on).view(torch.int32), torch.from_numpy(off).view(torch.int32))


@pytest.mark.parametrize("size,team", [(SMALL, 1), (LARGE, 0)])
def test_ineligible_launches_run_the_general_kernel(kl, size, team):
    _general(kl, *_scene(retype=(1, 2)), size, team=team)                      # a glossy material
    _general(kl, *_scene(retype=(2, 3)), size, team=team)                      # a glass material
    sc, cam, env = _scene()
    env[4] = 0.5                                                               # an IBL with power
    _general(kl, sc, cam, env, size, team=team)
    env[4] = -0.0                                                              # zero, but not the lean loop's +0
    _general(kl, sc, cam, env, size, team=team)
    _general(kl, *_scene(), size, team=team, fixed_point=0)
    _general(kl, *_scene(), size, team=team, sun_cache=0)


@pytest.mark.parametrize("size,team", [(SMALL, 1), (LARGE, 0)])
def test_a_progressive_add_runs_the_general_kernel(kl, size, team):
    sc, cam, env = _scene()
    got = {}
    for mode in (-1, 0):
        for key, v in dict(DEFAULTS, team=team, brute_lean=mode).items():
            kl.native.set_option(key, v)
        p = kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                 sc.BVH.exportArray, S._sized(cam, size), env, size[0] * size[1], MB, W.ibl_preview())
        for n in (2, 2):
            out = p.add(n)
            ll = _native.last_launch()
            assert ll["acc"] == 1 and ll["brute"] & 3 in (1, 3) and not ll["brute"] & LEAN, ll
        got[mode] = out.copy()
        p.close()
    S._same(got[-1], got[0], "2 x 2 spp")
    one, ll = _frame(kl, sc, cam, env, size, team=team)                        # ... and is the lean one-shot frame
    assert ll["brute"] & LEAN
    S._same(got[-1], one, "the one-shot frame")


def test_the_option_takes_minus_one_to_one(kl):
    for bad in (-2, 2):
        with pytest.raises(_native.NativeError, match="brute_lean must be -1"):
            kl.native.set_option("brute_lean", bad)

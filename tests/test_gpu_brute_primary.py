"""Option "brute_primary" on the GPU (rt_kernels.hip render_kernel PRE / PREPASS; rt_internal.h kBrutePrimary): a lean
sliced launch traces its camera rays in a pre-pass, which writes every pixel's slice record, and its loop kernel starts
every job from such a record.  Every frame it renders is the frame of "brute_primary" = 0, byte for byte;
rt_debug_last_launch says which form ran (its last field, ``primary``; the key's ``brute`` is the same either way).

Frames are Cornell at 4 spp, maxBounce 4 unless a case says otherwise.  A launch is eligible when it is lean
(tests/test_gpu_brute_lean.py) and sliced: 128 x 128 with "slices" = 2 slices every pixel (the lock-step loop, or the
clustered one with "brute_cluster" = 1); 1024 x 480 is the smallest frame of 1024 columns at which launch_pick slices
on its own (the clustered loop with a refill threshold; on an MI355X still every pixel), and 1024 x 704 the smallest at
which it hands out whole jobs first and only the tile's last pixels in slices."""
import numpy as np
import pytest
import torch

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests import test_gpu_brute_lean as L
from tests import test_gpu_brute_shell as S

pytestmark = pytest.mark.gpu

DEFAULTS = dict(L.DEFAULTS, brute_primary=-1, slices=-1, brute_refill=-1)
SPP, MB = L.SPP, L.MB
SMALL, LARGE, WHOLE, ODD = (128, 128), (1024, 480), (1024, 704), (128, 101)
ODD_NPIX = 128 * 100 + 37
LEAN, SLICED, REFILL = _native.BRUTE_LEAN, _native.BRUTE_SLICED, _native.BRUTE_REFILL
EVERY = dict(slices=2, team=1)            # every pixel of a small frame sliced, one lane per pixel


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


def _frame(kl, *args, **kw):
    return L._frame(kl, *args, **dict(DEFAULTS, **kw))


def _bits(a):
    return torch.from_numpy(a).view(torch.int32)


def _pair(kl, *args, loop=None, bits=None, **kw):
    """The frame with the option on auto and off: a pre-pass and the loop that starts from its records, then the same
    lean sliced kernel with its own camera rays -- the same launch otherwise, and the same frame to the byte."""
    on, ll = _frame(kl, *args, **kw)
    off, l0 = _frame(kl, *args, brute_primary=0, **kw)
    assert ll["primary"] == 1 and l0["primary"] == 0, (ll, l0)
    assert ll["brute"] == l0["brute"] and ll["brute"] & LEAN and ll["brute"] & SLICED, (ll, l0)
    assert (ll["grid"], ll["lds"], ll["slices"], ll["refill"]) == (l0["grid"], l0["lds"], l0["slices"], l0["refill"]), (ll, l0)
    assert loop is None or ll["brute"] & 3 == loop, ll
    assert bits is None or ll["brute"] & (SLICED | REFILL) == bits, ll
    assert torch.equal(_bits(on), _bits(off))
    return on, ll


def _camera(name):
    sc, cam, env = L._scene()
    if name == "inside":
        cam[0:3] = [0.2, -0.6, -0.1]
        cam[3:6] = [-6.0, 10.0, 0.0]
    elif name == "away":                  # the bench camera turned round: no camera ray meets the scene
        cam[3:6] = [0.0, 0.0, 180.0]
    else:
        assert name == "bench"            # (0, -3.5, 0): outside the room, in front of its open side
    return sc, cam, env


def test_the_lock_step_kernel_with_every_pixel_sliced(kl):
    one, ll = _pair(kl, *L._scene(), SMALL, loop=1, bits=SLICED, **EVERY)
    assert ll["slices"] == 2 | 256 << 8, ll
    assert np.isfinite(one).all() and one.max() > 0.0
    again, l1 = _frame(kl, *L._scene(), SMALL, brute_primary=1, **EVERY)       # 1 means auto
    assert l1["primary"] == 1
    S._same(again, one, "brute_primary 1")


def test_the_clustered_loop_with_every_pixel_sliced(kl):
    _pair(kl, *L._scene(), SMALL, loop=3, bits=SLICED, brute_cluster=1, **EVERY)


def test_the_auto_rule_at_its_smallest_frame(kl):
    _pair(kl, *L._scene(), LARGE, loop=3, bits=SLICED | REFILL)


def test_whole_jobs_before_the_slices(kl):
    """Auto slices the last two pixels per resident lane (rt_slices.h brute_slice_tail): on an MI355X's 327,680 lanes
    a frame of more than 655,360 pixels is the smallest that hands out whole jobs, which start from a record too."""
    _, ll = _pair(kl, *L._scene(), WHOLE, loop=3, bits=SLICED | REFILL)
    assert 0 < ll["slices"] >> 8 < 256, ll                                     # only the tile's last pixels are sliced
    _pair(kl, *L._scene(), (1024, 705), npix=1024 * 704 + 517, loop=3)         # ... with a partial last row


def test_a_partial_last_row(kl):
    _pair(kl, *L._scene(), ODD, npix=ODD_NPIX, loop=1, **EVERY)
    _pair(kl, *L._scene(), (1024, 481), npix=1024 * 480 + 517, loop=3)


@pytest.mark.parametrize("tile", [(0, 2), (1, 2), (1, 8)])
def test_row_tiles_as_the_multi_gpu_path_launches_them(kl, tile):
    _pair(kl, *L._scene(), ODD, npix=ODD_NPIX, tile=tile, **EVERY)


def test_fewer_pixels_than_a_wave(kl):
    _pair(kl, *L._scene(), (37, 1), npix=37, brute_refill=64, **EVERY)


def test_two_samples_a_slice_and_no_bounce(kl):
    _pair(kl, *L._scene(), SMALL, spp=4, **EVERY)
    _pair(kl, *L._scene(), SMALL, mb=0, **EVERY)
    _pair(kl, *L._scene(), LARGE, mb=0)


@pytest.mark.parametrize("name", ["inside", "bench", "away"])
def test_cameras(kl, name):
    one, _ = _pair(kl, *_camera(name), SMALL, **EVERY)
    assert (one.max() == 0.0) == (name == "away")                              # away: every camera ray misses
    _pair(kl, *_camera(name), LARGE, loop=3)


def test_a_camera_that_looks_straight_at_the_light(kl):
    """test_gpu_brute_lean's case: the camera ray ends on the lit emitter, so every sample ends at bounce 0 and a slice's
    job sums its samples without a ray.  Against the CPU oracle as well: 64 x 64 at 8 spp."""
    sc, cam, env = L._scene(power=3.0)
    cam[0:3] = [0.01, 0.1, 0.0]
    cam[3:6] = [90.0, 0.0, 0.0]
    size = (64, 64)
    got, _ = _pair(kl, sc, cam, env, size, spp=8, loop=1, **EVERY)
    px = got.reshape(-1, 3)
    assert (px[32 * 64 + 32] == 1.0).all() and (px >= 1.0).all(1).sum() > 400
    want = O.render(O.OracleScene.from_scene(sc, W.ibl_preview()), S._sized(cam, size), env, 64 * 64, 8, MB, nthreads=16)
    S._same(got, want, "the oracle")
    _pair(kl, sc, cam, env, LARGE, loop=3)


@pytest.mark.parametrize("sun", [0.0, 0.5, -0.0])
def test_sun_term_with_sun_skip_on_and_off(kl, sun):
    sc, cam, env = L._scene()
    env[3] = sun
    for size, kw in ((SMALL, EVERY), (LARGE, {})):
        _pair(kl, sc, cam, env, size, **kw)
        _pair(kl, sc, cam, env, size, sun_skip=0, **kw)


def test_two_frames_with_two_cameras_on_one_launcher(kl):
    """The records are written by every launch: a second camera's frame is its own, not the first's."""
    want = {}
    for name in ("bench", "inside"):
        want[name], l0 = _frame(kl, *_camera(name), SMALL, brute_primary=0, **EVERY)
        assert l0["primary"] == 0
    assert not torch.equal(_bits(want["bench"]), _bits(want["inside"]))
    for name in ("bench", "inside", "bench"):
        got, ll = _frame(kl, *_camera(name), SMALL, **EVERY)
        assert ll["primary"] == 1
        assert torch.equal(_bits(got), _bits(want[name])), name


def _ineligible(kl, *args, **kw):
    """No pre-pass with the option on auto or off: the same launch and the same frame."""
    on, ll = _frame(kl, *args, **kw)
    off, l0 = _frame(kl, *args, brute_primary=0, **kw)
    assert ll["primary"] == 0 and ll == l0, (ll, l0)
    assert torch.equal(_bits(on), _bits(off))
    return ll


def test_ineligible_launches_keep_their_kernels(kl):
    ll = _ineligible(kl, *L._scene(), SMALL, slices=0, team=1)                 # lean, not sliced
    assert ll["brute"] & LEAN and not ll["brute"] & SLICED, ll
    ll = _ineligible(kl, *L._scene(retype=(1, 2)), SMALL, **EVERY)             # a glossy material: sliced, not lean
    assert ll["brute"] & SLICED and not ll["brute"] & LEAN, ll
    sc, cam, env = L._scene()
    env[4] = 0.5                                                               # an IBL with power: not lean
    ll = _ineligible(kl, sc, cam, env, SMALL, **EVERY)
    assert ll["brute"] & SLICED and not ll["brute"] & LEAN, ll
    _ineligible(kl, *L._scene(), LARGE, slices=0)


def test_a_progressive_add_keeps_its_kernel(kl):
    sc, cam, env = L._scene()
    got = {}
    for mode in (-1, 0):
        for key, v in dict(DEFAULTS, brute_primary=mode, **EVERY).items():
            kl.native.set_option(key, v)
        p = kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                 sc.BVH.exportArray, S._sized(cam, SMALL), env, SMALL[0] * SMALL[1], MB, W.ibl_preview())
        notes = []
        for n in (2, 2):
            out = p.add(n)
            notes.append(_native.last_launch())
            assert notes[-1]["acc"] == 1 and notes[-1]["primary"] == 0, notes[-1]
        got[mode] = (out.copy(), notes)
        p.close()
    assert got[-1][1] == got[0][1]
    S._same(got[-1][0], got[0][0], "2 x 2 spp")


def test_the_option_takes_minus_one_to_one(kl):
    for bad in (-2, 2):
        with pytest.raises(_native.NativeError, match="brute_primary must be -1"):
            kl.native.set_option("brute_primary", bad)

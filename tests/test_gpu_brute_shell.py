"""Option "brute_shell" (rt_debug.h): the clustered brute-force loop tests a room's walls from one set of shared
plane distances (rt_device.h trace_brute_compact, scene_pack.cpp build_shell).  Every frame is that of
"brute_shell" = 0, bit for bit, and the CPU oracle's.

Each case runs at two sizes, 4 spp, maxBounce 4.  At 64 x 64 the one-lane clustered kernel runs only with forced
clusters and team = 1 (as in tests/test_gpu_brute_cluster.py), and forced clusters take these scenes' walls into
clusters: no shell, the option must change nothing.  The shell is taken among the single slots of the automatic
clusters, and those run the clustered kernel only on a tile of at least a pixel per resident lane (launch_pick):
1024 x 352, where the launch reports the shell (rt_debug_last_launch)."""
import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests.test_brute_shell import six_face_room, one_ulp_room

pytestmark = pytest.mark.gpu

DEFAULTS = {"brute_shell": -1, "brute_cluster": -1, "team": 0}
SPP, MB = 4, 4
SMALL, LARGE = (64, 64), (1024, 352)     # LARGE: more pixels than an MI355X keeps lanes resident (327,680)
NAN, INF = np.float32(np.nan), np.float32(np.inf)


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


def _cornell():
    sc, cam, env, *_ = W.PARITY_CASES["cornell_64_s4"].inputs()
    return sc, np.asarray(cam, np.float32), np.asarray(env, np.float32)


def _case(name):
    """(scene, camera, env): the camera's size fields are set per frame."""
    if name in ("six_face_room", "one_ulp_room"):
        sc = six_face_room() if name == "six_face_room" else one_ulp_room()
        _, cam, env = _cornell()
        cam = cam.copy()
        cam[0:3] = [0.1, -0.8, 0.2]          # inside the closed room
        cam[3:6] = [8.0, -5.0, 0.0]
        return sc, cam, env
    sc, cam, env = _cornell()
    cam = cam.copy()
    if name == "cornell_inside":
        cam[0:3] = [0.2, -0.6, -0.1]
        cam[3:6] = [-6.0, 10.0, 0.0]
    elif name == "cornell_cam_nan":
        cam[0] = NAN
    elif name == "cornell_cam_inf":
        cam[0:3] = INF
    else:
        assert name == "cornell_bench_camera"   # (0, -3.5, 0): outside the room, in front of its open side
    return sc, cam, env


CASES = ["cornell_bench_camera", "cornell_inside", "six_face_room", "one_ulp_room", "cornell_cam_nan", "cornell_cam_inf"]
_refs = {}


def _sized(cam, size):
    cam = cam.copy()
    cam[6], cam[7] = size
    return cam


def _want(name, size):
    """The CPU oracle's frame, computed once per (case, size)."""
    if (name, size) not in _refs:
        sc, cam, env = _case(name)
        _refs[name, size] = O.render(O.OracleScene.from_scene(sc, W.ibl_preview()), _sized(cam, size), env,
                                     size[0] * size[1], SPP, MB, nthreads=16)
    return _refs[name, size]


def _frame(kl, name, size, **opts):
    sc, cam, env = _case(name)
    for key, v in dict(DEFAULTS, **opts).items():
        kl.native.set_option(key, v)
    npix = size[0] * size[1]
    out = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                         sc.BVH.exportArray, _sized(cam, size), env, npix, SPP, MB, W.ibl_preview())
    assert kl.native.scene_info()["brute_records"] > 0
    return out, _native.last_launch()


def _same(a, b, msg):
    # the frames' bits (a NaN pixel equals itself)
    assert a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes(), msg


@pytest.mark.parametrize("name", CASES)
def test_large_tile_walks_the_shell_and_equals_off_and_the_oracle(kl, name):
    off, ll = _frame(kl, name, LARGE, brute_shell=0)
    assert ll["brute"] & 3 == 3 and ll["shell"] == 0
    np.testing.assert_array_equal(off, _want(name, LARGE))
    for mode in (-1, 1):
        got, ll = _frame(kl, name, LARGE, brute_shell=mode)
        assert ll["brute"] & 3 == 3 and ll["shell"] == 1, (mode, ll)
        _same(got, off, mode)


@pytest.mark.parametrize("name", CASES)
def test_64x64_equals_off_and_the_oracle(kl, name):
    """The clustered kernel on forced clusters (no shell among their singles) and the lock-step kernel."""
    want = _want(name, SMALL)
    for cluster in (1, -1):
        off, ll = _frame(kl, name, SMALL, brute_shell=0, brute_cluster=cluster, team=1)
        assert ll["brute"] & 3 == (3 if cluster == 1 else 1) and ll["shell"] == 0
        np.testing.assert_array_equal(off, want)
        for mode in (-1, 1):
            got, ll = _frame(kl, name, SMALL, brute_shell=mode, brute_cluster=cluster, team=1)
            assert ll["shell"] == 0, (cluster, mode, ll)
            _same(got, off, (cluster, mode))


def test_launch_field_reports_the_shell_only_where_it_runs(kl):
    name = "cornell_bench_camera"
    for opts, shell in ((dict(), 1), (dict(team=1), 1), (dict(brute_shell=1), 1), (dict(brute_shell=0), 0),
                        (dict(team=4), 0), (dict(brute_cluster=0), 0), (dict(brute_cluster=0, brute_shell=1), 0)):
        got, ll = _frame(kl, name, LARGE, **opts)
        assert ll["shell"] == shell, (opts, ll)
        assert (ll["brute"] & 3 == 3) == (opts.get("team", 0) <= 1 and opts.get("brute_cluster", -1) != 0), (opts, ll)
        np.testing.assert_array_equal(got, _want(name, LARGE))
    with pytest.raises(_native.NativeError, match="brute_shell"):
        kl.native.set_option("brute_shell", 2)


def _progressive(kl, name, size):
    sc, cam, env = _case(name)
    return kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                sc.BVH.exportArray, _sized(cam, size), env, size[0] * size[1], MB, W.ibl_preview())


@pytest.mark.parametrize("name", ("cornell_bench_camera", "six_face_room"))
def test_progressive_add(kl, name):
    """The rt_accum instantiation of the kernel: 1 + 2 + 1 samples."""
    for mode in (0, -1):
        kl.native.set_option("brute_shell", mode)
        p = _progressive(kl, name, LARGE)
        for n in (1, 2, 1):
            got = p.add(n)
            ll = _native.last_launch()
            assert ll["acc"] == 1 and ll["brute"] & 3 == 3 and ll["shell"] == (mode != 0), (mode, ll)
        p.close()
        np.testing.assert_array_equal(got, _want(name, LARGE))


@pytest.mark.parametrize("name", ("cornell_inside", "one_ulp_room"))
def test_adaptive_add_selected(kl, name):
    """The rt_adaptive instantiation: 2 samples, then 2 more for every pixel through the list."""
    for mode in (0, -1):
        kl.native.set_option("brute_shell", mode)
        p = _progressive(kl, name, LARGE)
        p.add(2)
        p.select_all()
        got = p.add_selected(2)
        ll = _native.last_launch()
        assert ll["acc"] == 2 and ll["brute"] & 3 == 3 and ll["shell"] == (mode != 0), (mode, ll)
        p.close()
        np.testing.assert_array_equal(got, _want(name, LARGE))

"""Option "brute_cluster" (rt_debug.h): the clustered brute-force loop (rt_device.h trace_brute_compact, CLU)
renders the frame of the lock-step loop, bit for bit.  -1 (auto) and 1 (force) against 0 (off).  The clustered
loop is the one-lane kernel's, and tiles this small would run teams of 4 by default, so every comparison runs
with team = 1 as well as with the default team size.  Auto keeps tiles of less than a pixel per resident lane on
the lock-step kernel (rt_kernels.hip launch_pick), so on these frames it is force that runs the clustered kernel;
auto must still give the same bits."""
import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests.test_brute_clusters import GPU_SOUPS
from tests.test_gpu_parity import _random_scene

pytestmark = pytest.mark.gpu

MODES = (-1, 1)


@pytest.fixture(scope="module")
def kl():
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    k = KernelLauncher(None, None, 0, None)
    yield k
    k.close()


def _reset(kl):
    kl.native.set_option("brute_cluster", -1)
    kl.native.set_option("team", 0)


def _frame(kl, sc, bvh, cam, env, npix, spp, mb, ibl, cluster, team):
    kl.native.set_option("brute_cluster", cluster)
    kl.native.set_option("team", team)
    out = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, bvh, cam, env,
                         npix, spp, mb, ibl)
    return out


def _same(a, b, msg):
    # torch.equal's meaning on the frames' bits (a NaN pixel equals itself)
    assert a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes(), msg


def _check_modes(kl, sc, bvh, cam, env, npix, spp, mb, ibl, want=None):
    try:
        off = _frame(kl, sc, bvh, cam, env, npix, spp, mb, ibl, 0, 1)
        assert kl.native.scene_info()["brute_records"] > 0
        if want is not None:
            np.testing.assert_array_equal(off, want)
        for team in (1, 0):
            for mode in MODES:
                _same(_frame(kl, sc, bvh, cam, env, npix, spp, mb, ibl, mode, team), off, (mode, team))
        return off
    finally:
        _reset(kl)


def test_cornell_64_s4_equals_off_and_the_oracle(kl):
    sc, cam, env, npix, spp, mb, ibl = W.PARITY_CASES["cornell_64_s4"].inputs()
    want = O.render(O.OracleScene.from_scene(sc, ibl), cam, env, npix, spp, mb, nthreads=16)
    _check_modes(kl, sc, sc.BVH.exportArray, cam, env, npix, spp, mb, ibl, want)


def test_cornell_partial_waves_and_last_row(kl):
    sc, cam, env, npix, spp, mb, ibl = W.PARITY_CASES["cornell_64_s4"].with_size(50, 37, 3).inputs()
    assert npix == 50 * 37
    _check_modes(kl, sc, sc.BVH.exportArray, cam, env, npix, spp, mb, ibl)
    # a frame whose last row is partial (the reference's imgSize need not be a whole number of rows)
    _check_modes(kl, sc, sc.BVH.exportArray, cam, env, npix - 13, spp, mb, ibl)


def test_cornell_max_bounce_0(kl):
    sc, cam, env, npix, spp, mb, ibl = W.PARITY_CASES["cornell_64_s4"].inputs()
    _check_modes(kl, sc, sc.BVH.exportArray, cam, env, npix, spp, 0, ibl)


def test_cornell_row_tile_1_of_3(kl):
    import torch
    sc, cam, env, npix, spp, mb, ibl = W.PARITY_CASES["cornell_64_s4"].inputs()
    w = int(cam[6])
    n = 3 * w * _native.tile_rows(npix, w, 1, 3)
    try:
        full = _frame(kl, sc, sc.BVH.exportArray, cam, env, npix, spp, mb, ibl, 0, 1)
        want = full.reshape(-1, 3 * w)[1::3].ravel()
        for mode in (0,) + MODES:
            kl.native.set_option("brute_cluster", mode)
            t = torch.zeros(n, dtype=torch.float32, device="cuda")
            kl.native.render_device(cam, env, npix, spp, mb, 1, 3, t.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(t.cpu(), torch.from_numpy(want.copy())), mode
    finally:
        _reset(kl)


def test_cornell_accumulation(kl):
    """One rt_accum add sequence (the ACC instantiation of the kernel): 1 + 2 + 1 samples."""
    sc, cam, env, npix, spp, mb, ibl = W.PARITY_CASES["cornell_64_s4"].inputs()
    try:
        off = _frame(kl, sc, sc.BVH.exportArray, cam, env, npix, 4, mb, ibl, 0, 1)
        for mode in MODES:
            kl.native.set_option("brute_cluster", mode)
            p = kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                     sc.BVH.exportArray, cam, env, npix, mb, ibl)
            for n in (1, 2, 1):
                got = p.add(n)
            p.close()
            _same(got, off, mode)
    finally:
        _reset(kl)


@pytest.mark.parametrize("which", GPU_SOUPS, ids=str)
def test_forced_clusters_on_soups(kl, which):
    """Soups whose forced clusters have sizes that are no multiple of 8 and reach both the compacted and the
    lock-step branch (tests/test_brute_clusters.py test_gpu_soups_reach_both_branches)."""
    from tests.test_gpu_nonfinite import SOUP_CAM, SOUP_ENV
    sc = _random_scene(*which)
    _check_modes(kl, sc, sc.BVH.exportArray, SOUP_CAM, SOUP_ENV, 32 * 32, 4, 4, W.ibl_preview())


def test_nonfinite_cameras(kl):
    """The non-finite camera classes of tests/test_gpu_nonfinite.py on Cornell and a soup: a NaN ray passes every
    union and every box (the wave takes the lock-step branch); the frame is the lock-step loop's."""
    from tests.test_gpu_nonfinite import CAMERA_CASES, NPIX, SPP, MB, poisoned
    for name in ("cornell", "soup5"):
        for case in CAMERA_CASES:
            _, sc = poisoned(name, case)
            _check_modes(kl, sc, sc.bvh, sc.cam, sc.env, NPIX, SPP, MB, W.ibl_preview())

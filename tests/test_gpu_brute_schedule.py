"""The lock-step walks of the brute-force kernels (rt_device.h trace_brute_compact): the clustered loop tests its
single slots and a cluster's members in whole groups of 4 and then the last 1-3 alone; the unclustered loop tests
brute_box in whole groups.  Four scenes whose clusters and box counts leave every tail length
(tests/test_brute_schedule.py test_scenes_cover_every_tail_length): brute_cluster 1 (force) and -1 (auto) against
0 (off), bit for bit, on single lanes (team = 1) -- as a one-shot frame, with two sample slices, as a progressive
accumulation, as one add of listed pixels, and as a row tile through render_device, which auto gives to the
unclustered kernel."""
import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests.test_gpu_parity import _random_scene

pytestmark = pytest.mark.gpu

MODES = (1, -1)
SCENES = ["cornell", (11, 23), (2, 64), (9, 33)]
DEFAULTS = {"slices": -1, "brute_cluster": -1, "team": 0}


@pytest.fixture(scope="module")
def kl():
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    k = KernelLauncher(None, None, 0, None)
    yield k
    k.close()


@pytest.fixture(scope="module")
def oracle_frame():
    sc, cam, env, npix, spp, mb, ibl = W.PARITY_CASES["cornell_64_s4"].inputs()
    return O.render(O.OracleScene.from_scene(sc, ibl), cam, env, npix, spp, mb, nthreads=16)


def _inputs(which):
    if which == "cornell":
        sc, cam, env, npix, spp, mb, ibl = W.PARITY_CASES["cornell_64_s4"].inputs()
        return sc, cam, env, npix, spp, mb, ibl
    from tests.test_gpu_nonfinite import SOUP_CAM, SOUP_ENV
    return _random_scene(*which), SOUP_CAM, SOUP_ENV, 32 * 32, 4, 4, W.ibl_preview()


def _frame(kl, inp, **opts):
    sc, cam, env, npix, spp, mb, ibl = inp
    for k, v in dict(DEFAULTS, team=1, **opts).items():
        kl.native.set_option(k, v)
    out = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.BVH.exportArray,
                         cam, env, npix, spp, mb, ibl)
    return out


def _reset(kl):
    for k, v in DEFAULTS.items():
        kl.native.set_option(k, v)


def _same(a, b, msg):
    assert a.view(np.uint32).tobytes() == b.view(np.uint32).tobytes(), msg


@pytest.mark.parametrize("which", SCENES, ids=str)
def test_every_launch_form_equals_the_unclustered_frame(kl, oracle_frame, which):
    import torch
    inp = _inputs(which)
    sc, cam, env, npix, spp, mb, ibl = inp
    assert spp == 4
    try:
        off = _frame(kl, inp, brute_cluster=0, slices=0)
        assert kl.native.scene_info()["brute_records"] > 0
        if which == "cornell":
            np.testing.assert_array_equal(off, oracle_frame)
        w = int(cam[6])
        tile = off.reshape(-1, 3 * w)[1::3].ravel()
        assert tile.size == 3 * w * _native.tile_rows(npix, w, 1, 3)
        for mode in MODES:
            _same(_frame(kl, inp, brute_cluster=mode, slices=0), off, (mode, "one shot"))
            _same(_frame(kl, inp, brute_cluster=mode, slices=2), off, (mode, "two slices"))
            assert _native.last_slices() == 2 | 256 << 8
            # (the options of the last frame hold: this mode on single lanes)
            kl.native.set_option("slices", -1)
            p = kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                     sc.BVH.exportArray, cam, env, npix, mb, ibl)
            for n in (1, 2, 1):
                got = p.add(n)
            p.close()
            _same(got, off, (mode, "accumulation"))
            p = kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                     sc.BVH.exportArray, cam, env, npix, mb, ibl)
            p.add(2)
            p.select_all()
            got = p.add_selected(2)
            p.close()
            _same(got, off, (mode, "listed add"))
            t = torch.zeros(tile.size, dtype=torch.float32, device="cuda")
            kl.native.render_device(cam, env, npix, spp, mb, 1, 3, t.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            _same(t.cpu().numpy(), tile, (mode, "row tile 1 of 3"))
    finally:
        _reset(kl)

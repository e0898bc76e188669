"""Which kernel a launch runs (rt_debug_last_launch): the key choose_kernel and launch_pick (rt_kernels.hip) make
of the scene, the frame, the options and the tile.  The frames of these launches are compared bit for bit
elsewhere (the forced-schedule tests); here each case renders a tiny frame and asserts the key.

The auto choices for the clustered loop, the refill threshold and the slices go by the device's resident lanes, so a
default launch asserts only its engine and that the key agrees with the parameters its kernel got.  At 32 x 32
the brute-force team rule (tile pixels x 4 <= resident lanes) takes the tile, so the cases about the one-lane
kernels set ``team 1``."""
import functools

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests.deep_bvh import caterpillar_scene

pytestmark = pytest.mark.gpu

DEFAULTS = {"traversal": _native.RT_TRAVERSAL_FAST, "bvh": _native.RT_BVH_SAH, "brute_max": 64, "brute_cluster": -1,
            "brute_refill": -1, "slices": -1, "team": 0, "walk_team": 0, "bvh_width": 0, "wdq": 1, "step": 0,
            "stack_lds": 0, "pilot": 0}
SPP, MB = 4, 4
FAST, REF = 0, 1


@functools.lru_cache(maxsize=None)
def _scene(name, w=32, h=32):
    """(arrays for set_scene, cam, env) of the bundled Cornell box or monkey, or of the 40-level chain."""
    if name == "chain":
        a = caterpillar_scene(40)
        cam = np.array([0, -3.5, 0, 0, 0, 0, w, h, 1, 45 * 3.14 / 180], np.float32)
        return ((a["V_p"], a["V_n"], a["V_uv"], a["faceData"], a["materialData"], a["bvh"]), cam,
                np.array([90, 0, 0, 1.0, 1.0], np.float32))
    case = {"cornell": "cornell_64_s4", "monkey": "monkey_c3_64_s4"}[name]
    sc, cam, env, *_ = W.PARITY_CASES[case].with_size(w, h, SPP).inputs()
    return (sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray), cam, env


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(device_ids=[0])
    c.set_env(W.ibl_preview())
    yield c
    c.close()


def _prepare(ctx, name, opts, w=32, h=32):
    arrays, cam, env = _scene(name, w, h)
    for key, v in dict(DEFAULTS, **opts).items():
        ctx.set_option(key, v)
    ctx.set_scene(*arrays)
    return cam, env, w * h


def _consistent(n):
    """The key agrees with the parameters the kernel got."""
    assert n["ts"] == n["walk_team"] and n["grid"] >= 1
    product = not n["count"] and not n["log"]
    if n["brute"]:
        assert not n["resume"] and not n["smem"] and not n["ovf"] and n["trav"] == FAST
        assert bool(n["brute"] & _native.BRUTE_SLICED) == (n["slices"] != 0)
        if product:
            assert bool(n["brute"] & _native.BRUTE_REFILL) == (n["refill"] > 1)
        assert (n["brute"] & 3 == 2) == (n["team"] > 1)
        assert n["brute"] & 3 != 2 or n["brute"] == 2   # teams: neither sliced nor with a threshold
    else:
        assert n["team"] == 1 and n["refill"] == 0
    if not n["resume"]:
        assert n["ts"] == 1 and n["wide"] == 0 and n["step"] == 1
    return n


def _render(ctx, name, w=32, h=32, **opts):
    cam, env, npix = _prepare(ctx, name, opts, w, h)
    out = ctx.render(cam, env, npix, SPP, MB)
    assert np.isfinite(out).all()
    n = _consistent(_native.last_launch())
    assert (n["count"], n["log"], n["acc"]) == (0, 0, 0)
    return n


def test_default_cornell_is_brute_force(ctx):
    n = _render(ctx, "cornell")
    assert n["trav"] == FAST and n["brute"] & 3 in (1, 2, 3) and n["resume"] == 0
    n = _render(ctx, "cornell", team=1)
    assert n["brute"] & 3 in (1, 3) and n["team"] == 1 and n["resume"] == 0


def test_brute_max_0_walks_the_staged_tree(ctx):
    n = _render(ctx, "cornell", brute_max=0)
    assert (n["trav"], n["brute"], n["smem"], n["ovf"]) == (FAST, 0, 1, 0)


@pytest.mark.parametrize("stack_lds", (0, 8))
def test_deep_tree_takes_the_overflow_walk(ctx, stack_lds):
    """The 40-level chain walked as built: 39 entries deep, beyond the 20 (or the 8 asked for) kept in LDS; small
    enough to stage, but the staged walks have no overflow."""
    n = _render(ctx, "chain", bvh=_native.RT_BVH_REFERENCE, brute_max=0, stack_lds=stack_lds)
    assert ctx.scene_info()["depth"] > 20
    assert (n["trav"], n["brute"], n["ovf"], n["smem"]) == (FAST, 0, 1, 0)


def test_step_2_walks_in_rounds(ctx):
    assert _render(ctx, "cornell", brute_max=0, step=1)["step"] == 1
    n = _render(ctx, "cornell", brute_max=0, step=2)
    assert n["resume"] == 1 and n["step"] == 0 and n["ts"] == 1


def test_wide_walk(ctx):
    n = _render(ctx, "monkey", brute_max=0, bvh_width=4)
    assert n["resume"] == 1 and n["wide"] >= 1 and n["smem"] == 0 and n["brute"] == 0 and n["ts"] == 1
    n = _render(ctx, "monkey", brute_max=0, bvh_width=4, wdq=0)
    assert n["wide"] == 1 and n["smem"] == 0
    n = _render(ctx, "monkey", brute_max=0, bvh_width=4, step=2)
    assert (n["wide"], n["step"]) == (1, 0)


@pytest.mark.parametrize("ts", (2, 4, 8))
def test_walk_teams(ctx, ts):
    n = _render(ctx, "monkey", brute_max=0, bvh_width=2, walk_team=ts)
    assert (n["resume"], n["step"], n["wide"], n["ts"], n["walk_team"]) == (1, 1, 0, ts, ts)


def test_brute_teams(ctx):
    n = _render(ctx, "cornell", team=4)
    assert n["brute"] == 2 and n["team"] == 4
    n = _render(ctx, "cornell", 16, 16)   # one 16 x 16 tile: 256 pixels x 4 lanes fit any device
    assert n["brute"] == 2 and n["team"] == 4


def test_set_slices(ctx):
    n = _render(ctx, "cornell", slices=2)
    assert n["brute"] & _native.BRUTE_SLICED and n["team"] == 1 and n["slices"] == (2 | 256 << 8)
    assert n["slices"] == _native.last_slices()


def test_refill(ctx):
    n = _render(ctx, "cornell", team=1, brute_refill=4)
    assert n["brute"] & _native.BRUTE_REFILL and n["refill"] == 4 == _native.last_refill()[0]
    n = _render(ctx, "cornell", team=1, brute_refill=0)
    assert not n["brute"] & _native.BRUTE_REFILL and n["refill"] == 0


@pytest.mark.parametrize("cluster,loop", [(1, 3), (0, 1)])
def test_brute_cluster(ctx, cluster, loop):
    assert _render(ctx, "cornell", team=1, brute_cluster=cluster)["brute"] & 3 == loop


def test_ref_traversal(ctx):
    n = _render(ctx, "cornell", traversal=_native.RT_TRAVERSAL_REF)
    assert (n["trav"], n["brute"], n["resume"], n["smem"], n["ovf"]) == (REF, 0, 0, 0, 0)


def test_adds(ctx):
    cam, env, npix = _prepare(ctx, "cornell", {})
    ctx.accum_begin(cam, env, npix, MB)
    try:
        ctx.accum_add(SPP)
        n = _consistent(_native.last_launch())
        assert n["acc"] == 1 and n["brute"] and n["trav"] == FAST
        ctx.accum_select_mask(np.arange(npix) % 3 == 0)
        ctx.accum_add_selected(SPP)
        n = _consistent(_native.last_launch())
        assert n["acc"] == 2 and n["brute"] and not n["brute"] & _native.BRUTE_SLICED and n["slices"] == 0
        assert n["team"] == 1   # a listed add on auto: one lane per pixel
    finally:
        ctx.accum_end()


def test_count_work_runs_the_lock_step_loop(ctx):
    cam, env, npix = _prepare(ctx, "cornell", {"team": 1, "brute_cluster": 1})
    ctx.render(cam, env, npix, SPP, MB)
    assert _native.last_launch()["brute"] & 3 == 3
    c = ctx.count_work(cam, env, npix, SPP, MB)
    assert c["rays"] > 0
    n = _consistent(_native.last_launch())
    assert n["count"] == 1 and n["brute"] & 3 == 1 and not n["brute"] & _native.BRUTE_REFILL

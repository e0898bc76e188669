"""rt_set_option, key by key: the values each option accepts, the values next to them it refuses, and the status
and message of every refusal.  The table below was written from the branch chain rt_set_option was before it became
a table lookup (rt_api.hip options()) and passed on that build first: accepted values, status codes and message text
are part of the boundary.

The option checks need a context and no scene.  The last test sets a scene (Cornell, 8 x 8, 2 spp) to see that a
refused value leaves the one before it in force, one key of each effect class: none ("team"), one that invalidates
an open accumulation ("ref_stack"), one that repacks the scene ("brute_max")."""
import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W

pytestmark = pytest.mark.gpu

ARG = _native.RT_ERR_ARG
BIG = 1 << 32   # an int64 whose low word is 0: refused everywhere, never taken for 0

BOOL = ([0, 1], [-1, 2])
TRI = ([-1, 0, 1], [-2, 2])           # -1 (auto), 0, 1
TEAM = ([0, 1, 2, 4, 8], [-1, 3, 5, 6, 7, 9, 16])

# key: (default, accepted: smallest, largest and every member of a short set, refused: the nearest on each side, message)
OPTIONS = {
    "traversal": (0, *BOOL, "traversal must be 0 (fast) or 1 (ref)"),
    "brute_near": (-1, *TRI, "brute_near must be -1 (auto), 0 (off) or 1 (auto)"),
    "bvh": (1, *BOOL, "bvh must be 0 (reference tree) or 1 (sah)"),
    "brute_cluster": (-1, *TRI, "brute_cluster must be -1 (auto), 0 (off) or 1 (force)"),
    "brute_shell": (-1, *TRI, "brute_shell must be -1 (auto), 0 (off) or 1 (force)"),
    "brute_max": (64, [0, 4096], [-1, 4097], "brute_max must be in 0..4096"),
    "resume_min": (-1, [-1, 0, 64], [-2, 65], "resume_min must be -1 (auto) or 0..64"),
    "team": (0, *TEAM, "team must be 0 (auto), 1, 2, 4 or 8"),
    "walk_team": (0, *TEAM, "walk_team must be 0 (auto), 1, 2, 4 or 8"),
    "sun_any": (1, *BOOL, "sun_any must be 0 or 1"),
    "sun_skip": (1, *BOOL, "sun_skip must be 0 or 1"),
    "step": (0, [0, 1, 2], [-1, 3], "step must be 0 (auto), 1 (item) or 2 (round)"),
    "waves": (0, [0, 8], [-1, 9], "waves must be in 0..8"),
    "pilot": (-1, [-1, 0, 1 << 20], [-2, (1 << 20) + 1], "pilot must be -1 (auto), 0 (off) or a sample count"),
    "pilot_chunk": (0, [0, 4096], [-1, 4097], "pilot_chunk must be in 0..4096 (0 = auto)"),
    "pilot_levels": (0, [0, 2, 256], [-1, 1, 257], "pilot_levels must be 0 (auto) or 2..256"),
    "stack_lds": (0, [0, 8, 20], [-1, 1, 7, 21], "stack_lds must be 0 (auto) or 8..20"),
    "sun_cache": (1, *BOOL, "sun_cache must be 0 or 1"),
    "fixed_point": (1, *BOOL, "fixed_point must be 0 or 1"),
    "bvh_width": (0, [0, 2, 4], [-1, 1, 3, 5], "bvh_width must be 0 (auto), 2 or 4"),
    "ref_stack": (20, [20, 64], [19, 65, 0], "ref_stack must be in 20..64 (20 = the reference's)"),
    "slices": (-1, [-1, 0, 16], [-2, 17], "slices must be -1 (auto), 0 (off) or 1..16"),
    "brute_refill": (-1, [-1, 0, 64], [-2, 65], "brute_refill must be -1 (auto), 0 or 1 (off) or 2..64"),
    "denoise_lds": (-1, *TRI, "denoise_lds must be -1 (auto), 0 or 1"),
    "query_engine": (0, [0, 1, 2], [-1, 3], "query_engine must be 0 (auto), 1 (plain) or 2 (persistent)"),
    "query_grid": (0, [0, 1 << 20], [-1, (1 << 20) + 1], "query_grid must be 0 (auto) or a block count"),
    "wdq": (1, *BOOL, "wdq must be 0 or 1"),
    "handout": (-1, *TRI, "handout must be -1 (auto), 0 or 1"),
    "spec": (-1, [-1, 0, 2, 4, 8], [-2, 1, 3, 5, 6, 7, 9, 16], "spec must be -1 (auto), 0 (off), 2, 4 or 8"),
    "block": (128, [64, 128, 256], [0, 63, 65, 127, 129, 255, 257, 512], "block must be 64/128/256"),
}


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(device_ids=[0])   # no scene: a key that repacks stores its value and touches no device
    yield c
    c.close()


def _refused(ctx, key, value, message):
    with pytest.raises(_native.NativeError) as e:
        ctx.set_option(key, value)
    assert e.value.status == ARG, (key, value)
    assert str(e.value) == f"[rt status {ARG}] {message}", (key, value)


@pytest.mark.parametrize("key", list(OPTIONS))
def test_accepted_values_and_their_neighbours(ctx, key):
    default, accepted, refused, message = OPTIONS[key]
    try:
        for v in accepted:
            ctx.set_option(key, v)
        for v in refused + [BIG, -BIG, BIG + accepted[-1]]:
            _refused(ctx, key, v, message)
    finally:
        ctx.set_option(key, default)


def test_unknown_and_null_keys(ctx):
    for key in ("no_such_option", "", "Team", "team ", "brute"):
        _refused(ctx, key, 0, f"unknown option '{key}'")
    L = _native.lib()
    assert L.rt_set_option(ctx.handle, None, 0) == ARG
    assert L.rt_last_error(ctx.handle) == b"null argument"
    assert L.rt_set_option(None, b"team", 0) == ARG
    assert L.rt_last_error(None) == b"null argument"


def test_a_refused_value_leaves_the_one_before_it(ctx):
    """One context with Cornell at 8 x 8, 2 spp; what the launch got is read from rt_debug_last_launch."""
    sc, cam, env, npix, spp, mb, ibl = W.PARITY_CASES["cornell_64_s4"].with_size(8, 8, 2).inputs()
    c = _native.Context(device_ids=[0])
    try:
        c.set_env(ibl)
        c.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray)

        def launch():
            assert np.isfinite(c.render(cam, env, npix, spp, mb)).all()
            return _native.last_launch()

        # no effect beyond the store: the brute-force team size
        c.set_option("team", 4)
        _refused(c, "team", 3, OPTIONS["team"][3])
        assert launch()["team"] == 4
        c.set_option("team", 1)
        assert launch()["team"] == 1
        # repacks the scene: 0 takes the brute-force layout away, and the frame goes to the tree walk
        assert launch()["brute"] != 0
        c.set_option("brute_max", 0)
        _refused(c, "brute_max", 4097, OPTIONS["brute_max"][3])
        assert launch()["brute"] == 0
        # invalidates an accumulation: the REF walk's stack is ref_stack words per lane of dynamic LDS
        c.set_option("traversal", _native.RT_TRAVERSAL_REF)
        lds20 = launch()["lds"]
        c.set_option("ref_stack", 32)
        _refused(c, "ref_stack", 65, OPTIONS["ref_stack"][3])
        n = launch()
        assert n["trav"] == _native.RT_TRAVERSAL_REF and n["lds"] * 20 == lds20 * 32 and lds20 > 0
        # ... and a refused value invalidates nothing: the accumulation begun before it goes on
        c.accum_begin(cam, env, npix, mb)
        c.accum_add(1)
        _refused(c, "ref_stack", 19, OPTIONS["ref_stack"][3])
        c.accum_add(1)
        c.set_option("ref_stack", 20)
        with pytest.raises(_native.NativeError, match="invalidated") as e:
            c.accum_add(1)
        assert e.value.status == _native.RT_ERR_STATE
        c.accum_end()
    finally:
        c.close()

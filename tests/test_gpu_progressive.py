"""Progressive rendering (rt_accum_*, KernelLauncher.begin_progressive): adding samples to a frame gives,
bit for bit, the one-shot frame at the total -- so the oracle's -- on every engine and under every forced
schedule, on tiles and several device slots, and whatever else the context renders in between.

Every comparison is exact (np.testing.assert_array_equal): the feature has no tolerance.
"""
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "examples", "bin", "render_scene")


def _launcher(device=0, **kw):
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    return KernelLauncher(None, None, device, None, **kw)


@pytest.fixture(scope="module")
def kl():
    """The launcher of the one-shot references (never holds an accumulation)."""
    k = _launcher()
    yield k
    k.close()


@pytest.fixture()
def pl():
    """The launcher under test, fresh per test: options at their defaults, nothing open."""
    k = _launcher()
    yield k
    k.close()


def _inputs(case, spp=None):
    if case == "grid":   # the 4-wide walk's scene (C5) at a parity size
        wl = W.CONFIGS["C5"].with_size(48, 27, 16)
    elif case == "monkey_128":   # C3's scene and materials at 128 x 128
        wl = W.CONFIGS["C3"].with_size(128, 128, 16)
    elif case in W.CONFIGS:
        wl = W.CONFIGS[case]
    else:
        wl = W.PARITY_CASES[case]
    sc, cam, env, npix, s, mb, ibl = wl.inputs()
    return sc, cam, env, npix, (s if spp is None else spp), mb, ibl


_ONE_SHOT = {}


def _one_shot(kl, case, spp, npix=None):
    """launch_Raytracing of the case at spp with every option at its default (computed once, kept unchanged)."""
    key = (case, spp, npix)
    if key not in _ONE_SHOT:
        sc, cam, env, n, _, mb, ibl = _inputs(case)
        n = npix or n
        out = np.zeros(3 * n, np.float32)
        kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                             sc.BVH.exportArray, cam, env, n, spp, mb, ibl)
        out.setflags(write=False)
        _ONE_SHOT[key] = out
    return _ONE_SHOT[key]


def _begin(pl, case, npix=None):
    sc, cam, env, n, _, mb, ibl = _inputs(case)
    return pl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                sc.BVH.exportArray, cam, env, npix or n, mb, ibl)


def _oracle(case, spp):
    sc, cam, env, npix, _, mb, ibl = _inputs(case)
    return O.render(O.OracleScene.from_scene(sc, ibl), cam, env, npix, spp, mb, nthreads=16)


# ---- 1. split = one shot = oracle ----
SPLITS = {"s4": [(1, 1, 2), (3, 1)], "b0": [(1, 2)], "s16": [(1, 15), (5, 4, 7), (8, 8)]}
SPLIT_CASES = ["cornell_64_s4", "cornell_64_b0", "monkey_c3_64_s4", "serre_96x54_s4", "proto_64_s4", "furnace_64_s4",
               "cornell_128_s16"]


@pytest.mark.parametrize("case", SPLIT_CASES)
def test_split_equals_one_shot_equals_oracle(kl, pl, case):
    """FAST: the frame every add returns is launch_Raytracing at the running total, and .image() returns it
    again without rendering; the last is the oracle's frame at the total."""
    want = _oracle(case, _inputs(case)[4])
    for split in SPLITS[case.rsplit("_", 1)[1]]:
        p = _begin(pl, case)
        assert p.samples == 0
        total = 0
        for n in split:
            got = p.add(n)
            total += n
            np.testing.assert_array_equal(got, _one_shot(kl, case, total), err_msg=f"{split} at {total}")
            np.testing.assert_array_equal(p.image(), got, err_msg=f"image() {split} at {total}")
            assert p.samples == total
        np.testing.assert_array_equal(got, want, err_msg=f"{split} vs oracle")
        p.close()


@pytest.mark.parametrize("case", ["cornell_64_s4", "monkey_c3_64_s4", "serre_96x54_s4"])
def test_split_ref_traversal_equals_oracle(case):
    """REF (the reference's own DFS): the last add is the oracle's frame."""
    want = _oracle(case, 4)
    rl = _launcher(traversal="ref")
    try:
        for split in SPLITS["s4"]:
            p = _begin(rl, case)
            for n in split:
                got = p.add(n)
            np.testing.assert_array_equal(got, want, err_msg=str(split))
            np.testing.assert_array_equal(p.image(), want)
            assert p.samples == 4
    finally:
        rl.close()


# ---- 2. every engine and forced schedule ----
DEFAULTS = {"bvh_width": 0, "step": 0, "walk_team": 0, "pilot": -1, "slices": -1, "spec": -1, "stack_lds": 0,
            "brute_max": 64, "team": 0}
WALK = {"brute_max": 0}
TREE_SETTINGS = [
    {"bvh_width": 2}, {"bvh_width": 4},
    {"step": 1}, {"step": 2}, {"bvh_width": 4, "step": 2},
    {"bvh_width": 2, "walk_team": 2}, {"bvh_width": 2, "walk_team": 4},
    {"pilot": 2}, {"pilot": 5},
    {"pilot": 0, "slices": 2}, {"pilot": 0, "slices": 3}, {"pilot": 0, "slices": 8, "bvh_width": 2},
    {"pilot": 0, "slices": 5, "bvh_width": 4},
    {"bvh_width": 2, "pilot": 2, "spec": 2}, {"bvh_width": 2, "pilot": 2, "spec": 4},
    {"bvh_width": 2, "stack_lds": 8}, {"bvh_width": 4, "stack_lds": 8},
]
UNEVEN = [(5, 1, 10), (1, 6, 9), (7, 8, 1)]   # 16 samples, three uneven adds, one of a single sample


def _forced(pl, kl, case, settings, base):
    # (the grid's million triangles take seconds to pack and upload: its one-shot frame comes from the
    # launcher under test, options still at their defaults, so the scene is uploaded once)
    want = _one_shot(pl if case == "grid" else kl, case, 16)
    try:
        for k, forced in enumerate(settings):
            opts = dict(base, **forced)
            for key, v in opts.items():
                pl.native.set_option(key, v)
            split = UNEVEN[k % len(UNEVEN)]
            p = _begin(pl, case)
            for n in split:
                got = p.add(n)
            np.testing.assert_array_equal(got, want, err_msg=f"{forced} split {split}")
            for key in opts:
                pl.native.set_option(key, DEFAULTS[key])
    finally:
        for key, v in DEFAULTS.items():
            pl.native.set_option(key, v)


@pytest.mark.parametrize("case", ["monkey_c3_64_s4", "serre_96x54_s4", "grid"])
def test_forced_tree_walk_schedules(kl, pl, case):
    """The tree walk under each forced layout, traversal loop, team size, pilot, slice count, trail count
    and LDS stack size (the option names and the 16 spp of the one-shot tests of those schedules): the
    accumulated frame is the one-shot frame with every option at its default."""
    _forced(pl, kl, case, TREE_SETTINGS, WALK)


def test_forced_brute_force_schedules(kl, pl):
    _forced(pl, kl, "cornell_64_s4", [{"team": 2}, {"team": 8}, {"team": 1}, {"brute_max": 0}], {})


# ---- 3. engine-neutral state ----
@pytest.mark.parametrize("case,steps", [
    ("cornell_128_s16", [("brute_max", 0), ("bvh", _native.RT_BVH_REFERENCE)]),
    ("monkey_c3_64_s4", [("bvh_width", 2), ("bvh_width", 4), ("bvh_width", 2)]),
])
def test_state_is_engine_neutral(kl, pl, case, steps):
    """The engine changes between adds (brute force -> SAH tree walk -> reference tree; BVH2 <-> 4-wide):
    each continues the other's state, and the frame is the one-shot 16."""
    adds = [5, 4, 7] if len(steps) == 2 else [5, 4, 6, 1]
    try:
        p = _begin(pl, case)
        got = p.add(adds[0])
        for (key, v), n in zip(steps, adds[1:]):
            pl.native.set_option(key, v)
            got = p.add(n)
        assert p.samples == 16
        np.testing.assert_array_equal(got, _one_shot(kl, case, 16))
    finally:
        pl.native.set_option("brute_max", 64)
        pl.native.set_option("bvh", _native.RT_BVH_SAH)
        pl.native.set_option("bvh_width", 0)


# ---- 4. partial last row and tiles ----
def test_partial_last_row(kl, pl):
    npix = 64 * 63 + 17
    p = _begin(pl, "monkey_c3_64_s4", npix=npix)
    p.add(1)
    got = p.add(3)
    np.testing.assert_array_equal(got, _one_shot(kl, "monkey_c3_64_s4", 4, npix=npix))


@pytest.mark.parametrize("row0,row_step", [(3, 8), (1, 3)])
def test_device_form_tiles(pl, row0, row_step):
    """rt_accum_begin_device / rt_accum_add_device into a torch tensor: the tile after adds of 2 and 2 is
    rt_render_device's tile at 4."""
    import torch
    sc, cam, env, npix, _, mb, ibl = _inputs("monkey_c3_64_s4")
    ctx = pl.native
    ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray)
    ctx.set_env(ibl)
    w = int(cam[6])
    n = 3 * w * _native.tile_rows(npix, w, row0, row_step)
    want = torch.zeros(n, dtype=torch.float32, device="cuda")
    ctx.render_device(cam, env, npix, 4, mb, row0, row_step, want.data_ptr())
    got = torch.zeros(n, dtype=torch.float32, device="cuda")
    ctx.accum_begin_device(cam, env, npix, mb, row0, row_step)
    ctx.accum_add_device(2, got.data_ptr())
    assert ctx.accum_samples() == 2
    ctx.accum_add_device(2, got.data_ptr())
    torch.cuda.synchronize()
    assert ctx.accum_samples() == 4
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    ctx.accum_end()
    assert ctx.accum_samples() == -1


def test_host_form_over_three_slots_of_one_device(kl):
    """Context(device_ids=[0, 0, 0]): row r accumulates on slot r mod 3, each slot with a state of its own."""
    ml = _launcher(device=[0, 0, 0])
    try:
        p = _begin(ml, "serre_96x54_s4")
        first = p.add(1)
        np.testing.assert_array_equal(first, _one_shot(kl, "serre_96x54_s4", 1))
        got = p.add(3)
        np.testing.assert_array_equal(got, _one_shot(kl, "serre_96x54_s4", 4))
        np.testing.assert_array_equal(p.image(), got)
    finally:
        ml.close()


# ---- 5. isolation ----
def test_other_renders_between_adds_leave_the_state_alone(kl, pl):
    """Between two adds the same context renders a larger frame of the same scene from another camera (one
    pass with slices, then the automatic two-pass pilot: d.out, d.slice, d.pilot and d.spec grow) and
    counts work; the accumulation still ends at the one-shot frame, and was not invalidated."""
    case = "monkey_c3_64_s4"
    sc, cam, env, npix, _, mb, ibl = _inputs(case)
    p = _begin(pl, case)
    p.add(5)
    big = W.PARITY_CASES[case].with_size(160, 120)
    cam2 = sc.camera(big.width, big.height)
    cam2[0] += 0.05
    other = np.zeros(3 * big.npix, np.float32)
    try:
        for opts in ({"pilot": 0, "slices": 4}, {"pilot": -1, "slices": -1}):
            for key, v in opts.items():
                pl.native.set_option(key, v)
            pl.launch_Raytracing(other, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                                 sc.BVH.exportArray, cam2, env, big.npix, 16, mb, ibl)
    finally:
        pl.native.set_option("pilot", -1)
        pl.native.set_option("slices", -1)
    assert other.mean() > 0.0
    assert pl.native.count_work(cam2, env, big.npix, 2, mb)["rays"] > 0
    assert p.samples == 5
    got = p.add(11)
    np.testing.assert_array_equal(got, _one_shot(kl, case, 16))


# ---- 6. rgb8 ----
@pytest.mark.parametrize("gamma", [False, True])
def test_add_rgb8_is_the_quantised_frame(kl, pl, gamma):
    case = "serre_96x54_s4"
    sc, cam, env, npix, _, mb, ibl = _inputs(case)
    p = _begin(pl, case)
    a = p.add_rgb8(1, gamma=gamma)
    np.testing.assert_array_equal(a, kl.native.rgb8(_one_shot(kl, case, 1), gamma=gamma))
    b = p.add_rgb8(3, gamma)
    np.testing.assert_array_equal(b, pl.native.rgb8(p.image(), gamma=gamma))
    want8 = np.zeros(3 * npix, np.uint8)
    kl.launch_Raytracing_rgb8(want8, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                              sc.BVH.exportArray, cam, env, npix, 4, mb, ibl, gamma=gamma)
    np.testing.assert_array_equal(b, want8)
    assert b.dtype == np.uint8 and int(b.max()) > 0


# ---- 7. errors and invalidation ----
def _status(fn, *a, **kw):
    with pytest.raises(_native.NativeError) as ei:
        fn(*a, **kw)
    return ei.value.status


def test_errors_and_invalidation(kl, pl):
    case = "cornell_64_s4"
    sc, cam, env, npix, _, mb, ibl = _inputs(case)
    ctx = pl.native
    STATE, ARG = _native.RT_ERR_STATE, _native.RT_ERR_ARG
    # nothing open
    assert ctx.accum_samples() == -1
    assert _status(ctx.accum_add, 1) == STATE
    assert _status(ctx.accum_read) == STATE
    ctx.accum_end()   # no error
    # begin needs a scene and an environment, and checks its arguments as a render does
    assert _status(ctx.accum_begin, cam, env, npix, mb) == STATE
    p = _begin(pl, case)
    assert _status(ctx.accum_begin, cam, env, 0, mb) == ARG
    assert _status(ctx.accum_begin, cam, env, npix, 4097) == ARG
    p = _begin(pl, case)
    assert p.samples == 0
    assert _status(p.image) == STATE   # no samples yet
    assert _status(p.add, 0) == ARG
    assert _status(p.add, -1) == ARG
    p.add(1)
    assert _status(p.add, _native.RT_ACCUM_MAX_SAMPLES) == ARG   # 1 + the limit
    assert p.samples == 1
    with pytest.raises((TypeError, ValueError)):
        p.add(1, out=np.zeros(3 * npix, np.float64))
    with pytest.raises(ValueError):
        p.add(1, out=np.zeros(3 * npix - 1, np.float32))
    assert p.samples == 1
    # every other option keeps it valid
    ctx.set_option("bvh_width", 2)
    ctx.set_option("bvh_width", 0)
    np.testing.assert_array_equal(p.add(3), _one_shot(kl, case, 4))

    def invalidated(p):
        assert _status(p.add, 1) == STATE
        assert _status(p.image) == STATE
        assert _status(p.add_rgb8, 1) == STATE
        assert p.samples == 4   # still readable

    ctx.set_env(ibl)
    invalidated(p)
    p = _begin(pl, case)
    p.add(4)
    ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray)
    invalidated(p)
    try:
        p = _begin(pl, case)
        p.add(4)
        ctx.set_option("traversal", _native.RT_TRAVERSAL_REF)
        invalidated(p)
        ctx.set_option("traversal", _native.RT_TRAVERSAL_FAST)
        p = _begin(pl, case)
        p.add(4)
        ctx.set_option("ref_stack", 32)
        invalidated(p)
    finally:
        ctx.set_option("traversal", _native.RT_TRAVERSAL_FAST)
        ctx.set_option("ref_stack", 20)
    # a launch_Raytracing of another scene invalidates; one of the same scene (an upload-cache hit) does not
    p = _begin(pl, case)
    p.add(1)
    tmp = np.zeros(3 * npix, np.float32)
    pl.launch_Raytracing(tmp, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                         sc.BVH.exportArray, cam, env, npix, 2, mb, ibl)
    np.testing.assert_array_equal(p.add(3), _one_shot(kl, case, 4))
    s2, c2, e2, n2, _, m2, i2 = _inputs("monkey_c3_64_s4")
    pl.launch_Raytracing(tmp, s2.V_p, s2.V_n, s2.V_uv, s2.faceData, s2.materialData, s2.lightData,
                         s2.BVH.exportArray, c2, e2, n2, 1, m2, i2)
    assert _status(p.add, 1) == STATE


def test_second_begin_replaces_the_first(kl, pl):
    first = _begin(pl, "monkey_c3_64_s4")
    first.add(3)
    p = _begin(pl, "cornell_64_s4")
    assert p.samples == 0
    with pytest.raises(RuntimeError):
        first.add(1)   # the replaced object does not add to its successor
    np.testing.assert_array_equal(p.add(1), _one_shot(kl, "cornell_64_s4", 1))
    np.testing.assert_array_equal(p.add(3), _one_shot(kl, "cornell_64_s4", 4))
    p.close()
    assert pl.native.accum_samples() == -1


# ---- 8. one full-size frame ----
def test_full_size_c2_in_four_adds(kl, pl):
    want = _one_shot(kl, "C2", 64)
    p = _begin(pl, "C2")
    for n in (8, 8, 16, 32):
        got = p.add(n)
    assert p.samples == 64
    np.testing.assert_array_equal(got, want)


# ---- 9. an add costs its own samples ----
def test_an_add_costs_its_own_samples_not_the_frames(pl):
    """Monkey 128 x 128 with C3's materials: the 16 samples added after 16 and the 16 added after 496
    trace the same number of samples, so they take about the same time; an implementation that re-rendered
    the frame from sample 0 would take about 16 times as long for the second.  Minimum of 5 fresh
    repetitions each; the factor 3 allows for jitter on a shared machine."""
    def timed(first):
        best = float("inf")
        for _ in range(5):
            p = _begin(pl, "monkey_128")
            p.add(first)
            t0 = time.perf_counter()
            p.add(16)
            best = min(best, time.perf_counter() - t0)
            assert p.samples == first + 16
        return best

    t_a = timed(16)
    t_b = timed(496)
    print(f"add(16) after 16: {t_a * 1e3:.3f} ms; after 496: {t_b * 1e3:.3f} ms; ratio {t_b / t_a:.2f}")
    assert t_b <= 3 * t_a


# ---- 10. the C host ----
def test_c_host_progressive_option(tmp_path):
    """examples/render_scene with its ADDS argument: 3 adds, 1 add and the one-shot path write the same files."""
    from ensem3a_openclraytracer_amd.scene import Scene
    assert os.path.exists(BIN), "examples/bin/render_scene is built by __graft_entry__.build()"
    n, side, spp, mb = 24, 48, 8, 4
    text = W.grid_obj_text(n)
    sc = Scene.from_text(text, None, build_bvh=True, name=f"grid{n}")
    cam, env, ibl = sc.camera(side, side), sc.env(), W.ibl_preview()
    mat = np.ascontiguousarray(sc.materialData, np.float32).reshape(-1)
    h, w = ibl.shape[:2]
    params = (struct.pack("<i", mat.size // 6) + mat.tobytes() + np.asarray(cam, np.float32)[:10].tobytes()
              + np.asarray(env, np.float32)[:5].tobytes() + struct.pack("<iiiii", side * side, spp, mb, w, h)
              + np.ascontiguousarray(ibl, np.uint8).tobytes())
    (tmp_path / "grid.obj").write_text(text)
    (tmp_path / "params.bin").write_bytes(params)
    files = {}
    for adds in ("", "1", "3"):
        prefix = str(tmp_path / f"out{adds}")
        cmd = [BIN, str(tmp_path / "grid.obj"), str(tmp_path / "params.bin"), prefix] + ([adds] if adds else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("accumulated in" in r.stdout) == bool(adds)
        files[adds] = [open(prefix + sfx, "rb").read() for sfx in (".f32", ".rgb8", ".gamma.f32")]
    assert len(files["3"][0]) == 12 * side * side and any(files["3"][0])
    assert files["3"] == files["1"]
    assert files["3"] == files[""]
    bad = subprocess.run([BIN, str(tmp_path / "grid.obj"), str(tmp_path / "params.bin"), str(tmp_path / "x"), "9"],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "ADDS" in bad.stderr   # more adds than samples

"""Radiance queries on the GPU (rt_radiance / rt_radiance_device, rt_camera_rays*, KernelLauncher.radiance): the
frame's integrator on the caller's own rays.  The contract under test: a radiance query of a frame's camera rays with
that frame's seeds is that frame, bit for bit.

Scenes, cameras and helpers: tests/radiance_scenes.py (cornell: brute force; soup7: brute force; soup150: BVH2;
caterpillar: a 39-level tree).  Frames are 25 x 23 pixels (575 rays: a partial last wave, a partial block at every
block size), 5 spp, max_bounce in {-1, 0, 1, 4}, sun and IBL power each zero and non-zero.  Every comparison is exact:
equal bits, or NaN on both sides.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from oracle import compare
from tests import nonfinite_rays as NR
from tests import radiance_scenes as RS
from tests.radiance_scenes import NPIX, SPP

pytestmark = pytest.mark.gpu

FAST, REF = _native.RT_TRAVERSAL_FAST, _native.RT_TRAVERSAL_REF
DEFAULTS = {"bvh": _native.RT_BVH_SAH, "brute_max": 64, "block": 128, "radiance_grid": 0}
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def kl():
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    k = KernelLauncher(None, None, 0, None)
    k.upload_env(W.ibl_preview())
    yield k
    k.close()


class using:
    """The scene uploaded with its own options and the given ones, under a traversal, for the length of a with block."""

    def __init__(self, kl, name, traversal=FAST, **options):
        self.kl, self.sc = kl, RS.scene(name)
        self.options = {**self.sc.options, **options}
        self.traversal = traversal

    def __enter__(self):
        sc = self.sc
        self.kl.upload_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.bvh)
        self.kl.set_traversal("ref" if self.traversal == REF else "fast")
        for k, v in self.options.items():
            self.kl.native.set_option(k, v)
        return self.kl

    def __exit__(self, *exc):
        for k in self.options:
            self.kl.native.set_option(k, DEFAULTS[k])
        self.kl.set_traversal("fast")


@functools.lru_cache(maxsize=None)
def frame_rays(name):
    """The reference's camera rays of the scene's frame, [575, 8] with the seed words (i, 0)."""
    return RS.oracle_rays(RS.scene(name).cam, NPIX)


def query(kl, rays8, env, spp, max_bounce, state=None):
    seeds = rays8.view(np.uint32)[:, 6:8]
    return kl.radiance(rays8[:, 3:6], rays8[:, 0:3], spp, max_bounce, env, seeds=seeds, state=state)


def render(kl, sc, cam, env, npix, spp, max_bounce):
    out = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.bvh, cam, env,
                         npix, spp, max_bounce, W.ibl_preview())
    return out.reshape(-1, 3)


def settings():
    return [(mb, sun, ibl) for mb in RS.BOUNCES for sun, ibl in RS.POWERS]


# ---- 1. REF equals the oracle ----

@pytest.mark.parametrize("name", RS.SCENES)
def test_ref_query_of_the_camera_rays_is_the_oracles_frame(kl, name):
    sc = RS.scene(name)
    rays = frame_rays(name)
    with using(kl, name, REF):
        for mb, sun, ibl in settings():
            env = RS.env_with(sc, sun, ibl)
            want = RS.oracle_frame(name, sc.cam, env, NPIX, SPP, mb)
            got = query(kl, rays, env, SPP, mb)
            assert (got["n"] == SPP).all()
            bad = RS.differing(RS.clamp(got["rgb"]), want)
            assert not len(bad), (name, mb, sun, ibl, bad[:8], RS.clamp(got["rgb"])[bad[:3]], want[bad[:3]])


# ---- 2. FAST equals the frame ----

def fast_option_sets(name):
    sets = [dict(block=64), dict(block=128), dict(block=256), dict(radiance_grid=1), dict(radiance_grid=1, block=64)]
    if name == "cornell":
        sets.append(dict(brute_max=0))   # the tree walk in place of the brute force
    return sets


@pytest.mark.parametrize("name", RS.SCENES)
def test_fast_query_of_the_camera_rays_is_the_fast_frame(kl, name):
    sc = RS.scene(name)
    rays = frame_rays(name)
    frames = {}
    with using(kl, name, FAST):
        for mb, sun, ibl in settings():
            env = RS.env_with(sc, sun, ibl)
            frames[mb, sun, ibl] = render(kl, sc, sc.cam, env, NPIX, SPP, mb)
    # the FAST frame against the independent reference: the parity gate, as everywhere (caterpillar's 39-level
    # chain overflows the reference's 20-slot stack, which FAST does not copy: its reference is the oracle over the
    # same triangles in the shallow tree, as in tests/test_gpu_nonfinite.py)
    for (mb, sun, ibl), frame in frames.items():
        want = RS.oracle_frame(name, sc.cam, RS.env_with(sc, sun, ibl), NPIX, SPP, mb, shallow=name == "caterpillar")
        compare.assert_gate(frame.ravel(), want.ravel(), f"{name} mb {mb} sun {sun} ibl {ibl} FAST vs oracle")
    for options in fast_option_sets(name):
        with using(kl, name, FAST, **options):
            for (mb, sun, ibl), frame in frames.items():
                got = query(kl, rays, RS.env_with(sc, sun, ibl), SPP, mb)
                bad = RS.differing(RS.clamp(got["rgb"]), frame)
                assert not len(bad), (name, options, mb, sun, ibl, bad[:8])
    assert any((f != f[0]).any() for f in frames.values()), "every frame is one flat colour"


# ---- 3. rays of several cameras in one batch ----

def cameras(sc):
    """Six cameras around the scene's own: other positions, angles, fields of view, widths and pixel counts (two
    of them not a multiple of the width)."""
    rng = np.random.default_rng(2300)
    cams = []
    for width, npix, fov in ((25, 575, 25.0), (16, 16 * 9, 45.0), (7, 7 * 11 + 3, 75.0), (40, 40 * 5, 30.0),
                             (13, 13 * 13, 60.0), (31, 31 * 4 + 17, 90.0)):
        cam = np.array(sc.cam, np.float32)
        cam[0:3] += rng.uniform(-0.4, 0.4, 3).astype(np.float32)
        cam[3:6] += rng.uniform(-15.0, 15.0, 3).astype(np.float32)
        cam[6], cam[7] = width, (npix + width - 1) // width
        cam[9] = np.float32(fov * (3.14 / 180))
        cams.append((cam, npix))
    return cams


@pytest.mark.parametrize("name", ["cornell", "soup150"])
def test_each_ray_of_a_mixed_batch_is_its_own_frames_pixel(kl, name):
    sc = RS.scene(name)
    env, mb = RS.env_with(sc, 0.5, 0.3), 4
    with using(kl, name, FAST):
        frames, rays = [], []
        for cam, npix in cameras(sc):
            frames.append(render(kl, sc, cam, env, npix, SPP, mb)[:npix])
            o, d, seeds = kl.camera_rays(cam, npix)
            assert (seeds[:, 0] == np.arange(npix)).all() and (seeds[:, 1] == 0).all()
            rays.append((o, d, seeds))
        o, d, seeds = (np.concatenate([r[q] for r in rays]) for q in range(3))
        want = np.concatenate(frames)
        perm = np.random.default_rng(2301).permutation(len(o))
        got = kl.radiance(o[perm], d[perm], SPP, mb, env, seeds=seeds[perm])
        bad = RS.differing(RS.clamp(got["rgb"]), want[perm])
        assert not len(bad), (name, bad[:8], perm[bad[:8]])
        # and in another order, next to other neighbours, every ray's record is the same record
        perm2 = np.random.default_rng(2302).permutation(len(o))
        got2 = kl.radiance(o[perm2], d[perm2], SPP, mb, env, seeds=seeds[perm2])
        a, b = np.empty_like(got["state"]), np.empty_like(got2["state"])
        a[perm], b[perm2] = got["state"], got2["state"]
        assert a.tobytes() == b.tobytes()
        assert len({f.tobytes() for f in frames}) == len(frames)


# ---- 4. rt_camera_rays ----

def test_camera_rays_are_the_references_rays_and_seeds(kl):
    sc = RS.scene("cornell")
    for cam, npix in cameras(sc) + [(sc.cam, NPIX)]:
        want = RS.oracle_rays(cam, npix)
        got = kl.native.camera_rays(cam, npix)
        assert got.shape == (npix, 8)
        assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (cam.tolist(), npix)
        first, count = npix // 3, npix // 2
        sub = kl.native.camera_rays(cam, npix, first, count)
        assert sub.view(np.uint32).tobytes() == want[first:first + count].view(np.uint32).tobytes()
        assert kl.native.camera_rays(cam, npix, npix, 0).shape == (0, 8)
        o, d, seeds = kl.camera_rays(cam, npix)
        assert o.tobytes() == want[:, 3:6].tobytes() and d.tobytes() == want[:, 0:3].tobytes()
        assert seeds.dtype == np.uint32 and seeds.tobytes() == want.view(np.uint32)[:, 6:8].tobytes()


def test_camera_rays_device_form(kl):
    import torch
    sc = RS.scene("cornell")
    cam, npix = cameras(sc)[2]
    want = RS.oracle_rays(cam, npix)
    first, count = 5, npix - 9
    d_rays = torch.zeros((count, 8), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    kl.native.camera_rays_device(0, cam, npix, first, count, d_rays.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert d_rays.cpu().numpy().view(np.uint32).tobytes() == want[first:first + count].view(np.uint32).tobytes()


# ---- 5. resume ----

@pytest.mark.parametrize("traversal", ["fast", "ref"])
@pytest.mark.parametrize("name", RS.SCENES)
def test_two_then_three_samples_leave_the_record_of_five(kl, name, traversal):
    sc = RS.scene(name)
    rays = frame_rays(name)
    with using(kl, name, REF if traversal == "ref" else FAST):
        for mb, sun, ibl in ((4, 0.5, 0.3), (1, 0.0, 0.3), (0, 0.5, 0.0), (-1, 0.5, 0.3)):
            env = RS.env_with(sc, sun, ibl)
            one = query(kl, rays, env, 5, mb)
            two = query(kl, rays, env, 2, mb)
            assert (two["n"] == 2).all()
            first = two["state"].copy()
            both = query(kl, rays, env, 3, mb, state=two["state"])
            assert (both["n"] == 5).all()
            assert both["state"].tobytes() == one["state"].tobytes(), (name, traversal, mb, sun, ibl)
            assert RS.bits(both["rgb"]).tobytes() == RS.bits(one["rgb"]).tobytes()
            # a resumed call ignores the ray's seed words
            other = rays.copy()
            other.view(np.uint32)[:, 6:8] = 0xdeadbeef
            again = query(kl, other, env, 3, mb, state=first.copy())
            assert again["state"].tobytes() == one["state"].tobytes()
            if mb == 4:
                assert (one["state"]["seed0"] != rays.view(np.uint32)[:, 6]).any(), "no sample drew a random number"


@pytest.mark.parametrize("traversal", ["fast", "ref"])
@pytest.mark.parametrize("name", ["cornell", "soup150"])
def test_a_resumed_triangle_out_of_range_is_a_miss(kl, name, traversal):
    sc = RS.scene(name)
    rays = frame_rays(name)
    env, T = RS.env_with(sc, 0.5, 0.3), RS.ntri(sc)
    with using(kl, name, REF if traversal == "ref" else FAST):
        start = query(kl, rays, env, 2, 4)["state"]
        assert (start["tri"] >= 0).any()
        miss = start.copy()
        miss["tri"] = -1
        want = query(kl, rays, env, 3, 4, state=miss)["state"]
        for tri in (T, -7, INT_MAX, -INT_MAX - 1):
            poisoned = start.copy()
            poisoned["tri"] = tri
            got = query(kl, rays, env, 3, 4, state=poisoned)["state"]
            assert got.tobytes() == want.tobytes(), (name, traversal, tri)
        assert (want["tri"] == -1).all() and (want["n"] == 5).all()


# ---- 6. first hit ----

@pytest.mark.parametrize("traversal", ["fast", "ref"])
@pytest.mark.parametrize("name", RS.SCENES)
def test_first_hit_is_rt_traces_closest_hit(kl, name, traversal):
    """The frame's rays and the non-finite ray classes of tests/nonfinite_rays.py (no index is
    derived from a ray's floats unchecked, so NaN and infinite rays are safe); two runs give identical records."""
    sc = RS.scene(name)
    leaf = sc.bvh.reshape(-1, 9)
    leaf = leaf[leaf[:, 8] >= 0][:, 2:8]
    classes = NR.ray_classes(sc.cam[:3], leaf, seed=len(name), per_class=9)
    odd = np.concatenate(list(classes.values())).astype(np.float32)
    assert not np.isfinite(odd).all()
    rays6 = np.concatenate([frame_rays(name)[:, :6], odd])
    o, d = rays6[:, 3:6], rays6[:, 0:3]
    env = RS.env_with(sc, 0.5, 0.3)
    with using(kl, name, REF if traversal == "ref" else FAST):
        hits = kl.trace_rays(o, d)
        got = kl.radiance(o, d, 3, 4, env)
        again = kl.radiance(o, d, 3, 4, env)
    assert (got["tri"] == hits["tri"]).all(), np.nonzero(got["tri"] != hits["tri"])[0][:8]
    assert (RS.bits(got["k"]) == RS.bits(hits["k"])).all()
    assert (got["hit"] == hits["hit"]).all() and got["hit"].any() and not got["hit"].all()
    assert (RS.bits(got["k"][~got["hit"]]) == RS.bits(np.float32(1000.0))).all()
    assert got["state"].tobytes() == again["state"].tobytes()
    assert (got["state"]["seed0"][:NPIX] != np.arange(NPIX)).any()


# ---- 7. the device form ----

def test_device_form_on_a_torch_stream_gives_the_host_forms_bits(kl):
    import torch
    name = "soup150"
    sc = RS.scene(name)
    rays = frame_rays(name)
    env, mb = RS.env_with(sc, 0.5, 0.3), 4
    with using(kl, name, FAST):
        host = query(kl, rays, env, SPP, mb)
        # an open accumulation of the same frame brackets the launches: a query leaves it untouched and valid
        ctx = kl.native
        ctx.accum_begin(sc.cam, env, NPIX, mb)
        try:
            ctx.accum_add(2)
            before = ctx.accum_read().copy()
            o, d = torch.from_numpy(rays[:, 3:6].copy()).cuda(), torch.from_numpy(rays[:, 0:3].copy()).cuda()
            seeds = torch.from_numpy(rays.view(np.int32)[:, 6:8].copy()).cuda()
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                dev2 = kl.radiance(o, d, 2, mb, env, seeds=seeds)
                dev = kl.radiance(o, d, 3, mb, env, state=dev2["state"])
                one = kl.radiance(o, d, SPP, mb, env)   # default seeds: (ray index, 0), the frame's
            s.synchronize()
            assert ctx.accum_read().tobytes() == before.tobytes()
            after = ctx.accum_add(3).copy()
        finally:
            ctx.accum_end()
    for got in (dev, one):
        assert got["state"].is_cuda and got["state"].cpu().numpy().tobytes() == host["state"].tobytes()
        for key in ("rgb", "sum", "k"):
            assert RS.bits(got[key].cpu().numpy()).tobytes() == RS.bits(host[key]).tobytes(), key
        for key in ("n", "tri", "hit"):
            assert (got[key].cpu().numpy() == host[key]).all(), key
    # ... and went on to the frame of 5 samples, which is the query's
    assert not len(RS.differing(after.reshape(-1, 3)[:NPIX], RS.clamp(host["rgb"])))


# ---- 8. the error table ----

def test_error_statuses():
    import torch
    L = _native.lib()
    sc = RS.scene("cornell")
    rays = np.ascontiguousarray(frame_rays("cornell")[280:288])   # the frame's middle: rays that hit
    env = RS.env_with(sc, 0.5, 0.3)
    out = np.zeros(8, _native.RADIANCE_STATE_DTYPE)
    ctx = _native.Context(device_ids=[0])
    ARG, STATE = _native.RT_ERR_ARG, _native.RT_ERR_STATE
    p, q, e = ctypes.c_void_p(rays.ctypes.data), ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(env.ctypes.data)

    def host(rays=p, n=8, env=e, spp=2, mb=4, flags=0, state=q):
        return L.rt_radiance(ctx.handle, rays, n, env, spp, mb, flags, state)

    try:
        assert host() == STATE                                                     # no scene
        ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.bvh)
        assert host() == STATE                                                     # no environment
        assert b"rt_set_env" in L.rt_last_error(ctx.handle)
        ctx.set_env(W.ibl_preview())
        assert host() == 0 and (out["n"] == 2).all() and (out["tri"] >= 0).any()
        assert host(n=-1) == ARG and host(n=1 << 31) == ARG
        assert host(spp=0) == ARG and host(spp=-3) == ARG and host(spp=_native.RT_ACCUM_MAX_SAMPLES + 1) == ARG
        assert host(flags=2) == ARG and host(flags=-1) == ARG and host(flags=3) == ARG
        assert host(rays=None) == ARG and host(state=None) == ARG and host(env=None) == ARG
        assert host(rays=None, n=0, state=None) == 0                               # nothing to do
        assert host(mb=-5) == 0 and host(flags=_native.RT_RADIANCE_RESUME) == 0
        assert (out["n"] == 4).all()
        assert L.rt_radiance(None, p, 8, e, 2, 4, 0, q) == ARG
        d_rays = torch.from_numpy(np.concatenate([rays, rays])).cuda()
        d_state = torch.zeros((16, 8), dtype=torch.int32, device="cuda")
        rp, sp = d_rays.data_ptr(), d_state.data_ptr()

        def dev(slot, r, n, s, spp=2, flags=0):
            return L.rt_radiance_device(ctx.handle, slot, ctypes.c_void_p(r) if r else None, n, e, spp, 4, flags,
                                        ctypes.c_void_p(s) if s else None, None)

        assert dev(1, rp, 8, sp) == ARG and dev(-1, rp, 8, sp) == ARG              # one slot only
        assert dev(0, rp + 4, 8, sp) == ARG and dev(0, rp, 8, sp + 8) == ARG       # alignment
        assert dev(0, rp, 8, rp + 16) == ARG and dev(0, rp, 8, rp + 8 * 32 - 16) == ARG   # overlap
        assert dev(0, rp, 8, sp, spp=0) == ARG and dev(0, rp, 8, sp, flags=4) == ARG
        assert dev(0, None, 0, None) == 0
        assert dev(0, rp, 8, sp) == 0
        torch.cuda.synchronize()
        want = np.zeros(8, _native.RADIANCE_STATE_DTYPE)
        assert L.rt_radiance(ctx.handle, p, 8, e, 2, 4, 0, ctypes.c_void_p(want.ctypes.data)) == 0
        assert d_state[:8].cpu().numpy().tobytes() == want.tobytes()
        # rt_camera_rays: the camera and the pixel range
        cam = np.array(sc.cam, np.float32)
        buf = np.zeros((8, 8), np.float32)
        c, b = ctypes.c_void_p(cam.ctypes.data), ctypes.c_void_p(buf.ctypes.data)
        assert L.rt_camera_rays(ctx.handle, c, NPIX, 0, 8, b) == 0
        assert L.rt_camera_rays(ctx.handle, c, NPIX, NPIX - 7, 8, b) == ARG
        assert L.rt_camera_rays(ctx.handle, c, NPIX, -1, 8, b) == ARG
        assert L.rt_camera_rays(ctx.handle, c, NPIX, 0, -1, b) == ARG
        assert L.rt_camera_rays(ctx.handle, c, 0, 0, 0, b) == ARG
        assert L.rt_camera_rays(ctx.handle, None, NPIX, 0, 8, b) == ARG
        assert L.rt_camera_rays(ctx.handle, c, NPIX, 0, 8, None) == ARG
        assert L.rt_camera_rays(ctx.handle, c, NPIX, 3, 0, None) == 0
        assert L.rt_camera_rays_device(ctx.handle, 1, c, NPIX, 0, 8, ctypes.c_void_p(rp), None) == ARG
        assert L.rt_camera_rays_device(ctx.handle, 0, c, NPIX, 0, 8, ctypes.c_void_p(rp + 4), None) == ARG
        zero_width = cam.copy()
        zero_width[6] = 0
        assert L.rt_camera_rays(ctx.handle, ctypes.c_void_p(zero_width.ctypes.data), NPIX, 0, 8, b) == ARG
        # a scene without the FAST layouts (a node reachable twice): FAST is a state error, REF runs
        bad = np.array(sc.bvh, np.float32).reshape(-1, 9).copy()
        bad[int(bad[0, 1]), 0] = bad[int(bad[0, 0]), 0]
        ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, bad.ravel())
        assert not ctx.scene_info()["fast_ok"]
        assert host() == STATE
        ctx.set_option("traversal", REF)
        assert host() == 0
    finally:
        ctx.close()


def test_radiance_grid_option():
    ctx = _native.Context(device_ids=[0])
    try:
        for v in (0, 1, 1 << 20):
            ctx.set_option("radiance_grid", v)
        for v in (-1, (1 << 20) + 1):
            with pytest.raises(_native.NativeError) as e:
                ctx.set_option("radiance_grid", v)
            assert e.value.status == _native.RT_ERR_ARG
            assert str(e.value).endswith("radiance_grid must be 0 (auto) or a block count")
    finally:
        ctx.close()

"""Lens frames on the GPU (rt_lens_radiance*, rt_lens_rays*, rt_radiance_resolve_device, KernelLauncher.lens_frame
and lens_rays): a camera ray per sample, generated on the device.  Under test, DESIGN.md 2.4's contracts:

  A  a pixel's record is that of one fresh radiance query per sample, of the ray lens_ray(i, s) at spp = 1, each
     starting from the seeds the one before left, the sums added in order;
  B  the degenerate lens (jitter 0, aperture 0) gives rt_radiance's records of the camera rays, and rt_render's frame;
  C  a then b samples with the state passed back leave the records of a + b;
  D  nothing depends on the form (host / device), the block, the grid, the engine or the split over device slots;

the rays themselves against the float64 restatement of tests/lens_ref.py, and rt_radiance_resolve_device.

Scenes, cameras and helpers: tests/radiance_scenes.py.  Frames are 25 x 23 pixels (575: a partial last wave, a partial
block at every block size).  Records are compared word for word: equal bits, or NaN on both sides.
"""
import ctypes

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests import lens_ref as LR
from tests import radiance_scenes as RS
from tests.radiance_scenes import NPIX, SPP
from tests.test_gpu_radiance import FAST, REF, render, using

pytestmark = pytest.mark.gpu

SEED = 23
NS = 16                                   # samples per pixel of the ray tests
S = 4                                     # samples of contract A
PINHOLE, LENS, WIDE, DEGENERATE = (1.0, 0.0, 1.0), (1.0, 0.05, 3.5), (2.0, 0.3, 0.5), (0.0, 0.0, 1.0)
CAMERAS = ("cornell", "soup7", "soup150")   # no angles at 45 degrees; no angles at 100; angles (16, 12, 0) at 25
# The float32 numpy evaluation of lens_ray deviates from the float64 one by at most 2.4e-7 on these cameras; the gate
# is that with a factor of 8, for rtm's few-ulp sincos and the quaternion form of the rotations.
RAY_TOL = 2e-6


@pytest.fixture(scope="module")
def kl():
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    k = KernelLauncher(None, None, 0, None)
    k.upload_env(W.ibl_preview())
    yield k
    k.close()


def lens_rays(kl, cam, lens, **kw):
    return kl.lens_rays(cam, NPIX, lens[0], lens[1], lens[2], SEED, **kw)


def lens_frame(kl, cam, env, spp, mb, lens, **kw):
    return kl.lens_frame(cam, env, NPIX, spp, mb, jitter=lens[0], aperture=lens[1], focus=lens[2], seed=SEED, **kw)


def record_words(st):
    """A RADIANCE_STATE_DTYPE array as float32 [n, 4] (sum, k) and uint32 [n, 4] (seed0, seed1, tri, n)."""
    raw = np.ascontiguousarray(st).view(np.uint32).reshape(len(st), 8)
    return raw[:, 0:4].view(np.float32), raw[:, 4:8]


def differing_records(a, b):
    """Records whose eight words are not the same bits (a NaN float equal to any NaN)."""
    fa, ia = record_words(a)
    fb, ib = record_words(b)
    return np.union1d(RS.differing(fa, fb), np.nonzero((ia != ib).any(1))[0])


def chained(kl, cam, lens, env, mb, nsamples, first=0, count=None):
    """Contract A's construction: one fresh radiance query at spp = 1 per sample, of the listed ray lens_ray(i, s),
    with the seeds the query before left; the sums added in order in fp32."""
    rays = lens_rays(kl, cam, lens, first=first, count=count, nsamples=nsamples)
    seeds = rays.view(np.uint32)[:, 0, 6:8].copy()
    total = np.zeros((len(rays), 3), np.float32)
    st = None
    for s in range(nsamples):
        st = kl.radiance(rays[:, s, 3:6], rays[:, s, 0:3], 1, mb, env, seeds=seeds)["state"]
        assert (st["n"] == 1).all()
        with np.errstate(all="ignore"):
            total = total + st["sum"]
        seeds = np.stack([st["seed0"], st["seed1"]], 1)
    want = st.copy()
    want["sum"] = total
    want["n"] = nsamples
    return want


# ---- 1. the rays against the restatement ----

@pytest.mark.parametrize("lens", [PINHOLE, LENS, WIDE, DEGENERATE])
@pytest.mark.parametrize("name", CAMERAS)
def test_rays_are_the_restatements_rays(kl, name, lens):
    cam = RS.scene(name).cam
    rays = lens_rays(kl, cam, lens, nsamples=NS)
    assert rays.shape == (NPIX, NS, 8) and rays.dtype == np.float32
    i, s = np.arange(NPIX)[:, None], np.arange(NS)[None, :]
    o, d = LR.lens_ray(cam, lens[0], lens[1], lens[2], SEED, i, s)
    dev_d = np.abs(rays[:, :, 0:3] - d).max()
    dev_o = np.abs(rays[:, :, 3:6] - o).max()
    print(f"lens rays {name} {lens}: max |direction - float64| {dev_d:.3e}, max |origin - float64| {dev_o:.3e}")
    assert dev_d <= RAY_TOL
    assert dev_o <= RAY_TOL * max(1.0, float(np.abs(cam[:3]).max()) + lens[1])
    # the seed words: the pixel's frame seeds, the same for each of its samples
    words = rays.view(np.uint32)
    assert (words[:, :, 6] == i).all() and (words[:, :, 7] == 0).all()
    # a window of samples and a slice of pixels are the same rays
    part = lens_rays(kl, cam, lens, first=37, count=301, sample0=5, nsamples=3)
    assert part.shape == (301, 3, 8) and part.tobytes() == np.ascontiguousarray(rays[37:338, 5:8]).tobytes()


def test_jitter_offsets_are_the_exact_uniforms(kl):
    """The uniforms through the rays, with no debug entry: a pinhole without angles has d ~ (pc.x, fd, pc.z), so
    u0 = (d.x / d.y * fd + 0.5) * W - pixelY + 0.5 (and u1 from d.z, pixelX).  A direction within RAY_TOL puts the
    recovered value within RAY_TOL * (1 + |d.x / d.y|) / d.y * fd * W of the restatement's exact u -- 2e-4 here, a
    ten-thousandth of the uniforms' range, where a wrong hash, counter or word order is off by a third on average."""
    cam = RS.scene("cornell").cam
    assert (cam[3:6] == 0).all()
    rays = lens_rays(kl, cam, PINHOLE, nsamples=NS).astype(np.float64)
    i, s = np.arange(NPIX)[:, None], np.arange(NS)[None, :]
    u = LR.uniforms(SEED, i, s).astype(np.float64)
    fd, width = LR.focal_distance(cam), float(cam[6])
    pixelY = (i + 1) % int(width)
    q = i - pixelY
    pixelX = np.sign(q) * (np.abs(q) // int(width))
    d = rays[:, :, 0:3]
    u0 = (d[..., 0] / d[..., 1] * fd + 0.5) * width - pixelY + 0.5
    u1 = -(d[..., 2] / d[..., 1] * fd - 0.5) * width - pixelX + 0.5
    for got, want, num in ((u0, u[..., 0], d[..., 0]), (u1, u[..., 1], d[..., 2])):
        tol = RAY_TOL * (1 + np.abs(num / d[..., 1])) / d[..., 1] * fd * width
        assert tol.max() < 2e-4
        assert (np.abs(got - want) <= tol).all(), np.abs(got - want).max()
    # another seed, other rays; the same seed, the same rays
    other = kl.lens_rays(cam, NPIX, 1.0, 0.0, 1.0, SEED + 1, nsamples=2)
    assert (other[:, :, 0:3] != rays[:, :2, 0:3].astype(np.float32)).any(-1).all()
    again = kl.lens_rays(cam, NPIX, 1.0, 0.0, 1.0, SEED, nsamples=2)
    assert again.tobytes() == rays[:, :2].astype(np.float32).tobytes()


# ---- 2. properties of the listed rays, in float64 ----

@pytest.mark.parametrize("name", CAMERAS)
def test_ray_properties(kl, name):
    cam = RS.scene(name).cam
    position = cam[:3].astype(np.float64)
    i = np.arange(NPIX)
    # jitter 0: the 16 rays of a pixel meet in one point of the plane in focus.  The point is o + d * tau with
    # tau ~ focus / d.y ~ focus; a direction error of 2e-6 times tau leaves 1e-5 * focus about 5 times the margin.
    for lens in ((0.0, LENS[1], LENS[2]), (0.0, WIDE[1], WIDE[2])):
        rays = lens_rays(kl, cam, lens, nsamples=NS).astype(np.float64)
        o, d = rays[:, :, 3:6], rays[:, :, 0:3]
        point, axis = LR.focus_point(cam, lens[2], i)
        tau = (lens[2] - (o - position) @ axis) / (d @ axis)
        off = np.linalg.norm(o + d * tau[..., None] - point[:, None, :], axis=-1)
        print(f"lens rays {name} {lens}: max distance from the point in focus {off.max():.3e} (focus {lens[2]})")
        assert off.max() <= 1e-5 * lens[2]
        assert (np.linalg.norm(o - position, axis=-1).max(1) > 0.5 * lens[1]).all()   # ... through a real aperture
        assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() <= 1e-6
    # aperture 0: every origin is the camera's position, in bits
    for lens in (PINHOLE, DEGENERATE, (2.0, 0.0, 0.5)):
        rays = lens_rays(kl, cam, lens, nsamples=NS)
        assert rays[:, :, 3:6].tobytes() == np.broadcast_to(cam[:3], (NPIX, NS, 3)).tobytes()
        assert np.abs(np.linalg.norm(rays[:, :, 0:3].astype(np.float64), axis=-1) - 1).max() <= 1e-6
    # jitter 0 and aperture 0: rt_camera_rays' rays, for every s
    want = kl.native.camera_rays(cam, NPIX)
    got = lens_rays(kl, cam, DEGENERATE, nsamples=NS)
    assert got.tobytes() == np.repeat(want[:, None, :], NS, 1).tobytes()


# ---- 3. contract A ----

@pytest.mark.parametrize("traversal", ["fast", "ref"])
@pytest.mark.parametrize("name", RS.SCENES)
def test_a_record_is_the_chain_of_single_sample_queries(kl, name, traversal):
    sc = RS.scene(name)
    frames = {}
    with using(kl, name, REF if traversal == "ref" else FAST):
        for mb in (0, 4):
            for sun, ibl in ((0.5, 0.3), (0.0, 0.0)):
                env = RS.env_with(sc, sun, ibl)
                for lens in (PINHOLE, LENS):
                    got = lens_frame(kl, sc.cam, env, S, mb, lens)
                    want = chained(kl, sc.cam, lens, env, mb, S)
                    bad = differing_records(got["state"], want)
                    assert not len(bad), (name, traversal, mb, sun, ibl, lens, bad[:8], got["state"][bad[:2]], want[bad[:2]])
                    assert (got["n"] == S).all()
                    frames[mb, sun, lens] = got["rgb"]
        if name == "cornell":   # a generator that ignored the lens would pass the above with the pinhole's rays
            env = RS.env_with(sc, 0.5, 0.3)
            flat = lens_frame(kl, sc.cam, env, S, 4, DEGENERATE)["rgb"]
            assert len(RS.differing(frames[4, 0.5, PINHOLE], flat))
            assert len(RS.differing(frames[4, 0.5, PINHOLE], frames[4, 0.5, LENS]))


# ---- 4. contract B ----

@pytest.mark.parametrize("traversal", ["fast", "ref"])
@pytest.mark.parametrize("name", RS.SCENES)
def test_b_degenerate_lens_is_the_query_of_the_camera_rays_and_the_frame(kl, name, traversal):
    sc = RS.scene(name)
    with using(kl, name, REF if traversal == "ref" else FAST):
        o, d, seeds = kl.camera_rays(sc.cam, NPIX)
        for mb in RS.BOUNCES:
            for sun, ibl in RS.POWERS:
                env = RS.env_with(sc, sun, ibl)
                got = lens_frame(kl, sc.cam, env, SPP, mb, DEGENERATE)
                want = kl.radiance(o, d, SPP, mb, env, seeds=seeds)["state"]
                assert got["state"].tobytes() == want.tobytes(), (name, traversal, mb, sun, ibl)
                frame = render(kl, sc, sc.cam, env, NPIX, SPP, mb)[:NPIX]
                bad = RS.differing(got["rgb"], frame)
                assert not len(bad), (name, traversal, mb, sun, ibl, bad[:8])


# ---- 5. contract C ----

@pytest.mark.parametrize("traversal", ["fast", "ref"])
@pytest.mark.parametrize("name", ["cornell", "soup150"])
def test_c_two_then_three_samples_leave_the_record_of_five(kl, name, traversal):
    import torch
    sc = RS.scene(name)
    with using(kl, name, REF if traversal == "ref" else FAST):
        for mb, sun, ibl, lens in ((4, 0.5, 0.3, LENS), (1, 0.0, 0.3, PINHOLE), (-1, 0.5, 0.3, LENS)):
            env = RS.env_with(sc, sun, ibl)
            one = lens_frame(kl, sc.cam, env, 5, mb, lens)
            two = lens_frame(kl, sc.cam, env, 2, mb, lens)
            assert (two["n"] == 2).all()
            # the record's tri and k are never read: any bits there change nothing
            start = two["state"].copy()
            start["tri"] = 2 ** 31 - 1
            start["k"] = np.float32("nan")
            both = lens_frame(kl, sc.cam, env, 3, mb, lens, state=start)
            assert (both["n"] == 5).all()
            assert both["state"].tobytes() == one["state"].tobytes(), (name, traversal, mb, sun, ibl, lens)
            assert RS.bits(both["rgb"]).tobytes() == RS.bits(one["rgb"]).tobytes()
            # the device form, on a stream of torch's, from the records a frame starts from
            state = kl.lens_state(NPIX)
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                dev2 = lens_frame(kl, sc.cam, env, 2, mb, lens, state=state)
                n2 = dev2["n"].clone()
                dev = lens_frame(kl, sc.cam, env, 3, mb, lens, state=dev2["state"])
            stream.synchronize()
            assert dev["state"] is state and state.is_cuda and (n2.cpu().numpy() == 2).all()
            assert state.cpu().numpy().tobytes() == one["state"].tobytes(), (name, traversal, mb, sun, ibl, lens)
            assert RS.bits(dev["rgb"].cpu().numpy()).tobytes() == RS.bits(one["rgb"]).tobytes()
            if mb == 4:
                assert (one["state"]["seed0"] != np.arange(NPIX)).any(), "no sample drew a random number"


# ---- 6. contract D ----

def option_sets(name):
    sets = [dict(block=64), dict(block=256), dict(radiance_grid=1), dict(radiance_grid=1, block=64)]
    if name == "cornell":
        sets.append(dict(brute_max=0))   # the tree walk in place of the brute force
    return sets


@pytest.mark.parametrize("name", RS.SCENES)
def test_d_nothing_depends_on_the_launch(kl, name):
    import torch
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    sc = RS.scene(name)
    env, mb = RS.env_with(sc, 0.5, 0.3), 4
    lenses = (LENS, PINHOLE, DEGENERATE)
    with using(kl, name, FAST):   # (block 128, the default)
        want = {lens: lens_frame(kl, sc.cam, env, S, mb, lens)["state"] for lens in lenses}
        # a slice of the pixels is that slice of the frame
        for lens in lenses:
            part = lens_frame(kl, sc.cam, env, S, mb, lens, first=37, count=301)["state"]
            assert part.tobytes() == want[lens][37:338].tobytes(), (name, lens)
        # the device form of a fresh call
        state = torch.zeros((NPIX, 8), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        kl.native.lens_radiance_device(0, sc.cam, env, _native.Lens(*LENS, SEED), NPIX, 0, NPIX, S, mb, 0,
                                       state.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert state.cpu().numpy().tobytes() == want[LENS].tobytes()
    for options in option_sets(name):
        with using(kl, name, FAST, **options):
            for lens in lenses:
                got = lens_frame(kl, sc.cam, env, S, mb, lens)["state"]
                assert got.tobytes() == want[lens].tobytes(), (name, options, lens)
    # two slots on one device: the pixels split in two chunks
    two = KernelLauncher(None, None, [0, 0], None)
    try:
        two.upload_env(W.ibl_preview())
        with using(two, name, FAST):
            for lens in lenses:
                got = lens_frame(two, sc.cam, env, S, mb, lens)["state"]
                assert got.tobytes() == want[lens].tobytes(), (name, "two slots", lens)
                part = lens_frame(two, sc.cam, env, S, mb, lens, first=37, count=301)["state"]
                assert part.tobytes() == want[lens][37:338].tobytes()
    finally:
        two.close()


# ---- 7. resolve ----

def test_resolve_is_the_clamped_mean(kl):
    import torch
    sc = RS.scene("cornell")
    env = RS.env_with(sc, 0.5, 0.3)
    with using(kl, "cornell", FAST):
        st = lens_frame(kl, sc.cam, env, S, 4, LENS)["state"].copy()
    st["n"][11] = 0                          # 0 / 0 and x / 0: NaN and infinity, which the clamp sends to 1
    st["sum"][12] = 0
    st["n"][12] = 0
    st["sum"][13] = (-0.25, 2.0, -3.0)       # a negative sum clamps to 0
    st["sum"][14] = (np.float32("nan"), np.float32("inf"), -np.float32("inf"))
    st["n"][15] = 3
    with np.errstate(all="ignore"):
        want = RS.clamp(st["sum"] / st["n"].astype(np.float32)[:, None])
    assert want[12].tolist() == [1, 1, 1] and want[13].tolist() == [0, 0.5, 0] and want[14].tolist() == [1, 1, 0]
    d_state = torch.from_numpy(st.view(np.int32).reshape(-1, 8).copy()).cuda()
    d_rgb = torch.full((NPIX + 1, 3), -7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    kl.native.radiance_resolve_device(0, d_state.data_ptr(), NPIX, d_rgb.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    got = d_rgb.cpu().numpy()
    assert RS.bits(got[:NPIX]).tobytes() == RS.bits(want).tobytes()
    assert (got[NPIX] == -7.0).all()         # nothing past the last record
    assert len(np.unique(want)) > 100


# ---- 8. a camera that makes non-finite rays ----

@pytest.mark.parametrize("name", ["cornell", "soup150"])
def test_non_finite_camera_is_safe(kl, name):
    sc = RS.scene(name)
    cam = np.array(sc.cam, np.float32)
    cam[9] = 0.0                             # tan(0) = 0: the focal point is infinitely far behind the camera
    env = RS.env_with(sc, 0.5, 0.3)
    with using(kl, name, FAST):
        for lens in (PINHOLE, LENS):
            rays = lens_rays(kl, cam, lens, nsamples=S)
            assert not np.isfinite(rays[:, :, 0:3]).all()
            got = lens_frame(kl, cam, env, S, 4, lens)
            want = chained(kl, cam, lens, env, 4, S)
            bad = differing_records(got["state"], want)
            assert not len(bad), (name, lens, bad[:8], got["state"][bad[:2]], want[bad[:2]])
            assert (got["n"] == S).all() and ((got["rgb"] >= 0) & (got["rgb"] <= 1)).all()


# ---- 9. the error table ----

def test_error_statuses():
    import torch
    L = _native.lib()
    sc = RS.scene("cornell")
    cam, env = np.array(sc.cam, np.float32), RS.env_with(sc, 0.5, 0.3)
    out = np.zeros(8, _native.RADIANCE_STATE_DTYPE)
    rays = np.zeros((8, 2, 8), np.float32)
    ctx = _native.Context(device_ids=[0])
    ARG, STATE = _native.RT_ERR_ARG, _native.RT_ERR_STATE
    c, e = ctypes.c_void_p(cam.ctypes.data), ctypes.c_void_p(env.ctypes.data)
    q, r = ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(rays.ctypes.data)
    good = _native.Lens(1.0, 0.05, 3.5, SEED)

    def host(cam=c, env=e, lens=good, npix=NPIX, first=280, count=8, spp=2, mb=4, flags=0, state=q):
        return L.rt_lens_radiance(ctx.handle, cam, env, ctypes.byref(lens) if lens else None, npix, first, count, spp,
                                  mb, flags, state)

    def listed(cam=c, lens=good, npix=NPIX, first=280, count=8, sample0=0, nsamples=2, rays=r):
        return L.rt_lens_rays(ctx.handle, cam, ctypes.byref(lens) if lens else None, npix, first, count, sample0,
                              nsamples, rays)

    inf, nan = float("inf"), float("nan")
    bad_lenses = [_native.Lens(-1.0, 0.0, 1.0), _native.Lens(nan, 0.0, 1.0), _native.Lens(inf, 0.0, 1.0),
                  _native.Lens(1.0, -0.1, 1.0), _native.Lens(1.0, nan, 1.0), _native.Lens(1.0, inf, 1.0),
                  _native.Lens(1.0, 0.0, 0.0), _native.Lens(1.0, 0.0, -2.0), _native.Lens(1.0, 0.0, nan),
                  _native.Lens(1.0, 0.0, inf)]
    try:
        assert listed() == 0 and np.isfinite(rays).all() and (rays[:, :, 0:3] != 0).any()   # needs no scene
        assert host() == STATE                                                              # no scene
        ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.bvh)
        assert host() == STATE                                                              # no environment
        assert b"rt_set_env" in L.rt_last_error(ctx.handle)
        ctx.set_env(W.ibl_preview())
        assert host() == 0 and (out["n"] == 2).all() and (out["tri"] >= 0).any()
        for lens in bad_lenses:
            assert host(lens=lens) == ARG and listed(lens=lens) == ARG, (lens.jitter, lens.aperture, lens.focus)
        assert host(lens=None) == ARG and listed(lens=None) == ARG
        assert host(cam=None) == ARG and host(env=None) == ARG and host(state=None) == ARG
        assert host(spp=0) == ARG and host(spp=_native.RT_ACCUM_MAX_SAMPLES + 1) == ARG
        assert host(flags=2) == ARG and host(flags=-1) == ARG and host(mb=4097) == ARG
        assert host(first=NPIX - 7) == ARG and host(first=-1) == ARG and host(count=-1) == ARG and host(npix=0) == ARG
        assert host(count=0, state=None) == 0                                               # nothing to do
        assert host(mb=-5) == 0 and host(flags=_native.RT_RADIANCE_RESUME) == 0 and (out["n"] == 4).all()
        assert L.rt_lens_radiance(None, c, e, ctypes.byref(good), NPIX, 0, 8, 2, 4, 0, q) == ARG
        assert listed(sample0=-1) == ARG and listed(nsamples=0) == ARG and listed(nsamples=-3) == ARG
        assert listed(first=NPIX - 7) == ARG and listed(rays=None) == ARG and listed(cam=None) == ARG
        assert listed(count=0, rays=None) == 0 and listed(sample0=2 ** 31 - 2) == 0
        zero_width = cam.copy()
        zero_width[6] = 0
        assert host(cam=ctypes.c_void_p(zero_width.ctypes.data)) == ARG
        # the device forms: the slot and the alignment
        d_state = torch.zeros((9, 8), dtype=torch.int32, device="cuda")
        d_rgb = torch.zeros((9, 3), dtype=torch.float32, device="cuda")
        sp, gp = d_state.data_ptr(), d_rgb.data_ptr()

        def dev(slot, s, count=8):
            return L.rt_lens_radiance_device(ctx.handle, slot, c, e, ctypes.byref(good), NPIX, 280, count, 2, 4, 0,
                                             ctypes.c_void_p(s) if s else None, None)

        def resolve(slot, s, n, g):
            return L.rt_radiance_resolve_device(ctx.handle, slot, ctypes.c_void_p(s) if s else None, n,
                                                ctypes.c_void_p(g) if g else None, None)

        assert dev(1, sp) == ARG and dev(-1, sp) == ARG and dev(0, sp + 8) == ARG and dev(0, None) == ARG
        assert dev(0, None, count=0) == 0 and dev(0, sp) == 0
        assert L.rt_lens_rays_device(ctx.handle, 0, c, ctypes.byref(good), NPIX, 0, 4, 0, 2, ctypes.c_void_p(sp + 4),
                                     None) == ARG
        assert L.rt_lens_rays_device(ctx.handle, 1, c, ctypes.byref(good), NPIX, 0, 4, 0, 2, ctypes.c_void_p(sp),
                                     None) == ARG
        assert resolve(1, sp, 8, gp) == ARG and resolve(0, sp + 8, 8, gp) == ARG and resolve(0, sp, 8, gp + 2) == ARG
        assert resolve(0, sp, -1, gp) == ARG and resolve(0, None, 8, gp) == ARG and resolve(0, sp, 8, None) == ARG
        assert resolve(0, sp, 8, sp + 32) == ARG                                            # overlap
        assert resolve(0, None, 0, None) == 0 and resolve(0, sp, 8, gp) == 0
        torch.cuda.synchronize()
        want = np.zeros(8, _native.RADIANCE_STATE_DTYPE)
        assert L.rt_lens_radiance(ctx.handle, c, e, ctypes.byref(good), NPIX, 280, 8, 2, 4, 0,
                                  ctypes.c_void_p(want.ctypes.data)) == 0
        assert d_state[:8].cpu().numpy().tobytes() == want.tobytes()
        with np.errstate(all="ignore"):
            assert RS.bits(d_rgb[:8].cpu().numpy()).tobytes() == RS.bits(RS.clamp(want["sum"] / np.float32(2))).tobytes()
    finally:
        ctx.close()

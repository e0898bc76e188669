"""Ray queries on the GPU (rt_trace / rt_trace_device, KernelLauncher.trace_rays): closest-hit and any-hit batches
of the caller's own rays give the frame's hits, bit for bit, on every engine.

Scenes (built as tests/test_gpu_nonfinite.py builds them): cornell (brute force, 22 boxes: two padding slots),
soup150 (BVH2; deeper than stack_lds 8, and the 4-wide walk with bvh_width 4 once it is not staged), caterpillar
(40 triangles in a 39-level chain: the overflow buffer in the persistent form, the whole stack in LDS in the plain
one), monkey, and monkey with bvh_width 4 (the 4-wide walk).  Rays: the classes of tests/nonfinite_rays.py around the
camera (finite, NaN, +-inf, far origins, the inf_dir_all rays that fill the stacks) plus seeded finite rays, some
with directions that are not unit vectors.

References: oracle.trace (hit flag, k, material), rt_debug_trace (triangle, k), oracle.intersect of the returned
triangle (k), and tests/query_ref.py (u, v; licensed by tests/test_query_api.py).
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests import query_ref as Q
from tests.test_gpu_nonfinite import rays_and_oracle, scene

pytestmark = pytest.mark.gpu

NAN, INF = np.float32(np.nan), np.float32(np.inf)
HORIZON = np.float32(1000.0)
FAST, REF = _native.RT_TRAVERSAL_FAST, _native.RT_TRAVERSAL_REF
CLOSEST, ANY = _native.RT_QUERY_CLOSEST, _native.RT_QUERY_ANY
DEFAULTS = {"bvh": _native.RT_BVH_SAH, "brute_max": 64, "bvh_width": 0, "stack_lds": 0, "block": 128, "resume_min": -1,
            "query_engine": 0, "query_grid": 0}
# name -> (scene of test_gpu_nonfinite, options on top of the scene's own)
SCENES = {"cornell": ("cornell", {}), "soup150": ("soup150", {}), "caterpillar": ("caterpillar", {}),
          "monkey": ("monkey", {}), "monkey_w4": ("monkey", {"bvh_width": 4})}


@pytest.fixture(scope="module")
def kl():
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    k = KernelLauncher(None, None, 0, None)
    yield k
    k.close()


class using:
    """The scene uploaded with its options and the given ones for the length of a with block."""

    def __init__(self, kl, name, traversal=FAST, **options):
        base, own = SCENES[name]
        self.kl, self.sc = kl, scene(base)
        self.options = {**self.sc.options, **own, **options}
        self.traversal = traversal

    def __enter__(self):
        sc = self.sc
        self.kl.upload_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.bvh)
        self.kl.native.set_option("traversal", self.traversal)
        for k, v in self.options.items():
            self.kl.native.set_option(k, v)
        return self.kl.native

    def __exit__(self, *exc):
        for k in self.options:
            self.kl.native.set_option(k, DEFAULTS[k])
        self.kl.native.set_option("traversal", FAST)


def engines(name):
    """The option sets whose closest hits must agree bit for bit (FAST): both forms, every block size, the reduced
    LDS stack, both trees, and on Cornell the tree walk in place of the brute force."""
    e = [dict(query_engine=1), dict(query_engine=2), dict(query_engine=2, block=64), dict(query_engine=2, block=256),
         dict(query_engine=1, block=64), dict(query_engine=1, block=256), dict(query_engine=2, stack_lds=8),
         dict(query_engine=1, stack_lds=8), dict(query_engine=2, bvh=_native.RT_BVH_REFERENCE),
         dict(query_engine=2, bvh=_native.RT_BVH_SAH), dict(query_engine=2, resume_min=0),
         dict(query_engine=2, resume_min=64)]
    if name == "cornell":
        e += [dict(query_engine=1, brute_max=0), dict(query_engine=2, brute_max=0),
              dict(query_engine=2, brute_max=0, stack_lds=8)]
    if name == "soup150":   # with stack_lds 8 it is not staged: bvh_width 4 is then the 4-wide walk
        e += [dict(query_engine=2, stack_lds=8, bvh_width=4), dict(query_engine=2, stack_lds=8, bvh_width=2)]
    return e


@functools.lru_cache(maxsize=None)
def case(name):
    """(rays [n, 6], REF oracle [n, 8], FAST oracle [n, 8], triangles [T, 9]) of a scene: the ray classes with
    their oracle (rays_and_oracle) and 48 seeded finite rays, every fourth not a unit vector."""
    base, _ = SCENES[name]
    sc = scene(base)
    rays, _, want, want_fast = rays_and_oracle(base)
    rng = np.random.default_rng(1600 + len(base))
    vp = sc.V_p.reshape(-1, 3)
    lo, hi = vp.min(0), vp.max(0)
    o = sc.cam[:3] + rng.uniform(-0.3, 0.3, (48, 3))
    d = rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (48, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::4] *= rng.uniform(0.2, 5.0, (12, 1))
    extra = np.concatenate([d, o], axis=1).astype(np.float32)
    osc = O.OracleScene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.bvh, W.ibl_preview())
    w = np.array([O.trace(osc, r) for r in extra])
    wf = w
    if base == "caterpillar":   # FAST has no 20-slot cap: its reference is the oracle on the shallow tree
        from ensem3a_openclraytracer_amd import bvh as B
        shallow = O.OracleScene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData,
                                B.build_export_array(sc.faceData, sc.V_p), W.ibl_preview())
        wf = np.array([O.trace(shallow, r) for r in extra])
    rays = np.concatenate([rays, extra]).astype(np.float32)
    want, want_fast = np.concatenate([want, w]), np.concatenate([want_fast, wf])
    assert 200 <= len(rays) <= 310
    for x in (want, want_fast):
        assert (x[:, 5] == 1).any() and not (x[:, 5] == 1).all()
    return rays, want, want_fast, Q.triangles9(sc)


def rays8(rays6, tmax=None):
    return _native.pack_rays(rays6[:, 3:6], rays6[:, 0:3], tmax)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """Equal bit patterns, or NaN in both."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def lim_of(rays6, tmax):
    """lim = fminf(tmax, 1000) per ray (fmin drops a NaN tmax)."""
    t = HORIZON if tmax is None else np.asarray(tmax, np.float32)
    return np.fmin(np.broadcast_to(t, (len(rays6),)), HORIZON).astype(np.float32)


def check_hits(name, rays6, hits, tri9, tmax=None, label=""):
    """What every result must satisfy whatever the mode: a miss reads (1000, -1, 0, 0); a hit names a triangle the
    oracle's intersect hits with the same k bits, k < lim, and carries the restatement's u, v."""
    hit = hits["tri"] >= 0
    miss = ~hit
    assert (bits(hits["k"][miss]) == bits(HORIZON)).all() and (hits["tri"][miss] == -1).all(), (name, label)
    assert (bits(hits["u"][miss]) == 0).all() and (bits(hits["v"][miss]) == 0).all(), (name, label)
    assert (hits["tri"][hit] < len(tri9)).all()
    lim = lim_of(rays6, tmax)
    assert (hits["k"][hit] < lim[hit]).all(), (name, label)
    for i in np.nonzero(hit)[0]:
        k, flag = O.intersect(tri9[hits["tri"][i]], rays6[i])
        assert flag == 1 and bits(k) == bits(hits["k"][i]), (name, label, i, rays6[i].tolist(), hits[i])
    _, _, u, v = Q.mt(tri9[hits["tri"][hit]], rays6[hit])
    bad = np.nonzero(~(same(u, hits["u"][hit]) & same(v, hits["v"][hit])))[0]
    assert not len(bad), (name, label, [(rays6[hit][i].tolist(), hits[hit][i], u[i], v[i]) for i in bad[:3]])


def check_closest(name, sc, rays6, hits, want, tri9, tmax=None, label=""):
    """The closest-hit contract against oracle.trace's rows: the hit flag (restricted to k < lim), the bits of k and
    the material."""
    lim = lim_of(rays6, tmax)
    exp = (want[:, 5] == 1) & (want[:, 3].astype(np.float32) < lim)
    hit = hits["tri"] >= 0
    bad = np.nonzero(hit != exp)[0]
    assert not len(bad), (name, label, [(rays6[i].tolist(), hits[i], want[i, 3:6].tolist()) for i in bad[:5]])
    assert (bits(hits["k"][hit]) == bits(want[hit, 3])).all(), (name, label)
    np.testing.assert_array_equal(sc.faceData.reshape(-1, 10)[hits["tri"][hit], 0], want[hit, 4], err_msg=f"{name} {label}")
    check_hits(name, rays6, hits, tri9, tmax, label)


# ---- closest hit ----

@pytest.mark.parametrize("traversal", ["ref", "fast"])
@pytest.mark.parametrize("name", list(SCENES))
def test_closest_hit_is_the_frames_hit(kl, name, traversal):
    rays6, want, want_fast, tri9 = case(name)
    trav = REF if traversal == "ref" else FAST
    want = want if trav == REF else want_fast
    for engine in (0, 1, 2):
        with using(kl, name, trav, query_engine=engine) as ctx:
            hits = ctx.trace(rays8(rays6), CLOSEST)
            dbg = ctx.debug_trace(rays6, trav)
        assert hits.dtype == _native.HIT_DTYPE and hits.shape == (len(rays6),)
        check_closest(name, scene(SCENES[name][0]), rays6, hits, want, tri9, label=f"{traversal} engine {engine}")
        hit = hits["tri"] >= 0
        assert hit.any() and not hit.all()
        np.testing.assert_array_equal(hits["tri"], dbg[:, 1].astype(np.int32))
        assert (bits(hits["k"]) == bits(dbg[:, 0])).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_every_engine_and_size_gives_the_same_bits(kl, name):
    rays6, _, want_fast, tri9 = case(name)
    r8 = rays8(rays6)
    with using(kl, name, FAST, query_engine=1) as ctx:
        base = ctx.trace(r8, CLOSEST)
    check_closest(name, scene(SCENES[name][0]), rays6, base, want_fast, tri9)
    for options in engines(name):
        with using(kl, name, FAST, **options) as ctx:
            got = ctx.trace(r8, CLOSEST)
        assert got.tobytes() == base.tobytes(), (name, options, np.nonzero(got != base)[0][:5])


@pytest.mark.parametrize("name", list(SCENES))
def test_one_block_refills_every_lane_many_times(kl, name):
    """query_grid 1: a single block of the persistent form takes the whole stream, so every lane is refilled many
    times (2,000 rays over 128 lanes) and the hand-out meets its edges (1, 63, 64, 65 rays)."""
    rays6, *_ = case(name)
    rng = np.random.default_rng(9)
    big = rays6[rng.integers(len(rays6), size=2000)]
    for n in (1, 63, 64, 65, 2000):
        r8 = rays8(big[:n])
        with using(kl, name, FAST, query_engine=1) as ctx:
            want = ctx.trace(r8, CLOSEST)
        for options in (dict(), dict(block=64), dict(stack_lds=8)):
            with using(kl, name, FAST, query_engine=2, query_grid=1, **options) as ctx:
                got = ctx.trace(r8, CLOSEST)
            assert got.tobytes() == want.tobytes(), (name, n, options, np.nonzero(got != want)[0][:5])


@pytest.mark.parametrize("name", ["monkey", "monkey_w4"])
def test_whole_grid_of_camera_rays_equals_debug_trace(kl, name):
    """1024 x 320 camera rays of the monkey, more than the device keeps resident lanes: the persistent grid's
    hand-out over a long stream, against rt_debug_trace bit for bit."""
    wl = W.PARITY_CASES["monkey_c3_64_s4"].with_size(1024, 320)
    cam = np.asarray(wl.inputs()[1], np.float32)
    n = 1024 * 320
    with using(kl, name, FAST, query_engine=2) as ctx:
        items = np.zeros((n, 11), np.float32)
        items[:, :10] = cam[:10]
        items[:, 10] = np.arange(n, dtype=np.int32).view(np.float32)
        d = ctx.debug_fn("camera", items)
        rays6 = np.concatenate([d, np.broadcast_to(cam[:3], (n, 3))], axis=1).astype(np.float32)
        hits = ctx.trace(rays8(rays6), CLOSEST)
        dbg = ctx.debug_trace(rays6, FAST)
    hit = hits["tri"] >= 0
    assert n // 10 < hit.sum() < n
    np.testing.assert_array_equal(hits["tri"], dbg[:, 1].astype(np.int32))
    assert (bits(hits["k"]) == bits(dbg[:, 0])).all()


# ---- tmax ----

@pytest.mark.parametrize("name", list(SCENES))
def test_tmax_is_a_strict_limit_on_every_engine(kl, name):
    rays6, _, want_fast, tri9 = case(name)
    sc = scene(SCENES[name][0])
    for trav, options in [(FAST, o) for o in engines(name)[:2] + engines(name)[6:7] + engines(name)[12:]] + [(REF, {})]:
        want = want_fast if trav == FAST else case(name)[1]
        with using(kl, name, trav, **options) as ctx:
            base = ctx.trace(rays8(rays6), CLOSEST)
            hit = base["tri"] >= 0
            hr, hb = rays6[hit], base[hit]
            assert len(hr) >= 10
            # the limit is strict: tmax = the hit's own k misses, the next float above it is the same hit
            at = ctx.trace(rays8(hr, hb["k"]), CLOSEST)
            above = ctx.trace(rays8(hr, np.nextafter(hb["k"], INF)), CLOSEST)
            anyat = ctx.trace(rays8(hr, hb["k"]), ANY)
            anyabove = ctx.trace(rays8(hr, np.nextafter(hb["k"], INF)), ANY)
            special = {t: ctx.trace(rays8(rays6, np.float32(t)), CLOSEST) for t in (0.0, -1.0, -INF, NAN, INF, 5000.0)}
            # a limit inside the scene: some hits survive it, some do not
            mid = np.float32(np.median(hb["k"]))
            cut = ctx.trace(rays8(rays6, mid), CLOSEST)
        label = f"{trav} {options}"
        assert (at["tri"] == -1).all() and (anyat["tri"] == -1).all(), (name, label)
        check_hits(name, hr, at, tri9, hb["k"], label)
        assert above.tobytes() == hb.tobytes(), (name, label)
        assert (anyabove["tri"] >= 0).all(), (name, label)
        check_hits(name, hr, anyabove, tri9, np.nextafter(hb["k"], INF), label)
        for t in (0.0, -1.0, -INF):
            assert (special[t]["tri"] == -1).all(), (name, label, t)
            check_hits(name, rays6, special[t], tri9, np.float32(t), label)
        for t in (NAN, INF, 5000.0):   # the reference's horizon
            assert special[t].tobytes() == base.tobytes(), (name, label, t)
        check_closest(name, sc, rays6, cut, want, tri9, mid, label)
        assert 0 < (cut["tri"] >= 0).sum() < hit.sum()


# ---- any hit ----

@pytest.mark.parametrize("name", list(SCENES))
def test_any_hit_flags_equal_the_closest_hits(kl, name):
    rays6, _, want_fast, tri9 = case(name)
    rng = np.random.default_rng(3)
    with using(kl, name, FAST, query_engine=1) as ctx:
        k = ctx.trace(rays8(rays6), CLOSEST)["k"]
    # per-ray limits: the horizon, and limits around the closest hit's distance (below it: a miss)
    tmax = np.where(rng.random(len(rays6)) < 0.4, HORIZON, k * rng.uniform(0.5, 1.5, len(rays6))).astype(np.float32)
    for tm in (None, tmax):
        for trav, options in [(FAST, o) for o in engines(name)] + [(REF, {})]:
            with using(kl, name, trav, **options) as ctx:
                closest = ctx.trace(rays8(rays6, tm), CLOSEST)
                got = ctx.trace(rays8(rays6, tm), ANY)
            label = f"any, {trav} {options} tmax {'set' if tm is not None else 'none'}"
            np.testing.assert_array_equal(got["tri"] >= 0, closest["tri"] >= 0, err_msg=f"{name} {label}")
            assert (got["tri"] >= 0).any() and not (got["tri"] >= 0).all()
            check_hits(name, rays6, got, tri9, tm, label)


# ---- state ----

def test_a_query_leaves_an_open_accumulation_untouched(kl):
    sc = scene("cornell")
    rays6, *_ = case("cornell")
    npix, mb = 32 * 32, 4
    ibl = W.ibl_preview()
    one = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(one, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.bvh, sc.cam,
                         sc.env, npix, 8, mb, ibl)
    ctx = kl.native
    ctx.accum_begin(sc.cam, sc.env, npix, mb)
    try:
        ctx.accum_add(3)
        for engine in (1, 2):
            ctx.set_option("query_engine", engine)
            ctx.trace(rays8(rays6), CLOSEST)
            ctx.trace(rays8(rays6), ANY)
        assert ctx.accum_samples() == 3
        got = ctx.accum_add(5).copy()
    finally:
        ctx.set_option("query_engine", 0)
        ctx.accum_end()
    np.testing.assert_array_equal(got, one)


def test_scene_upload_waits_for_a_query_in_flight():
    """rt_set_scene right after an rt_trace_device enqueued on a caller's stream: the query still traces the old
    scene (the upload, and any free of a buffer it reads, is ordered after it)."""
    import torch
    sc1, sc2 = scene("cornell"), scene("soup150")   # the second's buffers are larger: the upload frees the first's
    rays6, *_ = case("cornell")
    rng = np.random.default_rng(12)
    r8 = rays8(rays6[rng.integers(len(rays6), size=1 << 16)])
    ctx = _native.Context(device_ids=[0])
    try:
        ctx.set_option("query_engine", 2)
        ctx.set_scene(sc1.V_p, sc1.V_n, sc1.V_uv, sc1.faceData, sc1.materialData, sc1.bvh)
        want = ctx.trace(r8, CLOSEST)
        # 4 M rays, tiled on the device: about a millisecond in flight, longer than the small scene's repacking
        d_rays = torch.from_numpy(r8).cuda().repeat(64, 1).contiguous()
        d_out = torch.empty((len(d_rays), 4), dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        ctx.trace_device(0, d_rays.data_ptr(), len(d_rays), CLOSEST, d_out.data_ptr(), s.cuda_stream)
        ctx.set_scene(sc2.V_p, sc2.V_n, sc2.V_uv, sc2.faceData, sc2.materialData, sc2.bvh)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().reshape(64, -1)
        assert all(row.tobytes() == want.tobytes() for row in got)
        # and the next query traces the new scene
        assert ctx.trace(r8, CLOSEST).tobytes() != want.tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["cornell", "monkey"])
def test_two_slots_split_the_rays_in_contiguous_chunks(kl, name):
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    sc = scene(name)
    rays6, *_ = case(name)
    rng = np.random.default_rng(4)
    big = rays6[rng.integers(len(rays6), size=2001)]
    two = KernelLauncher(None, None, [0, 0], None)
    try:
        two.upload_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.bvh)
        for engine in (1, 2):
            two.native.set_option("query_engine", engine)
            for n in (1, 2, 2001):
                with using(kl, name, FAST, query_engine=engine) as ctx:
                    want = ctx.trace(rays8(big[:n]), CLOSEST)
                got = two.native.trace(rays8(big[:n]), CLOSEST)
                assert got.tobytes() == want.tobytes(), (name, engine, n)
    finally:
        two.close()


def test_error_statuses():
    L = _native.lib()
    sc = scene("cornell")
    r8 = rays8(case("cornell")[0][:8])
    out = np.zeros(8, _native.HIT_DTYPE)
    ctx = _native.Context(device_ids=[0])

    def status(fn, *args):
        return fn(ctx.handle, *args)

    p, q = ctypes.c_void_p(r8.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    try:
        assert status(L.rt_trace, p, 8, CLOSEST, q) == _native.RT_ERR_STATE            # no scene
        assert status(L.rt_trace_device, 0, p, 8, CLOSEST, q, None) == _native.RT_ERR_STATE
        ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.bvh)
        assert status(L.rt_trace, p, -1, CLOSEST, q) == _native.RT_ERR_ARG
        assert status(L.rt_trace, p, 1 << 31, CLOSEST, q) == _native.RT_ERR_ARG
        assert status(L.rt_trace, p, 8, 2, q) == _native.RT_ERR_ARG
        assert status(L.rt_trace, p, 8, -1, q) == _native.RT_ERR_ARG
        assert status(L.rt_trace, None, 8, CLOSEST, q) == _native.RT_ERR_ARG
        assert status(L.rt_trace, p, 8, CLOSEST, None) == _native.RT_ERR_ARG
        assert status(L.rt_trace, None, 0, CLOSEST, None) == 0                          # nothing to do
        assert status(L.rt_trace_device, 0, None, 0, ANY, None, None) == 0
        assert status(L.rt_trace, p, 8, CLOSEST, q) == 0 and (out["tri"] >= 0).any()
        import torch
        d_rays = torch.from_numpy(np.concatenate([r8, r8])).cuda()
        d_out = torch.empty((16, 4), dtype=torch.float32, device="cuda")
        rp, op = d_rays.data_ptr(), d_out.data_ptr()
        dev = lambda *a: status(L.rt_trace_device, *[ctypes.c_void_p(x) if i in (1, 4) else x for i, x in enumerate(a)], None)
        assert dev(1, rp, 8, CLOSEST, op) == _native.RT_ERR_ARG                        # one slot only
        assert dev(-1, rp, 8, CLOSEST, op) == _native.RT_ERR_ARG
        assert dev(0, rp + 4, 8, CLOSEST, op) == _native.RT_ERR_ARG                    # alignment
        assert dev(0, rp, 8, CLOSEST, op + 8) == _native.RT_ERR_ARG
        assert dev(0, rp, 8, CLOSEST, rp + 16) == _native.RT_ERR_ARG                   # overlap
        assert dev(0, rp, 8, CLOSEST, rp + 8 * 32 - 16) == _native.RT_ERR_ARG
        assert dev(0, rp, 8, 7, op) == _native.RT_ERR_ARG
        assert dev(0, rp, 8, CLOSEST, rp + 8 * 32) == 0                                # adjacent is not overlapping
        torch.cuda.synchronize()
        assert d_rays[8:12].cpu().numpy().reshape(-1).view(np.uint8).tobytes() == out.tobytes()
        # a scene without the FAST layouts (a node reachable twice): FAST is a state error, REF traces it
        b = np.array(sc.bvh, np.float32).reshape(-1, 9).copy()
        b[int(b[0, 1]), 0] = b[int(b[0, 0]), 0]
        ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, b.ravel())
        assert not ctx.scene_info()["fast_ok"]
        assert status(L.rt_trace, p, 8, CLOSEST, q) == _native.RT_ERR_STATE
        ctx.set_option("traversal", REF)
        assert status(L.rt_trace, p, 8, CLOSEST, q) == 0
        assert L.rt_trace(None, p, 8, CLOSEST, q) == _native.RT_ERR_ARG
    finally:
        ctx.close()


# ---- the launcher ----

def test_trace_rays_host_and_torch_forms_agree(kl):
    import torch
    name = "monkey"
    sc = scene(name)
    rays6, _, want_fast, _ = case(name)
    o, d = rays6[:, 3:6].copy(), rays6[:, 0:3].copy()
    tmax = np.where(np.arange(len(o)) % 3 == 0, np.float32(3.0), HORIZON).astype(np.float32)
    with using(kl, name, FAST):
        for any_hit in (False, True):
            for tm in (None, tmax):
                host = kl.trace_rays(o, d, tm, any_hit=any_hit)
                dev = kl.trace_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(),
                                    None if tm is None else torch.from_numpy(tm).cuda(), any_hit=any_hit)
                torch.cuda.synchronize()
                assert set(host) == set(dev) == {"k", "tri", "u", "v", "hit", "material"}
                for key in host:
                    assert dev[key].is_cuda
                    a, b = host[key], dev[key].cpu().numpy()
                    assert a.shape == b.shape == (len(o),)
                    ok = same(a, b) if a.dtype == np.float32 else a == b
                    assert ok.all(), (key, any_hit, np.nonzero(~ok)[0][:5])
        host = kl.trace_rays(o, d)
    hit = host["hit"]
    np.testing.assert_array_equal(hit, want_fast[:, 5] == 1)
    np.testing.assert_array_equal(host["material"][hit], want_fast[hit, 4])
    assert (host["material"][~hit] == -1).all() and (host["tri"][~hit] == -1).all()
    np.testing.assert_array_equal(host["material"][hit], sc.faceData.reshape(-1, 10)[host["tri"][hit], 0])

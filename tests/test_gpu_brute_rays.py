"""The clustered brute-force trace itself (rt_device.h trace_brute_compact<false, true>, the function the one-lane
product kernels call) on rays aimed at its guards: rt_debug_trace_clustered runs it on the families of
tests/brute_rays.py, one ray per lane, with the scene staged in LDS as the render kernel stages it.

For every scene x family, bit for bit on (k, triangle) of every ray, these are equal: the hook at the automatic
options; the hook with "brute_quad" 0, then also "brute_near" 0, then also "brute_shell" 0; rt_trace's closest hit (the
lock-step loop over brute_box); the numpy reference behind the leaf boxes on every finite ray; and the reference without
boxes on every ray it judges (tests/brute_rays.py judged: the finite rays no box test decides).  info says what each
run walked, so that an "on" run cannot silently be the off code.  The trace is cooperative -- ballots, the ring, owner
lists, the check that no lane passes two faces -- so a ray's result must not depend on its wave: partial waves, a
shuffle, a sort by target wall and a NaN ray in every wave give each ray the result it has in the plain order.  And the
rays and distances a product frame's kernel logged (rt_debug_pixel_log) come back from the hook with the same k."""
import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests import brute_rays as R

pytestmark = pytest.mark.gpu

FAST = _native.RT_TRAVERSAL_FAST
DEFAULTS = dict(brute_max=64, brute_cluster=-1, brute_shell=-1, brute_near=-1, brute_quad=-1)
OFF = (dict(brute_quad=0), dict(brute_quad=0, brute_near=0), dict(brute_quad=0, brute_near=0, brute_shell=0))


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(device_ids=[0])
    c.set_env(W.ibl_preview())
    yield c
    c.close()


class using:
    """Case c's scene uploaded with its own options for the length of a with block."""

    def __init__(self, ctx, c):
        self.ctx, self.c = ctx, c

    def __enter__(self):
        sc = self.c.sc
        self.ctx.set_option("traversal", FAST)
        self.now = dict(DEFAULTS, **self.c.options)
        for key, v in self.now.items():
            self.ctx.set_option(key, v)
        self.ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray)
        return self

    def hook(self, rays, **opts):
        for key, v in dict(DEFAULTS, **dict(self.c.options, **opts)).items():
            if self.now[key] != v:                               # (most of them pack the scene again)
                self.ctx.set_option(key, v)
                self.now[key] = v
        return self.ctx.debug_trace_clustered(rays)

    def __exit__(self, *exc):
        for key, v in DEFAULTS.items():
            self.ctx.set_option(key, v)


def _same(a, b, what, rays=None):
    (ka, ta), (kb, tb) = a, b
    bad = np.flatnonzero((R.bits(ka) != R.bits(kb)) | (np.asarray(ta) != np.asarray(tb)))
    assert not len(bad), (what, len(bad), [(int(i), None if rays is None else rays[i].tolist(), float(ka[i]), int(ta[i]),
                                            float(kb[i]), int(tb[i])) for i in bad[:4]])


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", list(R.SCENES))
def test_every_form_of_the_trace_and_the_reference_agree(ctx, name, family):
    c = R.case(name)
    rays, _ = c.rays(family)
    j = R.judged(c, family)
    with using(ctx, c) as u:
        k, tri, info = u.hook(rays)
        assert info[0] == c.nclusters > 0 and list(info[1:]) == c.info(), (name, info, c.info())
        for opts in OFF:
            k2, tri2, info2 = u.hook(rays, **opts)
            want = c.info(quad=opts.get("brute_quad", -1), near=opts.get("brute_near", -1), shell=opts.get("brute_shell", -1))
            assert info2[0] == c.nclusters and list(info2[1:]) == want, (name, opts, info2, want)
            _same((k, tri), (k2, tri2), (name, family, opts), rays)
        u.hook(rays[:1])                                        # (the automatic options again, for rt_trace)
        hits = ctx.trace(_native.pack_rays(rays[:, 3:6], rays[:, 0:3]), _native.RT_QUERY_CLOSEST)
    _same((k, tri), (hits["k"], hits["tri"]), (name, family, "rt_trace"), rays)
    miss = tri < 0
    assert (R.bits(k[miss]) == R.bits(R.HORIZON)).all() and (tri[miss] == -1).all()
    fin, dec = j["finite"], j["decided"]
    _same((k[fin], tri[fin]), (j["kb"][fin], j["trib"][fin]), (name, family, "reference behind the leaf boxes"), rays[fin])
    _same((k[dec], tri[dec]), (j["k"][dec], j["tri"][dec]), (name, family, "reference"), rays[dec])
    if family != "nonfinite":
        assert fin.all() and dec.mean() >= 0.84, (name, family, dec.mean())


def test_info_follows_the_options_on_cornell(ctx):
    c = R.case("cornell")
    rays = c.rays("band")[0][:256]
    with using(ctx, c) as u:
        assert list(u.hook(rays)[2]) == [2, 1, 1, 1]
        assert list(u.hook(rays, brute_quad=0)[2]) == [2, 1, 1, 0]
        assert list(u.hook(rays, brute_near=0)[2]) == [2, 1, 0, 1]
        assert list(u.hook(rays, brute_shell=0)[2]) == [2, 0, 0, 0]
        assert list(u.hook(rays, brute_near=0, brute_quad=0)[2]) == [2, 1, 0, 0]


def test_a_scene_without_clusters_is_an_error(ctx):
    c = R.case("cornell")
    rays = c.rays("band")[0][:64]
    with using(ctx, c) as u:
        with pytest.raises(_native.NativeError, match="no clustered brute-force array"):
            u.hook(rays, brute_cluster=0)
        with pytest.raises(_native.NativeError, match="no clustered brute-force array"):
            u.hook(rays, brute_max=0)                       # the tree walk's scene: no records at all
        k, tri, _ = u.hook(rays)
        assert (tri >= 0).any()


@pytest.mark.parametrize("name,family", [("cornell", "band"), ("mixed_room", "floor")])
def test_a_rays_result_does_not_depend_on_its_wave(ctx, name, family):
    c = R.case(name)
    rng = np.random.default_rng(99)
    rays, tag = c.rays(family)
    pick = np.sort(rng.choice(len(rays), 4096, replace=False))     # every wall, in the family's order
    rays, tag = rays[pick], tag[pick]
    with using(ctx, c) as u:
        k, tri, _ = u.hook(rays)
        j = R.judged(c, rays)
        _same((k, tri), (j["kb"], j["trib"]), (name, family, "reference behind the leaf boxes"), rays)
        for n in (1, 63, 64, 65, 257):                             # one lane, a partial wave, a block and one lane
            kn, tn, _ = u.hook(rays[:n])
            _same((kn, tn), (k[:n], tri[:n]), (name, "the first %d" % n))
        perm = rng.permutation(len(rays))
        kp, tp, _ = u.hook(rays[perm])
        _same((kp, tp), (k[perm], tri[perm]), (name, "shuffled"))
        by_wall = perm[np.argsort(tag[perm], kind="stable")]
        kw, tw, _ = u.hook(rays[by_wall])
        _same((kw, tw), (k[by_wall], tri[by_wall]), (name, "sorted by wall"))
        # a NaN ray in every wave, at a lane of its own choosing: 63 rays and it
        n = len(rays) // 63 * 63
        mixed = np.full((n // 63, 64, 6), np.nan, R.F32)
        lane = rng.integers(0, 64, n // 63)
        keep = np.ones((n // 63, 64), bool)
        keep[np.arange(n // 63), lane] = False
        mixed[keep] = rays[:n]
        km, tm, _ = u.hook(mixed.reshape(-1, 6))
        _same((km.reshape(-1, 64)[keep], tm.reshape(-1, 64)[keep]), (k[:n], tri[:n]), (name, "a NaN ray in every wave"))
        assert (tm.reshape(-1, 64)[~keep] == -1).all()


def test_the_rays_a_frame_logged_come_back_with_the_logs_k(ctx):
    """Every bounce and sun ray of 64 seeded pixels of cornell_64_s4, as the logging kernel traced them."""
    wl = W.PARITY_CASES["cornell_64_s4"]
    sc, cam, env, npix, spp, mb, ibl = wl.inputs()
    for key, v in DEFAULTS.items():
        ctx.set_option(key, v)
    ctx.set_option("traversal", FAST)
    ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray)
    ctx.set_env(ibl)
    events = []
    for pixel in np.random.default_rng(64).choice(npix, 64, replace=False):
        log, _ = ctx.debug_pixel_log(FAST, cam, env, npix, spp, mb, int(pixel))
        events.append(log[(log[:, 0] == 1) | (log[:, 0] == 2)])
    ev = np.concatenate(events)
    assert len(ev) >= 500 and (ev[:, 0] == 2).sum() >= 50 and (ev[:, 8] == -1).any() and (ev[:, 8] > 0).sum() >= 300
    rays = np.concatenate([ev[:, 5:8], ev[:, 2:5]], axis=1).astype(R.F32)
    k, tri, info = ctx.debug_trace_clustered(rays)
    assert list(info) == [2, 1, 1, 1]
    logged_hit = ev[:, 8] != -1
    assert ((tri >= 0) == logged_hit).all()
    assert (R.bits(k[logged_hit]) == R.bits(ev[logged_hit, 8])).all()
    hits = ctx.trace(_native.pack_rays(rays[:, 3:6], rays[:, 0:3]), _native.RT_QUERY_CLOSEST)
    _same((k, tri), (hits["k"], hits["tri"]), "logged, rt_trace", rays)

"""Option "brute_direct" on the GPU (rt_device.h trace_brute_compact's one queue step: a lane tests the first record of
the wall it leaves through in place, only second records go to the ring) and the LDS copy of the records that the
batches read 16 bytes at a time (stage_mt_records).  Neither changes a test, a cull's effect or a hit:

* rt_debug_trace_clustered -- the product trace itself -- returns, for every scene and family of tests/brute_rays.py,
  the same (k, triangle) bits with the option on and off, and the reference's on every ray that helper judges;
  Cornell's waves are also put together by kind (below);
* frames, progressive adds and listed adds are those of "brute_direct" = 0 and the CPU oracle's, bit for bit;
* the instrumented kernel counts the same work either way;
* the team kernel and the lock-step one-lane kernel, which share the batches and so the records' copy, render the
  oracle's frame.

The shell is walked only by the automatic clusters' kernel, which launch_pick takes from a pixel per resident lane:
1024 x 352 at 4 spp, as in tests/test_gpu_brute_quad.py, whose cases and oracle frames are shared.  At 64 x 64 (8
spp) one lane per pixel is the lock-step kernel: the option has nothing to act on there and must change nothing."""
import numpy as np
import pytest
import torch

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from ensem3a_openclraytracer_amd import workloads as W
from tests import brute_rays as R
from tests import test_gpu_brute_quad as GQ
from tests import test_gpu_brute_shell as S

pytestmark = pytest.mark.gpu

FAST = _native.RT_TRAVERSAL_FAST
RAY_DEFAULTS = dict(brute_max=64, brute_cluster=-1, brute_shell=-1, brute_near=-1, brute_quad=-1, brute_direct=-1)
DEFAULTS = dict(GQ.DEFAULTS, brute_direct=-1)
LARGE, MB = GQ.LARGE, GQ.MB


# ---- the trace itself ------------------------------------------------------------------------------------------------
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
        for key, v in dict(RAY_DEFAULTS, **self.c.options).items():
            self.ctx.set_option(key, v)
        self.ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray)
        return self

    def hook(self, rays, direct=-1):
        self.ctx.set_option("brute_direct", direct)
        on = bool(self.ctx.shell_word() & _native.SHELL_DIRECT)
        assert on == (direct != 0 and self.c.shell is not None), (self.c.name, direct, self.ctx.shell_word())
        k, tri, _ = self.ctx.debug_trace_clustered(rays)
        return k, tri

    def __exit__(self, *exc):
        for key, v in RAY_DEFAULTS.items():
            self.ctx.set_option(key, v)


def _same(a, b, what, rays=None):
    (ka, ta), (kb, tb) = a, b
    bad = np.flatnonzero((R.bits(ka) != R.bits(kb)) | (np.asarray(ta) != np.asarray(tb)))
    assert not len(bad), (what, len(bad), [(int(i), None if rays is None else rays[i].tolist(), float(ka[i]), int(ta[i]),
                                            float(kb[i]), int(tb[i])) for i in bad[:4]])


def _judge(got, j, what, rays):
    k, tri = got
    fin, dec = j["finite"], j["decided"]
    _same((k[fin], tri[fin]), (j["kb"][fin], j["trib"][fin]), (what, "reference behind the leaf boxes"), rays[fin])
    _same((k[dec], tri[dec]), (j["k"][dec], j["tri"][dec]), (what, "reference"), rays[dec])


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", list(R.SCENES))
def test_the_trace_is_the_same_with_the_option_on_and_off(ctx, name, family):
    c = R.case(name)
    rays, _ = c.rays(family)
    with using(ctx, c) as u:
        on = u.hook(rays)
        off = u.hook(rays, direct=0)
        one = u.hook(rays, direct=1)              # 1 means auto
    _same(on, off, (name, family, "brute_direct 0"), rays)
    _same(on, one, (name, family, "brute_direct 1"), rays)
    _judge(on, R.judged(c, family), (name, family), rays)


def _cornell_kinds():
    """Cornell's band, graze and floor rays by what the one queue step does with them: sure (one record, tested in
    place), unsure (in the band or grazing: a second record goes to the ring), absent (they leave through the open
    front: no face's row, pk == ~0u), several (they pass two faces: their wave takes the face-by-face path)."""
    c = R.case("cornell")
    rays = np.concatenate([c.rays(f)[0] for f in ("band", "graze", "floor")])
    face, cond = R.guards(c, rays)
    one = face >= 0
    present = np.zeros(len(rays), bool)
    present[one] = c.present[face[one]]
    split = np.zeros(len(rays), bool)
    split[one] = c.split[face[one]]
    sure = R.sure(cond)
    kinds = dict(sure=one & present & split & sure, unsure=one & present & split & ~sure, absent=one & ~present,
                 several=face == -2)
    return c, rays, {k: np.flatnonzero(v) for k, v in kinds.items()}


def test_waves_of_every_kind_on_cornell(ctx):
    c, rays, kind = _cornell_kinds()
    assert len(kind["sure"]) >= 400 and len(kind["unsure"]) >= 24 and len(kind["absent"]) >= 16 and len(kind["several"]) >= 1
    rng = np.random.default_rng(21)
    nonfinite = c.rays("nonfinite")[0]
    take = {k: iter(rng.permutation(v)) for k, v in kind.items()}

    def wave(**n):
        return np.stack([rays[next(take[k])] for k, m in n.items() for _ in range(m)])

    waves = [wave(sure=64),                                   # every lane tests its one record in place
             wave(sure=40, unsure=24),                        # second records in the ring beside them
             wave(sure=48, absent=16),                        # lanes without a face
             wave(sure=64),
             wave(sure=63, several=1),                        # one ray through two faces: the face-by-face path ...
             wave(sure=64),                                   # ... between waves that take the step
             np.concatenate([wave(sure=50), nonfinite[rng.choice(len(nonfinite), 14, replace=False)]]),
             wave(sure=20, unsure=13)]                        # a partial wave (33)
    for w in waves[:-1]:
        rng.shuffle(w)                                        # (lanes of a kind are not neighbours)
    all_rays = np.ascontiguousarray(np.concatenate(waves), R.F32)
    j = R.judged(c, all_rays)
    with using(ctx, c) as u:
        on, off = u.hook(all_rays), u.hook(all_rays, direct=0)
        _same(on, off, "waves by kind", all_rays)
        _judge(on, j, "waves by kind", all_rays)
        assert (on[1][j["finite"]] >= 0).sum() >= 300
        for n in (1, 33, 64):                                 # a lone ray, a partial wave, one full wave of sure lanes
            kn, tn = u.hook(all_rays[:n])
            _same((kn, tn), (on[0][:n], on[1][:n]), "the first %d" % n)
            _same(u.hook(all_rays[:n], direct=0), (kn, tn), "the first %d, off" % n)
        perm = rng.permutation(len(all_rays))                 # the same rays in other waves
        kp, tp = u.hook(all_rays[perm])
        _same((kp, tp), (on[0][perm], on[1][perm]), "permuted across waves")


# ---- frames ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kl():
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    k = KernelLauncher(None, None, 0, None)
    yield k
    for key, v in DEFAULTS.items():
        k.native.set_option(key, v)
    k.close()


@pytest.fixture(autouse=True)
def _defaults(request):
    yield
    if "kl" in request.fixturenames:
        k = request.getfixturevalue("kl")
        for key, v in DEFAULTS.items():
            k.native.set_option(key, v)


def _set(kl, **opts):
    for key, v in dict(DEFAULTS, **opts).items():
        kl.native.set_option(key, v)


def _frame(kl, name, **opts):
    sc, cam, env = GQ._case(name)
    _set(kl, **opts)
    npix = LARGE[0] * LARGE[1]
    out = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                         sc.BVH.exportArray, cam, env, npix, GQ.SPP, MB, W.ibl_preview())
    return out, _native.last_launch(), _native.last_direct()


@pytest.mark.parametrize("name", ["cornell_bench_camera", "room_wall_centre", "room_on_an_edge"])
def test_one_shot_equals_the_option_off_and_the_oracle(kl, name):
    got, ll, direct = _frame(kl, name)
    assert ll["brute"] & 3 == 3 and ll["shell"] == 1 and direct, ll
    off, ll, direct = _frame(kl, name, brute_direct=0)
    assert ll["brute"] & 3 == 3 and ll["shell"] == 1 and not direct, ll
    S._same(got, off, name)
    S._same(off, GQ._want(name), name)


def _adds(kl, name, direct):
    """Two adds of 2 samples, then 2 samples and 2 more through the list (rt_accum's and rt_adaptive's clustered
    kernels), with "brute_direct" = direct."""
    _set(kl, brute_direct=direct)
    p = GQ._progressive(kl, name)
    for n in (2, 2):
        two = p.add(n)
        ll = _native.last_launch()
        assert ll["acc"] == 1 and ll["brute"] & 3 == 3 and ll["shell"] == 1 and _native.last_direct() == (direct != 0), ll
    two = two.copy()
    p.close()
    p = GQ._progressive(kl, name)
    p.add(2)
    p.select_all()
    listed = p.add_selected(2).copy()
    ll = _native.last_launch()
    assert ll["acc"] == 2 and ll["brute"] & 3 == 3 and ll["shell"] == 1 and _native.last_direct() == (direct != 0), ll
    p.close()
    return two, listed


def test_adds_and_a_listed_add_equal_the_option_off_and_the_oracle(kl):
    name = "cornell_bench_camera"
    two, listed = _adds(kl, name, -1)
    two_off, listed_off = _adds(kl, name, 0)
    S._same(two, two_off, name)
    S._same(listed, listed_off, name)
    S._same(two_off, GQ._want(name), name)
    S._same(listed_off, GQ._want(name), name)


def test_without_split_walls_and_without_a_shell(kl):
    """"brute_quad" 0: every wall queues both records, the first in place and the second through the ring;
    "brute_shell" 0: no record carries the bit and no kernel takes the step."""
    got, ll, direct = _frame(kl, "cornell_bench_camera", brute_quad=0)
    assert ll["brute"] & 3 == 3 and ll["quad"] == 0 and direct, ll
    S._same(got, GQ._want("cornell_bench_camera"), "brute_quad 0")
    got, ll, direct = _frame(kl, "room_wall_centre", brute_shell=0)
    assert ll["brute"] & 3 == 3 and ll["shell"] == 0 and not direct, ll
    S._same(got, GQ._want("room_wall_centre"), "brute_shell 0")
    for bad in (-2, 2):
        with pytest.raises(_native.NativeError, match="brute_direct must be -1"):
            kl.native.set_option("brute_direct", bad)


def test_the_instrumented_kernel_counts_the_same_work(kl):
    """The instrumented kernels compile none of the option's code, so rays and box_tests are equal to the unit.
    tri_tests depends on which rays share a wave (a batch's cull is the owner's best hit as of the last batch), and
    which do is up to the hand-out's race: with the option left alone, three counts of the 1024 x 352 tile gave
    10044110, 10044019 and 10043265, and the first count of a 64 x 64 tile after an upload 170894 against 170871 from
    then on.  So the counts are taken at 128 x 128, after one that is dropped, twice per setting and alternating,
    and the two settings' tri_tests must not lie apart: equal when the counter repeats itself, as it did there
    (694496, six times), else within each other's range."""
    sc, cam, env = GQ._case("cornell_bench_camera")
    cam = S._sized(cam, (128, 128))
    c = _native.Context(device_ids=[0])
    try:
        c.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray)
        c.set_env(W.ibl_preview())
        c.count_work_detail(cam, env, 128 * 128, GQ.SPP, MB)
        counts = {0: [], -1: []}
        for mode in (0, -1, 0, -1):
            c.set_option("brute_direct", mode)
            counts[mode].append(c.count_work_detail(cam, env, 128 * 128, GQ.SPP, MB))
    finally:
        c.close()
    every = counts[0] + counts[-1]
    print("tri_tests", [d["tri_tests"] for d in every], "box_tests", every[0]["box_tests"], "rays", every[0]["rays"])
    assert every[0]["rays"] > 0 and every[0]["tri_tests"] > 0
    assert all(d["rays"] == every[0]["rays"] and d["box_tests"] == every[0]["box_tests"] for d in every)
    off, on = [d["tri_tests"] for d in counts[0]], [d["tri_tests"] for d in counts[-1]]
    assert max(on) >= min(off) and max(off) >= min(on), (off, on)


# ---- 64 x 64 at 8 spp, and the kernels that share the records' copy ---------------------------------------------------
_small = {}


def _small_want(size, spp, row0=0, row_step=1):
    key = (size, spp, row0, row_step)
    if key not in _small:
        sc, cam, env = S._cornell()
        _small[key] = O.render(O.OracleScene.from_scene(sc, W.ibl_preview()), S._sized(cam, size), env, size[0] * size[1],
                               spp, MB, row0=row0, row_step=row_step, nthreads=16)
    return _small[key]


def _small_frame(kl, size, spp, **opts):
    sc, cam, env = S._cornell()
    _set(kl, **opts)
    npix = size[0] * size[1]
    out = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                         sc.BVH.exportArray, S._sized(cam, size), env, npix, spp, MB, W.ibl_preview())
    return out, _native.last_launch()


def test_cornell_64_at_8_spp_one_shot_adds_and_a_listed_add(kl):
    size, spp = (64, 64), 8
    want = _small_want(size, spp)
    sc, cam, env = S._cornell()
    for direct in (-1, 0):
        got, ll = _small_frame(kl, size, spp, team=1, brute_direct=direct)
        assert ll["brute"] & 3 == 1 and ll["team"] == 1, ll       # the lock-step one-lane kernel
        S._same(got, want, "one shot, brute_direct %d" % direct)
        args = (sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.BVH.exportArray,
                S._sized(cam, size), env, size[0] * size[1], MB, W.ibl_preview())
        p = kl.begin_progressive(*args)
        p.add(4)
        S._same(p.add(4), want, "2 x 4 spp, brute_direct %d" % direct)
        p.close()
        p = kl.begin_progressive(*args)
        p.add(4)
        p.select_all()
        S._same(p.add_selected(4), want, "a listed add, brute_direct %d" % direct)
        p.close()


def test_the_team_kernel_reads_the_records_copy(kl):
    """32 x 32 at 4 spp: fewer pixels than lanes, the team rule takes the tile (tests/test_gpu_launch_pick.py)."""
    got, ll = _small_frame(kl, (32, 32), 4)
    assert ll["brute"] == 2 and ll["team"] == 4, ll
    S._same(got, _small_want((32, 32), 4), "teams of 4")


def test_the_lock_step_kernel_reads_the_records_copy(kl):
    """Rows 0::4 of 64 x 64 at 4 spp, one lane per pixel."""
    size, spp = (64, 64), 4
    sc, cam, env = S._cornell()
    _small_frame(kl, size, spp, team=1)                          # (uploads the scene)
    cam = S._sized(cam, size)
    npix = size[0] * size[1]
    t = torch.zeros(3 * size[0] * _native.tile_rows(npix, size[0], 0, 4), dtype=torch.float32, device="cuda")
    kl.native.render_device(cam, env, npix, spp, MB, 0, 4, t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ll = _native.last_launch()
    assert ll["brute"] & 3 == 1 and ll["team"] == 1, ll
    S._same(t.cpu().numpy(), _small_want(size, spp, 0, 4), "rows 0::4")


def test_the_launch_stages_the_records_copy_at_48_bytes_a_record(kl):
    """brute_lds_bytes' figure for Cornell at 1024 x 1024, as the launch got it (rt_debug_last_launch): whole wave areas
    of 4608 bytes, then 48 bytes a record (the copy's stride of three float4, two words of the last unused), a shading
    row of 32 bytes and three frame float4 a triangle, 32 bytes a clustered slot and the shell's seven rows."""
    sc, cam, env, npix, _, mb, ibl = W.CONFIGS["C2"].inputs()
    _set(kl)
    out = np.zeros(3 * npix, np.float32)
    kl.launch_Raytracing(out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData,
                         sc.BVH.exportArray, cam, env, npix, 4, mb, ibl)
    ll = _native.last_launch()
    assert ll["brute"] & 3 == 3 and ll["shell"] == 1 and _native.last_direct(), ll
    info = kl.native.scene_info()
    slots, _, _ = _native.brute_clusters(sc.V_p, sc.V_n, sc.faceData, sc.materialData, sc.BVH.exportArray)
    tables = info["brute_records"] * 48 + info["tris"] * (32 + 48) + len(slots) * 32 + 7 * 32
    waves, rest = divmod(ll["lds"] - tables, 4608)
    assert rest == 0 and waves in (1, 2, 4), (ll, tables)
    assert ll["lds"] % 16 == 0 and tables % 16 == 0

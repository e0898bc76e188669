"""The render kernels' own shading and hit functions, one call at a time (rt_debug_fn), against the CPU oracle's
functions bit for bit, against the reference's recorded outputs (tests/golden/kat_reference.npz) with the
tolerances tests/test_oracle_pins.py applies to the oracle, and -- the FAST box test, a different predicate from
the oracle's -- against a float64 evaluation of its own expression.  The inputs are tests/device_fn_inputs.py's:
the recorded vectors plus the edge classes tests/test_device_fn_inputs.py checks on the CPU.

The comparison is the project's: equal bits, or NaN on both sides."""
import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import _native
from tests import device_fn_inputs as D

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context()
    yield c
    c.close()


def _same(got, ref, S, what):
    """Every row of got equals ref (bits, or NaN in both); the message names the first rows and their classes."""
    got, ref = np.asarray(got, dtype=F32), np.asarray(ref, dtype=F32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ok = D.same_bits(got, ref).reshape(len(got), -1).all(axis=1)
    if not ok.all():
        bad = np.nonzero(~ok)[0]
        cls = S.class_of()
        lines = [f"row {i} ({cls[i]}): in {S.items[i].tolist()} device {got[i].tolist()} expected {ref[i].tolist()}"
                 for i in bad[:5]]
        by = {}
        for i in bad:
            by[cls[i]] = by.get(cls[i], 0) + 1
        pytest.fail(f"{what}: {len(bad)} of {len(got)} rows differ, by class {by}\n" + "\n".join(lines))


# ---- hemisphere samplers ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hemi_dev(ctx):
    """The four device forms on every row: [n, 4 forms (cosine, uniform, sample(true), sample(false)), 6]."""
    return ctx.debug_fn("hemi", D.hemi_set().items).reshape(-1, 4, 6)


@pytest.fixture(scope="module")
def hemi_oracle():
    """oracle.hemi of each row's own kind: dir.xyz, invPdf, seeds after (bits)."""
    it = D.hemi_set().items
    out = np.zeros((len(it), 6), dtype=F32)
    for i, r in enumerate(it):
        d, st = O.hemi(int(r[3]), r[:3], D.bits(r[4:6]))
        out[i, :4] = d
        out[i, 4:6] = D.from_bits(st)
    return out


def test_hemi_forms_match_the_oracle(hemi_dev, hemi_oracle):
    """hemi_cosine and hemi_sample(true) on the frame of a type-1 triangle, hemi_uniform and hemi_sample(false)
    on that of a type-2 one, against MathLib.cl:313-366 as the oracle states it per call: direction, invPdf
    (inf where the direction is in the surface) and the RNG words after."""
    S = D.hemi_set()
    t1 = S.items[:, 3] == 1
    for form, rows, name in ((0, t1, "hemi_cosine"), (2, t1, "hemi_sample(true)"), (1, ~t1, "hemi_uniform"),
                             (3, ~t1, "hemi_sample(false)")):
        got = np.where(rows[:, None], hemi_dev[:, form], hemi_oracle)
        _same(got, hemi_oracle, S, name + " vs oracle.hemi")
    inv = hemi_oracle[t1, 3]
    assert np.isinf(inv).any() and np.isfinite(inv).any()


def test_hemi_sample_is_the_two_samplers(hemi_dev):
    """The tree walks' merged sampler against the megakernel's two, on the device itself and on every row
    (either sampler on either material's frame)."""
    S = D.hemi_set()
    _same(hemi_dev[:, 2].copy(), hemi_dev[:, 0].copy(), S, "hemi_sample(true) vs hemi_cosine")
    _same(hemi_dev[:, 3].copy(), hemi_dev[:, 1].copy(), S, "hemi_sample(false) vs hemi_uniform")


@pytest.mark.parametrize("kind", [1, 2])
def test_hemi_against_the_reference_vectors(hemi_dev, kat_ref, kind):
    """tests/test_oracle_pins.py::test_hemisphere_samplers, with the device in the oracle's place."""
    S = D.hemi_set()
    sl = S.classes[f"kat_type{kind}"]
    for form in ((0, 2) if kind == 1 else (1, 3)):
        d = hemi_dev[sl, form]
        np.testing.assert_array_equal(D.bits(d[:, 4:6]), kat_ref[f"hemi{kind}_state"])  # RNG consumption exact
        ref = kat_ref[f"hemi{kind}_out"]
        ok = np.isfinite(ref[:, 3]) & (np.abs(ref[:, 3]) < 1e6)
        np.testing.assert_allclose(d[ok, :3], ref[ok, :3], rtol=0, atol=2e-5)
        np.testing.assert_allclose(d[ok, 3], ref[ok, 3], rtol=1e-4)


def test_rand_against_the_reference_vectors(ctx, kat_ref):
    """The device's rtm_rand, through the samplers' two draws: the words after two draws are the recorded ones
    after two (rand_state holds them after eight; the oracle's stream, pinned to it, gives the two-draw state)."""
    seeds = kat_ref["rand_seeds"].astype(np.uint32)
    it = np.zeros((len(seeds), 6), dtype=F32)
    it[:, 2] = 1.0
    it[:, 3] = 2.0
    it[:, 4:6] = D.from_bits(seeds.reshape(-1)).reshape(-1, 2)
    dev = ctx.debug_fn("hemi", it).reshape(-1, 4, 6)
    for i, (s0, s1) in enumerate(seeds):
        d8, st8 = O.rand_stream(int(s0), int(s1), 8)
        np.testing.assert_array_equal(d8, kat_ref["rand_out"][i])
        assert st8 == tuple(int(x) for x in kat_ref["rand_state"][i])
        _, st2 = O.rand_stream(int(s0), int(s1), 2)
        for form in range(4):
            assert tuple(int(x) for x in D.bits(dev[i, form, 4:6])) == st2, (i, form)


# ---- camera and sun -------------------------------------------------------------------------------------------
def test_camera_matches_the_oracle_and_the_reference_vectors(ctx, kat_ref):
    S = D.camera_set()
    it = S.items
    dev = ctx.debug_fn("camera", it)
    pix = D.bits(it[:, 10])
    ref = np.stack([O.camera_ray(r[:10], int(p))[:3] for r, p in zip(it, pix)])
    _same(dev, ref, S, "make_const + camera_dir vs oracle.camera_ray")
    k = S.classes["kat"]
    np.testing.assert_allclose(dev[k].reshape(4, -1, 3), kat_ref["cam_out"][:, :, :3], rtol=0, atol=2e-6)


def test_sun_matches_three_rotations(ctx):
    S = D.sun_set()
    dev = ctx.debug_fn("sun", S.items)
    ref = np.zeros_like(dev)
    k = F32(3.14) / F32(180.0)
    for i, e in enumerate(S.items):
        v = np.array([1, 1, 1], dtype=F32)
        for ax, axis in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
            v = O.rotate(float(F32(e[ax] * k)), axis, v)
        ref[i] = v
    _same(dev, ref, S, "make_const().sun vs three oracle.rotate")


# ---- GGX ------------------------------------------------------------------------------------------------------
def test_ggx_matches_the_oracle_and_the_reference_vectors(ctx, kat_ref):
    S = D.ggx_set()
    it = S.items
    dev = ctx.debug_fn("ggx", it)
    ref = np.stack([O.brdf_ggx([2, r[0], r[1], r[2], r[3], 1.5], r[4:7], r[7:10], r[10:13]) for r in it])
    _same(dev, ref, S, "brdf_ggx vs oracle.brdf_ggx")
    np.testing.assert_allclose(dev[S.classes["kat"]], kat_ref["ggx_out"], rtol=2e-5, atol=1e-7)


# ---- IBL ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["1x1", "2x1", "small_ibl", "600x300", "255x3"])
def test_ibl_matches_the_oracle(ctx, env):
    """sample_ibl on the texel-sum table rt_set_env built, against the oracle's four-texel lookup, and
    sample_ibl_if's shortcut: exactly (0, 0, 0) at power +-0, the lookup otherwise.  (The reference's recorded
    texel outputs are not in the fixture -- it was generated without image support -- so no line compares
    with them; small_ibl is its image.)"""
    img = D.ibl_envs()[env]
    S = D.ibl_set()
    it = S.items
    ctx.set_env(img)
    dev = ctx.debug_fn("ibl", it)
    z = np.zeros((3, 1), dtype=F32)
    osc = O.OracleScene(z.T, z.T, None, np.zeros(10, np.int32), np.zeros(6, F32), np.zeros(9, F32), img)
    ref = np.stack([O.sample_ibl(osc, r[:3]) for r in it])
    _same(dev[:, :3], ref, S, f"sample_ibl vs oracle.sample_ibl ({env})")
    off = it[:, 3] == 0
    assert off.any() and np.signbit(it[off, 3]).any() and not np.signbit(it[off, 3]).all()
    assert (D.bits(dev[off, 3:6]) == 0).all(), "sample_ibl_if at power +-0 is exactly +0"
    _same(dev[~off, 3:6], ref[~off], _Rows(S, ~off), f"sample_ibl_if vs oracle.sample_ibl ({env})")
    assert len(np.unique(ref, axis=0)) >= min(img.shape[0] * img.shape[1], 8)   # the lookups are spread


class _Rows:
    """A row subset of a Set, for _same's messages."""

    def __init__(self, S, mask):
        self.items = S.items[mask]
        self._cls = S.class_of()[mask]

    def class_of(self):
        return self._cls


# ---- Moller-Trumbore ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mt_oracle():
    return np.stack([O.intersect(r[:9], r[9:15]) for r in D.mt_set().items])   # k, hit


def test_mt_ref_matches_the_oracle_and_the_reference_vectors(ctx, mt_oracle, kat_ref):
    S = D.mt_set()
    dev = ctx.debug_fn("mt_ref", D.mt_records(S.items))          # hit, k
    _same(dev[:, ::-1].copy(), mt_oracle, S, "mt_test vs oracle.intersect (k, hit)")
    np.testing.assert_array_equal(dev[S.classes["kat"]][:, ::-1], kat_ref["intersect_out"])


def test_mt_fast_matches_the_oracle_and_the_reference_vectors(ctx, mt_oracle, kat_ref):
    """mt_core's hit flag on every row, and its k where it hits (a miss leaves k unused: the branch-free form
    computes it regardless).  Every row has |a| <= 2^126, the range pack_fast guarantees
    (tests/test_device_fn_inputs.py)."""
    S = D.mt_set()
    dev = ctx.debug_fn("mt_fast", D.mt_records(S.items))
    hit = mt_oracle[:, 1] == 1
    got = np.stack([np.where(hit, dev[:, 1], F32(1000.0)), dev[:, 0]], axis=1)
    _same(got, mt_oracle, S, "mt_core vs oracle.intersect (k where hit, hit)")
    np.testing.assert_array_equal(got[S.classes["kat"]], kat_ref["intersect_out"])


# ---- boxes ----------------------------------------------------------------------------------------------------
def test_box_ref_matches_the_oracle_and_the_reference_vectors(ctx, kat_ref):
    S = D.box_set()
    it = S.items
    dev = ctx.debug_fn("box_ref", it[:, :12])[:, 0]
    ref = np.array([O.box(r[:6], r[6:12]) for r in it], dtype=F32)
    _same(dev.reshape(-1, 1), ref.reshape(-1, 1), S, "ref_box vs oracle.box")
    np.testing.assert_array_equal(dev[S.classes["kat"]].astype(bool), kat_ref["box_out"].astype(bool))


def test_box_fast_against_float64(ctx):
    """slab + box_hit with the walks' inverses decide max(tmin, 0) <= min(tmax, cull) as a float64 evaluation of
    the same expression does, except at near-ties (device_fn_inputs.box_fast_reference: the two sides within 4
    float32 ulps; at most 1 % of the items, checked on the CPU).  Off the near-ties the test is never lossy: it
    rejects no box that the oracle's test accepts with tmax >= 0 (and cull = +inf).  And everywhere, near-ties
    and the tie classes included, the decision is box_hit's predicate on the slab values the device returns,
    which are the IEEE float32 evaluation of (b - o) * (1.0f / d)."""
    S = D.box_set()
    it = S.items
    dev = ctx.debug_fn("box_fast", it)
    flag, tmin, tmax = dev[:, 0] == 1, dev[:, 1], dev[:, 2]
    assert set(np.unique(dev[:, 0]).tolist()) <= {0.0, 1.0}
    dec, tie = D.box_fast_reference(it)
    cls = S.class_of()
    bad = np.nonzero(~tie & (flag != dec))[0]
    assert len(bad) == 0, [(int(i), cls[i], it[i].tolist(), dev[i].tolist()) for i in bad[:5]]
    t64min, t64max = D.slab64(it[:, :6], it[:, 6:12])
    ob = np.array([O.box(r[:6], r[6:12]) for r in it])
    must = ~tie & ob & (t64max >= 0) & np.isinf(it[:, 12])
    assert must.sum() > 3000 and flag[must].all(), [(int(i), cls[i]) for i in np.nonzero(must & ~flag)[0][:5]]
    # box_hit itself, exactly
    with np.errstate(invalid="ignore"):
        pred = np.fmax(tmin, F32(0)) <= np.fmin(tmax, it[:, 12])
    bad = np.nonzero(flag != pred)[0]
    assert len(bad) == 0, [(int(i), cls[i], it[i].tolist(), dev[i].tolist()) for i in bad[:5]]
    for k in D.BOX_TIE_CLASSES:
        assert flag[S.classes[k]].any(), k
    assert flag[S.classes["cull_at_tmin"]].any() and (~flag[S.classes["cull_at_tmin"]]).any()
    # the slab values (== : a zero's sign is fminf / fmaxf's own business)
    e_min, e_max = D.slab32(it[:, :6], it[:, 6:12])
    bad = np.nonzero(~((tmin == e_min) | (np.isnan(tmin) & np.isnan(e_min))) |
                     ~((tmax == e_max) | (np.isnan(tmax) & np.isnan(e_max))))[0]
    assert len(bad) == 0, [(int(i), cls[i], it[i].tolist(), dev[i].tolist(), float(e_min[i]), float(e_max[i]))
                           for i in bad[:5]]


def test_hook_rejects_what_it_cannot_evaluate(ctx):
    with pytest.raises(_native.NativeError):
        _native.check(_native.lib().rt_debug_fn(ctx.handle, 99, 0, 0, 0), ctx.handle)
    cam = np.zeros((1, 11), dtype=F32)          # width 0: camera_dir would divide by it
    with pytest.raises(_native.NativeError):
        ctx.debug_fn("camera", cam)
    fresh = _native.Context()
    try:
        with pytest.raises(_native.NativeError, match="no environment"):
            fresh.debug_fn("ibl", np.zeros((1, 4), dtype=F32))
        assert fresh.debug_fn("ggx", np.zeros((0, 13), dtype=F32)).shape == (0, 3)
    finally:
        fresh.close()

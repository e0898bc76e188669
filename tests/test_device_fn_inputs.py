"""The inputs of the per-function device tests (tests/device_fn_inputs.py) do what they are for: checked on the
CPU with the oracle alone, so that a GPU comparison that passes has met the cases it was written for.  Each test
prints its class counts (pytest -s shows them)."""
import numpy as np

import oracle.oracle as O
from tests import device_fn_inputs as D

F32 = np.float32


def _f2i(x):
    """rtm_f2i on an array."""
    x = np.asarray(x, dtype=F32)
    out = np.zeros(x.shape, dtype=np.int64)
    ok = ~np.isnan(x)
    out[ok] = np.clip(np.trunc(x[ok].astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
    return out


def test_every_set_is_small_and_finite_where_it_must_be():
    for name in ("hemi", "ggx", "ibl", "camera", "sun", "mt", "box"):
        S = getattr(D, name + "_set")()
        n = len(S.items)
        print(f"{name}: {n} items, classes " + ", ".join(f"{k} {v.stop - v.start}" for k, v in S.classes.items()))
        assert 0 < n <= D.MAX_ITEMS
        assert sum(v.stop - v.start for v in S.classes.values()) == n
    # non-finite rays belong to tests/test_gpu_nonfinite.py: here rays, triangles and boxes are finite
    assert np.isfinite(D.mt_set().items).all()
    assert np.isfinite(D.box_set().items[:, :12]).all()
    assert not np.isnan(D.box_set().items[:, 12]).any()


def test_normals_take_both_branches_of_the_samplers():
    """At least 50 edge normals take the colinear branch and 50 do not.  The branch is |normalize(n).z| == 1 in
    float32 (device_fn_inputs.colinear32, rtm.h's arithmetic exactly); the oracle confirms it where the branch
    shows: a colinear normal's uniform sample is that of (0, 0, 1) scaled by n.z, bit for bit."""
    normals = D.edge_normals()
    col = np.array([D.colinear32(v) for _, v in normals])
    seeds = (12345, 67890)
    base = O.hemi(2, (0, 0, 1), seeds)[0][:3]
    shown = 0
    for (name, v), c in zip(normals, col):
        got = O.hemi(2, v, seeds)[0][:3]
        as_colinear = (base * F32(v[2])).astype(F32)
        if c:
            assert D.same_bits(got, as_colinear).all(), (name, v)
        elif not D.same_bits(got, as_colinear).all():
            shown += 1
    print(f"edge normals: {col.sum()} colinear, {(~col).sum()} not ({shown} of those visibly rotated by the oracle)")
    assert col.sum() >= 50 and (~col).sum() >= 50 and shown >= 50
    # the threshold itself: the last colinear tilt of (t, 0, +-1), the first one past it, and normals whose
    # normalised z is one float32 step below 1 (1 - 2^-24) -- with z = 1 exactly the first tilt past the
    # threshold normalises to 1 - 2^-23, so that step comes from normals of other lengths
    for sg in (1, -1):
        t_last, t_next = D.tilt_threshold(sg)
        assert D.bits(t_next)[0] == D.bits(t_last)[0] + 1
        assert abs(D.normalize32((t_last, 0, sg))[2]) == 1 and abs(D.normalize32((t_next, 0, sg))[2]) < 1
        assert t_last > F32(1e-4)          # normalize((1e-4, 0, 1)) is still colinear
    nz = np.array([abs(D.normalize32(v)[2]) for _, v in normals])
    one_below = F32(1) - F32(2.0 ** -24)
    print(f"normalised |z| == 1 - 2^-24: {(nz == one_below).sum()} normals, == 1 - 2^-23: "
          f"{(nz == F32(1) - F32(2.0 ** -23)).sum()}")
    assert (nz == one_below).sum() >= 8
    names = {k for k, _ in normals}
    assert {"axis_z", "tilt_last", "tilt_next", "tilt_1e-3", "tilt_1e-2", "tilt_0.1", "axis_xy", "diagonal",
            "length_1e-3", "length_50", "zero", "overflow"} <= names
    over = [v for k, v in normals if k == "overflow"]
    with np.errstate(over="ignore"):
        assert all(np.isinf(np.sum(v.astype(F32) ** 2, dtype=F32)) for v in over)
    types = D.hemi_set().items[:, 3]
    assert set(np.unique(types)) == {1.0, 2.0}


def test_seeds_reach_the_extremes_of_the_draws():
    it = D.hemi_set().items
    pairs = np.unique(D.bits(it[:, 4:6]), axis=0)
    ra, rb = [], []
    for s0, s1 in pairs:
        d, _ = O.rand_stream(int(s0), int(s1), 2)
        ra.append(d[0])
        rb.append(d[1])
    ra, rb = np.array(ra, dtype=F32), np.array(rb, dtype=F32)
    print(f"{len(pairs)} seed pairs: ra == 0 {(ra == 0).sum()}, rb == 0 {(rb == 0).sum()}, ra == max "
          f"{(ra == D.RAND_MAX32).sum()}, rb == max {(rb == D.RAND_MAX32).sum()}")
    assert (ra == 0).any() and (rb == 0).any()
    assert (ra == D.RAND_MAX32).any() and (rb == D.RAND_MAX32).any()
    assert ra.max() == D.RAND_MAX32 and rb.max() == D.RAND_MAX32     # the largest value rtm_rand returns
    for want in ((0, 0), (0, 1), (1, 0), (0xFFFFFFFF, 0xFFFFFFFF)):
        assert (pairs == np.array(want, dtype=np.uint32)).all(axis=1).any(), want
    assert O.rand_stream(0, 0, 4)[1] == (0, 0)       # the stuck state of pixel 0
    for s in (D.SEED_RA0, D.SEED_RB0, D.SEED_RAMAX, D.SEED_RBMAX):
        assert O.rand_stream(7, s, 2)[0].tolist() == O.rand_stream(99, s, 2)[0].tolist()   # the first word is unused


def test_ggx_inputs_meet_the_floor_on_both_sides():
    S = D.ggx_set()
    x = S.items.astype(np.float64)
    v, l, n = x[:, 4:7], x[:, 7:10], x[:, 10:13]
    q = 4 * np.maximum((v * n).sum(1), 0) * np.maximum((l * n).sum(1), 0)
    active = q < 0.001
    print(f"ggx: floor active {active.sum()}, inactive {(~active).sum()}; roughness "
          f"{sorted(set(float(r) for r in np.round(x[S.classes['generic'], 3], 6)))}")
    assert active.sum() >= 1 and (~active).sum() >= 1
    edge = S.classes["floor_edge"]
    assert active[edge].any() and (~active[edge]).any()
    assert set(F32(r) for r in D.GGX_ROUGHNESS) <= set(S.items[:, 3])
    lmv = S.items[S.classes["l_is_minus_v"]]
    assert (lmv[:, 7:10] == -lmv[:, 4:7]).all()
    eq = S.items[S.classes["l_v_n_equal"]]
    assert (eq[:, 7:10] == eq[:, 4:7]).all() and (eq[:, 10:13] == eq[:, 4:7]).all(axis=1).any()
    assert ((v * n).sum(1)[S.classes["v_behind"]] < 0).all()
    nlen = np.linalg.norm(n, axis=1)
    assert (np.abs(nlen - 5) < 1e-5).any() and (np.abs(nlen - 0.2) < 1e-6).any()
    assert (S.items[:, :3] == 0).all(axis=1).any() and (S.items[:, :3] > 1).any() and (S.items[:, :3] < 0).any()
    # the specular term's reciprocal leaves the range of the kernels' short sequence (|x| <= 2^126) on some
    # items, and there the result shows it: a denormal, non-zero
    huge = S.classes["n_huge"]
    assert ((q[huge] > 2.0 ** 126) & (q[huge] < 3.4e38)).all()
    h = S.items[huge]
    out = np.stack([O.brdf_ggx([2, r[0], r[1], r[2], r[3], 1.5], r[4:7], r[7:10], r[10:13]) for r in h])
    tiny = (out != 0) & (np.abs(out) < np.finfo(F32).tiny)
    print(f"ggx n_huge: {int(tiny.all(axis=1).sum())} of {len(h)} items give a denormal result")
    assert tiny.all(axis=1).sum() >= 3


def test_ibl_directions_reach_the_edges_of_the_map():
    """Every environment size has lookups at X = 0 and Y = 0 and at the largest coordinates a direction can
    reach.  Those are W - 1 and H - 1, not the W and H the sum table also holds: u = atan2 * 0.1591 + 0.5 never
    exceeds 0.99982738 and v = asin * 0.3183 + 0.5 never exceeds 0.99998450 (the seam and the pole give them, both
    are in the set), so int(u W) < W and int(v H) < H for every W, H below 5000 -- the table's last row and
    column are read by no lookup, and no input can test them."""
    S = D.ibl_set()
    uv = np.stack([O.spherical_map(d[:3]) for d in S.items])
    u_max = F32(F32(3.14159274) * F32(0.1591) + F32(0.5))
    v_max = F32(F32(1.57079637) * F32(0.3183) + F32(0.5))
    assert np.nanmax(uv[:, 0]) == u_max < 1 and np.nanmax(uv[:, 1]) == v_max < 1
    ring = uv[S.classes["seam_ring"], 0]
    assert (ring < 0.001).sum() >= 1000 and (ring > 0.999).sum() >= 1000      # both sides of the seam
    assert len(ring) == 4096
    assert np.isnan(uv[S.classes["poles"], 1]).any()                          # |d'.y| one step above 1
    assert set(S.items[:, 3].tolist()) == {0.0, 1.0, -1.0} and np.signbit(S.items[S.items[:, 3] == 0, 3]).any()
    envs = D.ibl_envs()
    assert sorted((e.shape[1], e.shape[0]) for e in envs.values()) == [(1, 1), (2, 1), (7, 5), (255, 3), (600, 300)]
    for name, img in envs.items():
        H, W = img.shape[:2]
        X = np.clip(_f2i(uv[:, 0] * F32(W)), 0, W)
        Y = np.clip(_f2i(uv[:, 1] * F32(H)), 0, H)
        print(f"ibl {name}: X {X.min()}..{X.max()} of 0..{W}, Y {Y.min()}..{Y.max()} of 0..{H}, "
              f"{len(set(zip(X.tolist(), Y.tolist())))} table entries")
        assert X.min() == 0 and Y.min() == 0
        assert X.max() == int(u_max * F32(W)) == W - 1 and Y.max() == int(v_max * F32(H)) == H - 1


def test_camera_and_sun_inputs_cover_their_classes():
    S = D.camera_set()
    it = S.items
    pix = D.bits(it[:, 10]).astype(np.int64)
    W = it[:, 6].astype(np.int64)
    npix = W * it[:, 7].astype(np.int64)
    assert (pix >= 0).all() and (pix < np.maximum(npix, pix + 1)).all()
    for w in D.CAM_WIDTHS:
        m = W == w
        got = set(pix[m].tolist())
        h = int(it[m, 7][-1])
        assert {0, w - 1, (h - 1) * w, w * h - 1} <= got, w       # row ends, and the seam pixel i = W - 1
    assert set(D.CAM_FOVS) <= set(it[:, 9])
    for k in (3, 4, 5):
        assert set(F32(a) for a in D.ANGLES) <= set(it[:, k])
    sun = D.sun_set().items
    for k in (0, 1, 2):
        assert set(F32(a) for a in D.ANGLES) <= set(sun[:, k])
    print(f"camera: {len(it)} items over widths {D.CAM_WIDTHS}; sun: {len(sun)} items")


def test_triangle_inputs_sit_on_the_thresholds():
    """The oracle takes every exit of MathLib.cl:117-160 on the inputs, and the exact cases occur: |a| on both
    sides of 1e-7, k on both sides of 1e-7 and (for the traversals) 1e-4, u == 0, v == 0 and u + v == 1."""
    S = D.mt_set()
    it = S.items
    out = np.stack([O.intersect(r[:9], r[9:15]) for r in it])
    hit = out[:, 1] == 1
    print("mt: " + ", ".join(f"{k} {int(hit[v].sum())}/{v.stop - v.start} hit" for k, v in S.classes.items()))
    g = it[S.classes["grid_down"]]
    gh = hit[S.classes["grid_down"]]
    x, y = g[:, 12], g[:, 13]
    assert (gh == (x + y <= 1)).all()                  # the edges u == 0, v == 0, u + v == 1 are hits, exactly
    assert ((x == 0) & gh).any() and ((y == 0) & gh).any() and ((x + y == 1) & gh).any() and (~gh).any()
    assert hit[S.classes["through_vertex"]].all() and hit[S.classes["through_edge"]].all()
    assert not hit[S.classes["in_plane"]].any() and not hit[S.classes["degenerate"]].any()
    a = S.classes["a_at_epsilon"]
    eps = F32(0.0000001)
    az = np.abs(it[a, 11])
    assert (az < eps).any() and (az == eps).any() and (az > eps).any()
    assert not hit[a][az < eps].any() and hit[a][az >= eps].any()
    k = S.classes["k_at_thresholds"]
    kz = it[k, 14]
    assert (hit[k] == (kz > eps)).all() and hit[k].any() and (~hit[k]).any()
    assert (kz[hit[k]] < F32(0.0001)).any() and (kz[hit[k]] > F32(0.0001)).any() and (kz == F32(0.0001)).any()
    r = S.classes["grid_random"]
    assert 100 <= hit[r].sum() <= (r.stop - r.start) - 100
    # mt_core's reciprocal is the IEEE one for |a| <= 2^126, the range pack_fast guarantees: all of these
    t = it.astype(np.float64)
    e1, e2 = t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3]
    assert np.abs((e1 * np.cross(t[:, 9:12], e2)).sum(1)).max() < 2.0 ** 100


def test_box_inputs_and_the_near_tie_share():
    """box_fast is compared with a float64 evaluation except at near-ties (device_fn_inputs.box_fast_reference):
    at most 1 % of the items of each class and 1 % overall may be such.  Three small classes are ties by
    construction (BOX_TIE_CLASSES: the tie is what they test) and count towards the overall share only."""
    S = D.box_set()
    it = S.items
    dec, tie = D.box_fast_reference(it)
    ob = np.array([O.box(r[:6], r[6:12]) for r in it])
    for k, sl in S.classes.items():
        n = sl.stop - sl.start
        print(f"box {k}: {n} items, float64 predicate true {int(dec[sl].sum())}, oracle box true {int(ob[sl].sum())}, "
              f"near-ties {int(tie[sl].sum())} ({100.0 * tie[sl].mean():.2f} %)")
        if k in D.BOX_TIE_CLASSES:
            assert tie[sl].all(), k
        else:
            assert tie[sl].mean() <= 0.01, k
    print(f"box overall: near-ties {int(tie.sum())} of {len(it)} ({100.0 * tie.mean():.2f} %)")
    assert tie.mean() <= 0.01
    assert dec[S.classes["random"]].any() and (~dec[S.classes["random"]]).any()
    assert not dec[S.classes["behind"]].any() and ob[S.classes["behind"]].all()   # tmax >= tmin, but behind
    for k in ("origin_on_face", "origin_on_edge", "origin_on_corner"):
        assert dec[S.classes[k]].all(), k
    z = it[S.classes["zero_component"]]
    assert ((z[:, 0:3] == 0).sum(1) >= 1).all()
    for ax in range(3):
        m = z[:, ax] == 0
        inside = (z[m, 3 + ax] > z[m, 6 + ax]) & (z[m, 3 + ax] < z[m, 9 + ax])
        outside = (z[m, 3 + ax] < z[m, 6 + ax]) | (z[m, 3 + ax] > z[m, 9 + ax])
        assert inside.any() and outside.any() and (inside | outside).all()     # strictly: never on the slab's face
    f = it[S.classes["flat_through"]]
    assert ((f[:, 6:9] == f[:, 9:12]).sum(1) == 1).any() and ((f[:, 6:9] == f[:, 9:12]).sum(1) == 3).any()
    c = it[S.classes["cull_at_tmin"]]
    tmin, _ = D.slab32(c[:, :6], c[:, 6:12])
    step = D.bits(c[:, 12]).astype(np.int64) - D.bits(tmin).astype(np.int64)
    assert set(step.tolist()) == {0, -1, 1}
    assert np.isinf(it[S.classes["random"], 12]).all()
    cull = np.concatenate([it[S.classes["cull_around_tmin"]], it[S.classes["cull_around_tmax"]]])
    d2, _ = D.box_fast_reference(cull)
    assert d2.any() and (~d2).any()

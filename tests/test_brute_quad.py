"""Option "brute_quad" (rt_debug.h; scene_pack.cpp quad_split, rt_device.h quad_pick, rt_layout.h kQuadBand, DESIGN.md
4.2), on the host alone: which walls of a shell the packer splits and on which side of a wall's line its first record
lies, the packer's bound restated, and the proof executed in numpy float32 -- over every split wall of the rooms below,
no ray that passes the wall's face test and that quad_pick is sure of has an accepted Moller-Trumbore hit on the record
quad_pick leaves out.  A cap keeps that honest: on Cornell at least 90 % of the rays that leave through a wall are sure.

The rooms with a reversed diagonal, with mixed diagonals and with a one-triangle wall are built here and rendered by
tests/test_gpu_brute_quad.py."""
import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from tests import test_brute_near as N
from tests.test_brute_shell import UNIT, wall_box

F32 = np.float32
M, G, DMAX = _native.QUAD_BAND, _native.QUAD_GRAZE, _native.QUAD_DIR_MAX
SAFETY, SLACK, RATIO, KAPPA, EXP = 8.0, 2.0 ** -20, 4.0, 4.0, 24      # rt_layout.h kQuad*
EPS = 2.0 ** -24 * (1 + 2.0 ** -10)


# ---- scenes -----------------------------------------------------------------------------------------------------
def _walls_diag(reverse, room=UNIT, single=()):
    """The room's walls as triangle pairs: (c0 c1 c2), (c0 c2 c3) as tests/test_brute_near.py _walls has them, or
    (c0 c1 c3), (c1 c2 c3) -- the other diagonal -- for the faces in `reverse`; one triangle (c0 c1 c2, whose box is
    still the wall's) for the faces in `single`."""
    out = []
    for f in range(6):
        c = N._quad(wall_box(room, f))
        if f in single:
            out += [c[[0, 1, 2]]]
        elif f in reverse:
            out += [c[[0, 1, 3]], c[[1, 2, 3]]]
        else:
            out += [c[[0, 1, 2]], c[[0, 2, 3]]]
    return out


def reversed_room():
    return N.soup(_walls_diag({1}))


def mixed_room():
    return N.soup(_walls_diag({0, 3, 4}))


def one_record_room():
    return N.soup(_walls_diag((), single={3}))


def moved_room(offset):
    """The unit room and its blocks moved by `offset`: sigma then cancels from about |offset| to 1, and the bound
    grows with it."""
    from ensem3a_openclraytracer_amd import bvh as B
    sc = N.soup(_walls_diag(()))
    vp = (sc.V_p.reshape(-1, 3).astype(np.float64) + np.asarray(offset, np.float64)).astype(F32)
    sc.V_p = vp.ravel()
    sc.BVH = B.BVH(sc.faceData, sc.V_p)
    return sc


def far_room():
    return moved_room((300.0, -200.0, 100.0))


SCENES = dict(N.SCENES, reversed_room=reversed_room, mixed_room=mixed_room, one_record_room=one_record_room,
              far_room=far_room, small_room=lambda: N.scaled_room(2.0 ** -20), huge_room=lambda: N.scaled_room(2.0 ** 30))
ALL_SPLIT = ("six_face_room", "reversed_room", "mixed_room", "thin_room", "big_room", "small_room", "far_room")
PROOF_SCENES = ("cornell",) + ALL_SPLIT + ("one_record_room", "skinny_room")


@pytest.fixture(scope="module")
def quads():
    out = {}
    for name in SCENES:
        sc = SCENES[name]()
        out[name] = (_native.brute_quad(*N._args(sc)), _native.brute_shell(*N._args(sc)))
    return out


# ---- the packer -------------------------------------------------------------------------------------------------
def _tri(rec):
    """The vertices of a record p0 e1 e2 in float64 (exact for every split wall: the packer checks it)."""
    p0, e1, e2 = rec.astype(np.float64)
    return np.stack([p0, p0 + e1, p0 + e2])


def _sigma(line, P):
    return P @ line[:3].astype(np.float64) + float(line[3])


def test_the_guards_are_the_constants_of_rt_layout(quads):
    q, _ = quads["cornell"]
    assert (q["guard"] == np.array([2.0 ** -8, 2.0 ** -6, 2.0], F32)).all()
    assert (M, G, DMAX) == (F32(2.0 ** -8), F32(2.0 ** -6), F32(2.0))


@pytest.mark.parametrize("name", ("cornell",) + ALL_SPLIT)
def test_every_wall_is_split_and_the_line_separates_its_records(quads, name):
    q, sh = quads[name]
    present = sh["faces"][:, 0] >= 0
    assert q["nfaces"] == present.sum() == (5 if name == "cornell" else 6)
    assert (q["split"] == present).all() and q["nsplit"] == present.sum(), (name, q["split"])
    for f in np.flatnonzero(q["split"]):
        line, a = q["lines"][f], f // 2
        assert line[a] == 0 and np.isfinite(line).all()
        first_nonzero = line[:3][np.flatnonzero(line[:3])[0]]
        assert first_nonzero > 0                                          # the canonical sign
        t1, t2 = _tri(q["recs"][f, 0]), _tri(q["recs"][f, 1])
        s1, s2 = _sigma(line, t1), _sigma(line, t2)
        s = 1.0 if q["side"][f] else -1.0
        # the expected side bit: the first record's centroid lies on its side, strictly
        assert s * s1.mean() > 0.2 and s * s2.mean() < -0.2, (name, f, s1, s2)
        assert (s * s1 >= -SLACK).all() and (s * s2 <= SLACK).all()
        # the far vertex of the smaller triangle at |sigma| = 1, the larger one's within kQuadRatio
        far = sorted([np.abs(s1).max(), np.abs(s2).max()])
        assert abs(far[0] - 1) <= SLACK and 1 - SLACK <= far[1] <= RATIO + SLACK
        both, pos, neg = (int(w) for w in q["words"][f])
        q0, q1 = both & 0xffff, both >> 16
        assert (q0, q1) == tuple(sh["faces"][f])
        assert (pos, neg) == ((q0 | 0xffff0000, q1 | 0xffff0000) if q["side"][f] else (q1 | 0xffff0000, q0 | 0xffff0000))


def test_the_diagonal_may_run_either_way(quads):
    """Reversing a wall's diagonal turns its line by 90 degrees in the wall's plane; the other walls keep theirs."""
    base, rev, mix = quads["six_face_room"][0], quads["reversed_room"][0], quads["mixed_room"][0]
    for q, turned in ((rev, {1}), (mix, {0, 3, 4})):
        for f in range(6):
            a, b = base["lines"][f], q["lines"][f]
            u, v = [k for k in range(3) if k != f // 2]
            if f in turned:
                assert abs(a[u]) == abs(b[u]) and abs(a[v]) == abs(b[v]) and (a[u] * a[v]) * (b[u] * b[v]) < 0, (f, a, b)
            else:
                assert (a == b).all() and base["side"][f] == q["side"][f]


def test_walls_the_rule_does_not_cover_are_not_split(quads):
    q, _ = quads["skinny_room"]            # the +x wall's second triangle cancels by 2001: not near-safe
    assert q["nfaces"] == 6 and list(q["split"]) == [True, False, True, True, True, True]
    assert (q["lines"][1] == 0).all() and q["words"][1, 0] == q["words"][1, 1] == q["words"][1, 2]
    q, _ = quads["off_plane_room"]         # the +x wall is no face at all
    assert q["nfaces"] == 5 and not q["split"][1] and q["nsplit"] == 5 and (q["words"][1] == 0xffffffff).all()
    q, _ = quads["one_record_room"]        # one triangle: nothing to choose
    assert q["nfaces"] == 6 and list(q["split"]) == [True, True, True, False, True, True]
    assert q["words"][3, 0] >> 16 == 0xffff and (q["words"][3] == q["words"][3, 0]).all() and (q["lines"][3] == 0).all()
    # the proof's ranges: every component within 2^+-24 (2^30 is near-safe, 2^-45 is not even that)
    for name in ("huge_room", "tiny_room"):
        q, _ = quads[name]
        assert q["nfaces"] == 6 and q["nsplit"] == 0 and not q["split"].any() and (q["lines"] == 0).all()
    flags, floor, _ = _native.brute_near(*N._args(SCENES["huge_room"]()))
    assert floor == N.T


def test_the_options_that_clear_it():
    sc = SCENES["cornell"]()
    on = _native.brute_quad(*N._args(sc))
    off = _native.brute_quad(*N._args(sc), quad=0)
    assert off["nfaces"] == 5 and off["nsplit"] == 0 and not off["split"].any() and (off["lines"] == 0).all()
    # ... but the packed words stay: the kernel reads them from the record with the rule off as well
    assert (off["words"][:, 0] == on["words"][:, 0]).all()
    assert (off["words"][:, 1] == off["words"][:, 0]).all() and (off["words"][:, 2] == off["words"][:, 0]).all()
    same = _native.brute_quad(*N._args(sc), quad=1)
    assert (same["lines"] == on["lines"]).all() and (same["split"] == on["split"]).all()
    # no shell, no rows ("brute_shell" 0, or no clusters for it to stand among)
    for cluster, shell in ((-1, 0), (0, -1)):
        none = _native.brute_quad(*N._args(sc), cluster, shell)
        assert none["nfaces"] == 0 and none["nsplit"] == 0 and (none["words"] == 0xffffffff).all()
    # "brute_near" is a launch-time option (DevScene::near_floor) and "brute_quad" does not need it: the packer asks
    # for near-safe walls, which it finds whatever the option; tests/test_gpu_brute_quad.py renders it
    with pytest.raises(_native.NativeError, match="brute_quad must be -1"):
        _native.brute_quad(*N._args(sc), quad=2)


def _coords(rec, ax):
    """The edge coordinates u, v, w of a record over the in-plane point (P[ax[0]], P[ax[1]]): rows (g0, g1, c)."""
    p0, e1, e2 = rec.astype(np.float64)[:, ax]
    n = e1[0] * e2[1] - e1[1] * e2[0]
    u = np.array([e2[1] / n, -e2[0] / n, -(p0[0] * e2[1] - p0[1] * e2[0]) / n])
    v = np.array([-e1[1] / n, e1[0] / n, -(e1[0] * p0[1] - e1[1] * p0[0]) / n])
    return np.stack([u, v, np.array([0, 0, 1.0]) - u - v]), p0, e1, e2, n


def wall_bound(S, f, recs, line, side):
    """DESIGN.md 4.2's bound for face f of shell box S (6 bounds), as scene_pack.cpp quad_split evaluates it:
    max over the two records of E_cls + r (slack + E_mt), and the dropped coordinate's index for each record."""
    S = np.asarray(S, np.float64)
    ax = [(f // 2 + 1) % 3, (f // 2 + 2) % 3]
    W = np.array([S[2 * k + 1] - S[2 * k] for k in ax])
    Cm = np.array([max(abs(S[2 * k]), abs(S[2 * k + 1])) for k in ax])
    corners = np.array([[S[2 * ax[0] + (c & 1)], S[2 * ax[1] + (c >> 1)], 1.0] for c in range(4)])
    A, g = line[:3].astype(np.float64)[ax], float(line[3])
    sig = corners[:, :2] @ A + g
    s = 1.0 if side else -1.0
    Ecls = EPS * (abs(A[0]) * (4 * W[0] + Cm[0]) + abs(A[1]) * (4 * W[1] + Cm[1]) + 3 * (np.abs(A) @ Cm + abs(g)))
    out, which = [], []
    for t, sign in ((0, s), (1, -s)):
        L, p0, e1, e2, n = _coords(recs[t], ax)
        vals = corners @ L.T                                         # [corner, coordinate]
        mx = np.abs(vals).max(axis=0)
        Qu = (W[0] * abs(e2[1]) + W[1] * abs(e2[0])) / abs(n)
        Qv = (W[0] * abs(e1[1]) + W[1] * abs(e1[0])) / abs(n)
        eu, ev = EPS * (24 * mx[0] + 16 * Qu), EPS * (24 * mx[1] + 16 * Qv)
        err = np.array([eu, ev, eu + ev + EPS * (mx[0] + mx[1])])
        # the coordinate that is sign sigma / r over the whole face, r its far vertex's |sigma|
        verts = _tri(recs[t])
        r = np.abs(_sigma(line, verts)).max()
        fit = [k for k in range(3) if np.abs(vals[:, k] - sign * sig / r).max() <= SLACK]
        assert len(fit) == 1, (f, t, vals, sig, r)
        out.append(Ecls + r * (SLACK + err[fit[0]]))
        which.append(fit[0])
    return max(out), which


@pytest.mark.parametrize("name", ("cornell",) + ALL_SPLIT)
def test_the_band_is_eight_bounds_wide_on_every_split_wall(quads, name):
    q, sh = quads[name]
    worst = 0.0
    for f in np.flatnonzero(q["split"]):
        E, _ = wall_bound(sh["box"], f, q["recs"][f], q["lines"][f], q["side"][f])
        assert float(M) >= SAFETY * E, (name, f, E)
        worst = max(worst, E)
    print(name, "largest bound 2^%.2f" % np.log2(worst))
    if name in ("cornell", "six_face_room"):
        assert worst < 2.0 ** -17          # rt_layout.h: 8 times that is 2^6 below the band
    if name == "far_room":
        assert worst > 2.0 ** -14          # ... and the bound does grow with the room's distance from the origin


def test_a_room_too_far_for_the_band_is_not_split():
    sc = moved_room((30000.0, 0.0, 0.0))                  # sigma cancels from 2^14 to 1 on the y and z walls
    q = _native.brute_quad(*N._args(sc))
    assert q["nfaces"] == 6
    assert list(q["split"]) == [True, True, False, False, False, False]


# ---- the rule and the proof, executed ---------------------------------------------------------------------------
def face_pass(S, f, rays, floor=N.T):
    """rt_device.h: the shell's test of face f (floor: kNearFloor), and the per-axis slab distances (mn, mx)."""
    S = np.asarray(S, F32)
    with np.errstate(all="ignore"):
        inv = F32(1.0) / rays[:, 0:3]
        t0, t1 = (S[0::2] - rays[:, 3:6]) * inv, (S[1::2] - rays[:, 3:6]) * inv
        mn, mx = np.fmin(t0, t1), np.fmax(t0, t1)
        a = f // 2
        tf = (t0 if f % 2 == 0 else t1)[:, a]
        lo, hi = mn.copy(), mx.copy()
        lo[:, a], hi[:, a] = tf, tf
        tn = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
        tx = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
        return np.fmax(tn, F32(floor)) <= np.fmin(tx, F32(N.NR.CULL)), mn, mx


def quad_pick(line, f, rays, mn, mx):
    """rt_device.h quad_pick in float32: (sure, sigma~) for rays (dir, origin) against the line of face f."""
    d, o = rays[:, 0:3], rays[:, 3:6]
    line = np.asarray(line, F32)
    with np.errstate(all="ignore"):
        T = np.fmin(np.fmin(mx[:, 0], mx[:, 1]), mx[:, 2])
        P = [N.fma32(T, d[:, k], o[:, k]) for k in range(3)]
        n = len(rays)
        A = [np.full(n, line[k], F32) for k in range(4)]
        sg = N.fma32(A[0], P[0], N.fma32(A[1], P[1], N.fma32(A[2], P[2], A[3])))
        dm = np.fmax(np.fmax(np.abs(d[:, 0]), np.abs(d[:, 1])), np.abs(d[:, 2]))
        inside = np.fmax(np.fmax(mn[:, 0], mn[:, 1]), mn[:, 2]) <= 0
        sure = inside & (T >= 0) & (np.abs(d[:, f // 2]) >= G * dm) & (dm <= DMAX) & (np.abs(sg) >= M)
    return sure, sg


def mt_rec(rec, rays):
    """tests/test_brute_near.py mt_numpy on a record p0 e1 e2 as the kernel reads it; the accepted hits."""
    n = len(rays)
    p0, e1, e2 = (np.broadcast_to(np.asarray(x, F32), (n, 3)) for x in rec)
    d, o = rays[:, 0:3], rays[:, 3:6]
    with np.errstate(all="ignore"):
        h = N._cross(d, e2)
        a = N._dot(e1, h)
        fi = F32(1.0) / a
        s = o - p0
        u = fi * N._dot(s, h)
        q = N._cross(s, e1)
        v = fi * N._dot(d, q)
        k = fi * N._dot(e2, q)
        parallel = (a > F32(-0.0000001)) & (a < F32(0.0000001))
        return (~parallel & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & (k > F32(0.0000001)) & (k > N.C) &
                (k < F32(1000.0)))


def test_the_numpy_record_test_is_mt_numpy():
    q = _native.brute_quad(*N._args(SCENES["cornell"]()))
    rays = _interior_rays(np.array(UNIT, F32), np.random.default_rng(5), 20000)
    for f in (0, 3):
        for t in range(2):
            k, hit = N.mt_numpy(_tri(q["recs"][f, t]).astype(F32), rays)
            with np.errstate(all="ignore"):
                want = hit & (k > N.C) & (k < F32(1000.0))
            assert (mt_rec(q["recs"][f, t], rays) == want).all() and want.sum() > 500


def _unit_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def _interior_rays(S, rng, n):
    o = np.stack([rng.uniform(S[2 * k], S[2 * k + 1], n) for k in range(3)], axis=1).astype(F32)
    return np.concatenate([_unit_dirs(rng, n), o], axis=1)


def _towards(P, o, scale=None):
    """Rays from o through P (float32 differences; scale: a factor per ray on the direction, None: unit length)."""
    d = P.astype(np.float64) - o.astype(np.float64)
    nrm = np.linalg.norm(d, axis=1, keepdims=True)
    d = d / np.maximum(nrm, 1e-300) if scale is None else d * scale[:, None]
    return np.concatenate([d.astype(F32), o.astype(F32)], axis=1)


def _plane_points(S, f, line, rng, n):
    """Points of face f: at sigma = +-m (1 + a few 2^-22 either way) along the line, on the line itself, at the
    corners, along the edges, and anywhere."""
    a = f // 2
    u, v = [k for k in range(3) if k != a]
    lo, hi = np.array([S[2 * u], S[2 * v]], np.float64), np.array([S[2 * u + 1], S[2 * v + 1]], np.float64)
    P = rng.uniform(lo, hi, (n, 2))
    A, g = line[[u, v]].astype(np.float64), float(line[3])
    kind = np.arange(n) % 8
    # move along the line's normal to the wanted sigma
    want = np.where(kind < 4, np.where(kind % 2 == 0, 1.0, -1.0) * float(M) * (1 + rng.integers(-8, 9, n) * 2.0 ** -22), 0.0)
    move = kind < 5                                         # kinds 0-3 at the band's edge, 4 on the line
    sig = P @ A + g
    P[move] += ((want - sig)[:, None] * A / (A @ A))[move]
    edge = kind == 5
    k = rng.integers(0, 2, n)
    P[edge, k[edge]] = np.where(rng.integers(0, 2, n) == 0, lo[k], hi[k])[edge]
    corner = kind == 6
    P[corner] = np.where(rng.integers(0, 2, (n, 2)) == 0, lo, hi)[corner]
    P = np.clip(P, lo, hi)
    out = np.zeros((n, 3))
    out[:, a], out[:, u], out[:, v] = S[f], P[:, 0], P[:, 1]
    return out


def _to_band_edge(S, f, line, rays, span=1 << 14):
    """Rays moved onto the band's edge in float32: for each ray that passes face f, the origin's in-plane coordinate
    along the line's larger component is stepped ulp by ulp (a bisection over +-span ulps: sigma~ is monotone in it,
    every operation on the way being monotone) to the two adjacent floats between which |sigma~| >= m flips.  Returns
    both rays of each pair: the nearest a float32 ray comes to |sigma~| = m from either side."""
    a = f // 2
    u, v = [k for k in range(3) if k != a]
    b = u if abs(line[u]) >= abs(line[v]) else v
    ok, mn, mx = face_pass(S, f, rays)
    rays = rays[ok]
    _, sg0 = quad_pick(line, f, rays, mn[ok], mx[ok])
    side = np.where(sg0 >= 0, 1.0, -1.0)
    up = side * np.sign(float(line[b]))                     # +1: the signed distance from the line grows with o_b

    def outside(n):                                         # is |sigma~| >= m on the ray's side, at step n
        r = rays.copy()
        r[:, 3 + b] = N._ulp_step(rays[:, 3 + b], (n * up).astype(np.int64))
        _, mn_, mx_ = face_pass(S, f, r)
        _, sg = quad_pick(line, f, r, mn_, mx_)
        with np.errstate(all="ignore"):
            return side * sg >= M, r

    lo, hi = np.full(len(rays), -span, np.int64), np.full(len(rays), span, np.int64)
    good = ~outside(lo)[0] & outside(hi)[0]                 # the edge lies within the span
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        o = outside(mid)[0]
        hi, lo = np.where(o, mid, hi), np.where(o, lo, mid)
    return np.concatenate([outside(lo)[1][good], outside(hi)[1][good]]), int(good.sum())


def _guard_dirs(S, f, P, rng):
    """Origins for rays through the plane points P of face f whose direction sits at the grazing guard: |d_a| =
    g max(|d_b|, |d_c|), and one ulp either side; the origin inside the box, a short way back along the ray."""
    n = len(P)
    a = f // 2
    u, v = [k for k in range(3) if k != a]
    d = np.zeros((n, 3), F32)
    swap = rng.integers(0, 2, n) == 1
    mag = rng.choice([0.25, 0.5, 1.0, 1.9], n).astype(F32)
    other = (mag * rng.uniform(-1, 1, n)).astype(F32)
    d[:, u] = np.where(swap, other, mag * rng.choice([-1, 1], n)).astype(F32)
    d[:, v] = np.where(swap, mag * rng.choice([-1, 1], n), other).astype(F32)
    da = N._ulp_step(F32(G) * mag, rng.integers(-1, 2, n))
    d[:, a] = da if f % 2 == 1 else -da                     # towards the face
    # back along the ray while the origin stays in the box: T in (0, Tmax)
    Sd = np.asarray(S, np.float64)
    with np.errstate(all="ignore"):
        room = [np.where(d[:, k] > 0, (P[:, k] - Sd[2 * k]) / d[:, k], np.where(d[:, k] < 0, (P[:, k] - Sd[2 * k + 1]) / d[:, k], np.inf))
                for k in range(3)]
    T = np.minimum(np.minimum(room[0], room[1]), room[2]) * rng.uniform(0.05, 0.95, n)
    o = P - T[:, None] * d.astype(np.float64)
    return np.concatenate([d, o.astype(F32)], axis=1)


def _boundary_origins(S, rng, n):
    """Origins on the faces, edges and corners of the box: one, two or three coordinates snapped to a bound."""
    o = np.stack([rng.uniform(S[2 * k], S[2 * k + 1], n) for k in range(3)], axis=1)
    nsnap = 1 + np.arange(n) % 3
    for j in range(3):
        k = rng.integers(0, 3, n) if j else np.arange(n) % 3
        snap = nsnap > j
        o[snap, k[snap]] = np.where(rng.integers(0, 2, n) == 0, np.asarray(S)[2 * k], np.asarray(S)[2 * k + 1])[snap]
    return o


N_RANDOM = 1_000_000
N_AIMED = 60_000


@pytest.mark.parametrize("name", PROOF_SCENES)
def test_no_sure_ray_hits_the_record_it_does_not_queue(quads, name):
    q, sh = quads[name]
    S = sh["box"].astype(F32)
    rng = np.random.default_rng(1900 + len(name))
    rays = [_interior_rays(S, rng, N_RANDOM)]
    nedge = 0
    for f in np.flatnonzero(q["split"]):
        P = _plane_points(S, f, q["lines"][f], rng, N_AIMED)
        o = np.stack([rng.uniform(S[2 * k], S[2 * k + 1], N_AIMED) for k in range(3)], axis=1)
        rays.append(_towards(P, o))
        rays.append(_towards(P, o, rng.choice([2.0 ** -6, 0.3, 0.9], N_AIMED)))        # not unit length
        rays.append(_towards(P, _boundary_origins(S, rng, N_AIMED)))
        rays.append(_guard_dirs(S, f, P, rng))
        edge, npairs = _to_band_edge(S, f, q["lines"][f], np.concatenate(rays[-4:-2])[(np.arange(2 * N_AIMED) % 8) < 4])
        rays.append(edge)
        nedge += npairs
    with np.errstate(all="ignore"):
        extra = list(N.NR.ray_classes([0.0, 0.0, 0.0], np.concatenate([S[0::2], S[1::2]])[None, :], seed=3).values())
    rays = np.concatenate(rays + extra).astype(F32)
    nsure = ndropped_close = 0
    for f in range(6):
        if sh["faces"][f, 0] < 0:
            continue
        ok, mn, mx = face_pass(S, f, rays)
        sub, mn, mx = rays[ok], mn[ok], mx[ok]
        sure, sg = quad_pick(q["lines"][f], f, sub, mn, mx)
        if not q["split"][f]:
            assert not sure.any(), (name, f)                  # a zero line: sigma~ is 0 or a NaN
            continue
        first_dropped = sure & ((sg < 0) == bool(q["side"][f]))          # sigma~ >= 0 queues the positive side's
        for t, dropped in ((0, first_dropped), (1, sure & ~first_dropped)):
            bad = mt_rec(q["recs"][f, t], sub[dropped])
            assert not bad.any(), (name, f, t, sub[dropped][bad][:3], sg[dropped][bad][:3])
            with np.errstate(all="ignore"):
                ndropped_close += int((np.abs(sg[dropped]) < F32(1.01) * M).sum())
        # ... and the record that is queued is the only one of the two that can be hit: nothing else is lost
        kept_hits = mt_rec(q["recs"][f, 0], sub[sure & ~first_dropped]).sum() + mt_rec(q["recs"][f, 1], sub[first_dropped]).sum()
        # (the thin room's rays between its x walls travel less than the hit condition's 1e-4: fewer are accepted;
        # the small room's all do, and in the big room only a ray that starts within 1000 of a wall passes its test)
        if name not in ("big_room", "small_room"):
            assert kept_hits > (0.5 if name == "thin_room" else 0.9) * sure.sum(), (name, f, kept_hits, sure.sum())
        nsure += int(sure.sum())
    if q["nsplit"] and name not in ("big_room", "small_room"):
        assert nsure >= 500_000 and ndropped_close >= 10_000, (name, nsure, ndropped_close)
        assert nedge >= 10_000 * q["nsplit"], (name, nedge)      # adjacent-float pairs across the band's edge, per wall


def test_one_ulp_inside_the_guards_is_sure_and_one_ulp_outside_is_not(quads):
    """The unit room's +x wall (sigma = 0.5 y - 0.5 z, exact in float32 for the points below): a ray from (0, y, z)
    along (1, 0, 0) has T = 1 and P~ = (1, y, z) exactly."""
    q, sh = quads["six_face_room"]
    S = sh["box"].astype(F32)
    f, line = 1, q["lines"][1]
    assert (line == np.array([0, 0.5, -0.5, 0], F32)).all()

    def pick(d, o):
        rays = np.array([list(d) + list(o)], F32)
        ok, mn, mx = face_pass(S, f, rays)
        assert ok[0]
        sure, sg = quad_pick(line, f, rays, mn, mx)
        return bool(sure[0]), float(sg[0])

    two_m = F32(2) * M
    below, above = np.nextafter(two_m, F32(0)), np.nextafter(two_m, F32(1))
    for sign in (1, -1):
        assert pick((1, 0, 0), (0, sign * two_m, 0)) == (True, sign * float(M))
        assert pick((1, 0, 0), (0, sign * above, 0))[0] is True
        sure, sg = pick((1, 0, 0), (0, sign * below, 0))
        assert sure is False and abs(sg) < float(M)
        assert pick((1, 0, 0), (0, 0, -sign * two_m)) == (True, sign * float(M))
    # the grazing guard, closed: |d_a| = g max|d| is sure, one ulp less is not (the plane point stays far from the line)
    for dmax in (F32(1.0), F32(0.5), F32(2.0)):
        da = G * dmax
        assert pick((da, dmax, 0), (F32(1) - da * F32(0.25), F32(-0.75), F32(0.5)))[0] is True
        assert pick((np.nextafter(da, F32(0)), dmax, 0), (F32(1) - da * F32(0.25), F32(-0.75), F32(0.5)))[0] is False
        assert pick((np.nextafter(da, F32(1)), -dmax * F32(0.5), dmax), (F32(1) - da * F32(0.25), F32(-0.5), F32(0.25)))[0] is True
    # the direction's magnitude, closed at kQuadDirMax; an origin outside the box; a NaN anywhere
    o = (F32(0.5), F32(-0.5), F32(0.5))
    assert pick((2, 0, 0), o)[0] is True and pick((np.nextafter(F32(2), F32(3)), 0, 0), o)[0] is False
    rays = np.array([[1, 0, 0, -1.5, -0.5, 0.5], [1, 0, 0, 0.5, np.nan, 0.5], [1, np.nan, 0, 0.5, -0.5, 0.5],
                     [np.nan, 0, 0, 0.5, -0.5, 0.5], [1, 0, 0, 0.5, np.inf, 0.5], [0, 0, 0, 1, -0.5, 0.5]], F32)
    ok, mn, mx = face_pass(S, f, rays)
    sure, _ = quad_pick(line, f, rays, mn, mx)
    assert not sure.any()


def test_at_least_nine_in_ten_of_cornells_wall_rays_are_sure(quads):
    """The cap: 10^6 interior origins, uniform directions, the exit face a real wall (not the open front)."""
    q, sh = quads["cornell"]
    S = sh["box"].astype(F32)
    rays = _interior_rays(S, np.random.default_rng(19), N_RANDOM)
    nwall = nsure = 0
    for f in range(6):
        ok, mn, mx = face_pass(S, f, rays)
        if sh["faces"][f, 0] < 0:
            assert ok.sum() > 100_000         # the open front
            continue
        sure, _ = quad_pick(q["lines"][f], f, rays[ok], mn[ok], mx[ok])
        nwall += int(ok.sum())
        nsure += int(sure.sum())
    print("sure: %d of %d wall rays (%.2f %%)" % (nsure, nwall, 100.0 * nsure / nwall))
    assert nwall > 800_000 and nsure >= 0.9 * nwall

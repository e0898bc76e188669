"""Inputs of the per-function device tests (tests/test_gpu_device_fns.py), and the CPU check that they do what
they are for (tests/test_device_fn_inputs.py).  No GPU import: numpy, the committed known-answer vectors of
the reference (tests/golden/kat_reference.npz) and, for the float32 arithmetic of a few constructions, nothing
but IEEE operations numpy performs exactly.

Every builder returns a ``Set``: ``items`` (float32[n, k], integer words as bit patterns), ``classes``
(name -> slice of rows) and whatever index arrays tie rows to the recorded vectors.  Each array stays at or
below MAX_ITEMS rows.
"""
from __future__ import annotations

import functools
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_ITEMS = 20000
F32 = np.float32
U32 = np.uint32


@functools.lru_cache(maxsize=None)
def kat():
    with np.load(os.path.join(GOLDEN, "kat_reference.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=F32).view(U32)


def from_bits(u) -> np.ndarray:
    return np.ascontiguousarray(u, dtype=U32).view(F32)


def same_bits(a, b) -> np.ndarray:
    """The project's comparison: equal bits, or NaN on both sides (elementwise)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return (a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))


def ulp_step(x, n: int) -> np.ndarray:
    """x moved n float32 steps (n of either sign) along the finite positive or negative floats."""
    u = bits(x).astype(np.int64)
    return from_bits((u + n).astype(U32))


class Set:
    def __init__(self, width: int):
        self.width = width
        self._rows = []
        self.classes = {}
        self._n = 0

    def add(self, name: str, rows) -> slice:
        rows = np.ascontiguousarray(rows, dtype=F32).reshape(-1, self.width)
        assert name not in self.classes and len(rows) > 0, name
        sl = slice(self._n, self._n + len(rows))
        self.classes[name] = sl
        self._rows.append(rows)
        self._n += len(rows)
        return sl

    @property
    def items(self) -> np.ndarray:
        if len(self._rows) != 1:
            self._rows = [np.concatenate(self._rows)]
        assert len(self._rows[0]) <= MAX_ITEMS, len(self._rows[0])
        return self._rows[0]

    def class_of(self) -> np.ndarray:
        out = np.empty(self._n, dtype=object)
        for k, sl in self.classes.items():
            out[sl] = k
        return out


# ---- float32 arithmetic of rtm.h, exactly (small inputs only: Fractions) ---------------------------------------
def _round_f32(fr: Fraction) -> np.float32:
    """The float32 nearest to an exact value (ties to even)."""
    if fr == 0:
        return F32(0)
    with np.errstate(over="ignore"):
        c = F32(float(fr))
    if not np.isfinite(c):
        return c
    best = c
    for nb in (np.nextafter(c, F32(-np.inf)), np.nextafter(c, F32(np.inf))):
        if not np.isfinite(nb):
            continue
        d1, d0 = abs(Fraction(float(nb)) - fr), abs(Fraction(float(best)) - fr)
        if d1 < d0 or (d1 == d0 and (int(nb.view(U32)) & 1) == 0):
            best = nb
    return best


def fma32(a, b, c) -> np.float32:
    a, b, c = F32(a), F32(b), F32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return F32(a * b + c)
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def normalize32(v):
    """rtm_normalize: v * (1 / sqrtf(fma dot))."""
    x, y, z = (F32(t) for t in v)
    with np.errstate(all="ignore"):
        dot = fma32(z, z, fma32(y, y, x * x))
        s = F32(1) / np.sqrt(dot)
        return np.array([x * s, y * s, z * s], dtype=F32)


def colinear32(v) -> bool:
    """The samplers' branch (MathLib.cl:325, 349): |normalize(n).z| == 1."""
    return bool(np.abs(normalize32(v)[2]) == F32(1))


@functools.lru_cache(maxsize=None)
def tilt_threshold(sign: int):
    """(t_last, t_next): the largest t for which normalize((t, 0, sign)).z is still +-1 in float32, and the
    next float32 up, the smallest tilt that leaves the colinear branch."""
    lo, hi = int(bits(F32(1e-6))[0]), int(bits(F32(1e-2))[0])
    assert colinear32((from_bits(lo)[0], 0, sign)) and not colinear32((from_bits(hi)[0], 0, sign))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if colinear32((from_bits(mid)[0], 0, sign)):
            lo = mid
        else:
            hi = mid
    return from_bits(lo)[0], from_bits(hi)[0]


# ---- hemisphere samplers ----------------------------------------------------------------------------------------
# second RNG words (the samplers' first draw reads only its second argument's word) whose first / second draw is
# 0 or the largest value rtm_rand returns, 1 - 2^-23 (found by search; test_device_fn_inputs checks them)
SEED_RA0, SEED_RB0, SEED_RAMAX, SEED_RBMAX = 0x8D482, 0x21024B, 0x5DBEC9, 0x761BF9
RAND_MAX32 = F32(1) - F32(2.0 ** -23)
EDGE_SEEDS = [(0, 0), (0, 1), (1, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF),
              (7, SEED_RA0), (7, SEED_RB0), (7, SEED_RAMAX), (7, SEED_RBMAX)]


def edge_normals():
    """[(class, n.xyz)]: the normals of the issue's edge classes."""
    out = []
    for sg in (1.0, -1.0):
        for sc in (1.0, 3.0, 1e-3):
            out.append(("axis_z", (0, 0, sg * sc)))
        t_last, t_next = tilt_threshold(int(sg))
        for name, t in (("tilt_last", t_last), ("tilt_next", t_next), ("tilt_1e-3", 1e-3), ("tilt_1e-2", 1e-2),
                        ("tilt_0.1", 0.1)):
            for ax, ay in ((1, 0), (0, 1), (-1, 0), (0.6, -0.8)):
                raw = np.array([t * ax, t * ay, sg], dtype=F32)
                out.append((name, raw))                      # as a loader leaves it, |n| slightly above 1
                out.append((name + "_unit", normalize32(raw)))   # stored normalised: z rounds below 1
                out.append((name + "_x3", raw * F32(3)))
        # tiny tilts well inside the colinear branch, in many directions and lengths
        for k in range(24):
            t = F32(10.0 ** (-8 + 4.3 * k / 23))
            ph = 0.7 * k
            out.append(("tilt_tiny", np.array([t * np.cos(ph), t * np.sin(ph), sg], dtype=F32) *
                        F32((1.0, 3.0, 1e-3)[k % 3])))
    # the unit normals one and two float32 steps below |z| = 1 (normalised z = 1 - 2^-24, 1 - 2^-23)
    for sg in (1.0, -1.0):
        for steps in (1, 2):
            z = ulp_step(F32(1), -steps)[0]
            x = F32(np.sqrt(1.0 - float(z) ** 2))
            out.append(("z_below_one", (x, 0, sg * z)))
            out.append(("z_below_one", (0, -x, sg * z)))
    for a in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)):
        out.append(("axis_xy", a))
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                out.append(("diagonal", (sx, sy, sz)))
                out.append(("diagonal_unit", normalize32((sx, sy, sz))))
    for a in ((1, 1, 0), (1, 0, 1), (0, 1, 1), (-1, 1, 0), (1, 0, -1), (0, -1, -1)):
        out.append(("diagonal", a))
    rng = np.random.default_rng(11)
    for k in range(24):
        u = rng.standard_normal(3)
        u /= np.linalg.norm(u)
        out.append(("length_1e-3", u * 1e-3))
        out.append(("length_50", u * 50.0))
    out.append(("zero", (0, 0, 0)))
    out.append(("zero", (0.0, -0.0, -0.0)))
    out.append(("overflow", (3e19, 3e19, 3e19)))      # dot(n, n) = inf
    out.append(("overflow", (0, 0, 3e19)))
    out.append(("overflow", (1e-3, 0, -2e19)))
    return [(k, np.asarray(v, dtype=F32)) for k, v in out]


@functools.lru_cache(maxsize=None)
def hemi_set() -> Set:
    """Rows: n.xyz, material type (1 cosine, 2 uniform), seed0 bits, seed1 bits (oracle.hemi's order).
    Rows [0, 3000) / [3000, 6000): the recorded normals and seeds as type 1 / 2; then every edge normal x
    type x edge seed; then recorded normals under the edge seeds."""
    K = kat()
    n, seeds = K["hemi_n"].astype(F32), K["hemi_seeds_in"].astype(U32)
    S = Set(6)

    def rows(normals, types, sd):
        r = np.zeros((len(normals), 6), dtype=F32)
        r[:, :3] = normals
        r[:, 3] = types
        r[:, 4:6] = from_bits(np.asarray(sd, dtype=U32).reshape(-1)).reshape(-1, 2)
        return r

    S.add("kat_type1", rows(n, 1, seeds))
    S.add("kat_type2", rows(n, 2, seeds))
    by_class = {}
    for k, v in edge_normals():
        by_class.setdefault(k, []).append(v)
    for k, vs in by_class.items():
        nn, tt, ss = [], [], []
        for v in vs:
            for t in (1, 2):
                for si, sd in enumerate(EDGE_SEEDS + [tuple(int(x) for x in seeds[(len(nn) + 13) % len(seeds)])]):
                    nn.append(v)
                    tt.append(t)
                    ss.append(sd)
        S.add(k, rows(np.array(nn), np.array(tt), np.array(ss, dtype=np.uint64).astype(U32)))
    m = 60
    nn = np.repeat(n[:m], len(EDGE_SEEDS), axis=0)
    ss = np.tile(np.array(EDGE_SEEDS, dtype=np.uint64).astype(U32), (m, 1))
    S.add("kat_normals_edge_seeds_type1", rows(nn, 1, ss))
    S.add("kat_normals_edge_seeds_type2", rows(nn, 2, ss))
    S.items
    return S


# ---- GGX ------------------------------------------------------------------------------------------------------
GGX_ROUGHNESS = (0.0, 1e-4, 0.25, 1.0, 2.0, -0.3)
GGX_COLOURS = ((0.0, 0.0, 0.0), (2.0, 3.0, 1.5), (-0.5, -1.0, -0.1), (0.8, 0.5, 0.3))


def _basis(n):
    n = np.asarray(n, dtype=np.float64)
    n = n / np.linalg.norm(n)
    a = np.array([1.0, 0, 0]) if abs(n[0]) < 0.9 else np.array([0, 1.0, 0])
    t = np.cross(n, a)
    t /= np.linalg.norm(t)
    return t, np.cross(n, t), n


@functools.lru_cache(maxsize=None)
def ggx_set() -> Set:
    """Rows: colour.rgb, roughness, v.xyz, l.xyz, n.xyz.  Rows [0, 2000): the recorded vectors."""
    K = kat()
    g = K["ggx_in"].astype(F32)
    S = Set(13)
    S.add("kat", np.concatenate([g[:, 1:5], g[:, 6:15]], axis=1))

    def el(elev, az):   # a direction by its height above the tangent plane
        c = np.sqrt(max(0.0, 1.0 - elev * elev))
        return np.array([c * np.cos(az), c * np.sin(az), elev])

    configs = []   # (class, v, l) in the frame of n = z
    configs.append(("l_is_minus_v", el(0.6, 0.3), -el(0.6, 0.3)))
    configs.append(("l_is_minus_v", el(1e-4, 2.0), -el(1e-4, 2.0)))
    configs.append(("l_v_n_equal", el(1.0, 0.0), el(1.0, 0.0)))
    for ev in (1e-4, 1e-5, 0.0, -1e-5, -1e-4):
        for elv in (1e-4, 3e-5, 0.0, -1e-4, 0.5):
            configs.append(("tangent", el(ev, 0.4), el(elv, 2.5)))
    configs.append(("tangent", el(0.7, 0.4), el(1e-4, -1.0)))
    # 4 (n.v) (n.l) on both sides of the 0.001 floor
    for p in (0.0158, 0.01581, 0.015812, 0.0159, 0.01, 0.02):
        configs.append(("floor_edge", el(p, 0.1), el(p, 1.3)))
    configs.append(("floor_edge", el(0.5, 0.1), el(0.0005, 1.3)))
    configs.append(("floor_edge", el(0.5, 0.1), el(0.000501, 1.3)))
    for ev in (-0.3, -0.9, -1.0):
        configs.append(("v_behind", el(ev, 0.2), el(0.5, 1.0)))
    configs.append(("l_behind", el(0.4, 0.2), el(-0.5, 1.0)))
    rng = np.random.default_rng(21)
    for _ in range(12):
        configs.append(("generic", el(rng.uniform(0.05, 1), rng.uniform(0, 6.28)),
                        el(rng.uniform(0.05, 1), rng.uniform(0, 6.28))))
    normals = [((0, 0, 1), 1.0), ((0, 0, 1), 5.0), ((0, 0, 1), 0.2), ((0.3, -0.5, 0.81), 1.0), ((-0.7, 0.1, -0.7), 5.0)]
    per = {}
    for name, v, l in configs:
        for nd, nl in normals:
            t, b, n = _basis(nd)
            V = v[0] * t + v[1] * b + v[2] * n
            L = l[0] * t + l[1] * b + l[2] * n
            if name in ("l_is_minus_v", "l_v_n_equal"):   # exact in float32, not only to rounding
                V = V.astype(F32)
                L = (-V if name == "l_is_minus_v" else V)
            N = (n.astype(F32) if name == "l_v_n_equal" and nl == 1.0 else n * nl)
            if name == "l_v_n_equal" and nl == 1.0:
                V = L = N
            for r in GGX_ROUGHNESS:
                for c in GGX_COLOURS:
                    per.setdefault(name, []).append(np.concatenate([c, [r], V, L, N]))
    # |n| = 1e19: 4 (n.v) (n.l) lies above 2^126, where the reciprocal of the specular term is denormal -- past the
    # range of the kernels' short reciprocal sequence (dev_recip's IEEE branch); with colour 0 and roughness 1 the
    # result is that denormal times F G D, and nothing else
    for nl in (1e19, 1.3e19, 1.6e19):
        for ev, elv in ((0.5, 0.5), (0.9, 0.3), (0.35, 0.8)):
            for r in GGX_ROUGHNESS:
                for c in GGX_COLOURS:
                    per.setdefault("n_huge", []).append(np.concatenate([c, [r], el(ev, 0.3), el(elv, 2.0), [0, 0, nl]]))
    for name, rows in per.items():
        S.add(name, np.array(rows))
    S.items
    return S


# ---- IBL ------------------------------------------------------------------------------------------------------
IBL_POWERS = (0.0, -0.0, 1.0, -1.0)


@functools.lru_cache(maxsize=None)
def ibl_envs():
    """name -> uint8[H, W, 4]: 1x1, 2x1, the recorded 5 x 7 image, 600x300 and 255x3 (W x H), with full-white
    and black texels among seeded noise so a channel sum reaches 4 x 255."""
    rng = np.random.default_rng(31)
    out = {}
    for name, (w, h) in (("1x1", (1, 1)), ("2x1", (2, 1)), ("600x300", (600, 300)), ("255x3", (255, 3))):
        img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        img[rng.random((h, w)) < 0.1] = 255
        img[rng.random((h, w)) < 0.05] = 0
        if name == "1x1":
            img[...] = (255, 254, 1, 9)
        out[name] = img
    out["small_ibl"] = np.ascontiguousarray(kat()["small_ibl"])
    return out


@functools.lru_cache(maxsize=None)
def ibl_set() -> Set:
    """Rows: dir.xyz, power.  The same rows serve every environment of ibl_envs()."""
    S = Set(4)
    S.add("kat", K3(kat()["ibl_dirs"]))
    ax = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=F32)
    S.add("axes", K3(np.concatenate([ax, ax * F32(3), ax * F32(1e-3)])))
    S.add("zero", K3(np.array([(0, 0, 0), (-0.0, 0, 0), (0, -0.0, -0.0)], dtype=F32)))
    # the atan2 seam and the poles, placed in the map's own frame d' = Ry(1.57) Rx(1.57) dir (u = atan2(d'.z,
    # d'.x), v = asin(d'.y); 1.57 = 90 * 3.14 / 180, not pi / 2) and turned back in float64.  The seam u = 0 | 1
    # is the half plane d'.z = 0, d'.x < 0: a ring of 4096 directions about it over the whole height of the map,
    # the closest 1e-8 radians to each side (float32 then decides which side such a direction is on)
    k = np.arange(2048)
    off = 1e-8 * (2e7) ** (k / 2047.0)          # 1e-8 .. 0.2
    elev = np.where(k % 2 == 0, 0.0, 1.5 * np.sin(k))
    ring = [_ibl_unrotate(np.stack([-np.cos(elev) * np.cos(off), np.sin(elev), sgn * np.cos(elev) * np.sin(off)],
                                   axis=1)) for sgn in (1.0, -1.0)]
    S.add("seam_ring", K3(np.concatenate(ring)))
    # both poles d' = (0, +-1, 0) with perturbations down to one float32 step of each component
    pole = []
    for sg in (1.0, -1.0):
        for e in (0.0, 1e-8, 1e-6, 1e-4, 1e-3, 2e-3, 1e-2, 0.1):
            for a, b in ((1, 0), (0, 1), (-1, 0), (0, -1), (0.7, 0.7)):
                pole.append(_ibl_unrotate(np.array([[e * a, sg * np.sqrt(1 - e * e * (a * a + b * b)), e * b]]))[0])
        p0 = _ibl_unrotate(np.array([[0.0, sg, 0.0]]))[0].astype(F32)
        for c in range(3):
            for st in (-3, -2, -1, 1, 2, 3):
                q = p0.copy()
                q[c] = ulp_step(q[c], st)[0]     # |d'.y| may exceed 1: asin -> NaN
                pole.append(q)
    S.add("poles", K3(np.array(pole)))
    rng = np.random.default_rng(33)
    g = rng.standard_normal((2000, 3))
    S.add("random", K3(g / np.linalg.norm(g, axis=1, keepdims=True)))
    S.items
    return S


def _ibl_unrotate(dp):
    """dir for which SampleSphericalMap's two turns give d' (float64 rotation matrices)."""
    a = 90.0 * (3.14 / 180.0)
    c, sn = np.cos(a), np.sin(a)
    rx = np.array([[1, 0, 0], [0, c, -sn], [0, sn, c]])
    ry = np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]])
    return np.asarray(dp, dtype=np.float64) @ (ry @ rx)     # rows: (Ry Rx)^T d'


def K3(d):
    d = np.asarray(d, dtype=F32)
    r = np.zeros((len(d), 4), dtype=F32)
    r[:, :3] = d
    r[:, 3] = np.array(IBL_POWERS, dtype=F32)[np.arange(len(d)) % 4]
    return r


# ---- camera and sun -------------------------------------------------------------------------------------------
ANGLES = (0.0, 90.0, -90.0, 180.0, 360.0, 1e4)
CAM_WIDTHS = (1, 2, 3, 40, 4096)
CAM_FOVS = tuple(np.float32(d * 3.14 / 180.0) for d in (1.0, 45.0, 179.0))


def cam_pixels(w: int, h: int):
    """First and last pixel of the first and last row, the seam pixel i = W - 1 where (i + 1) % W wraps, and
    the start of the second row."""
    return sorted({0, w - 1, (h - 1) * w, w * h - 1, min(w, w * h - 1), (h // 2) * w + w // 2})


@functools.lru_cache(maxsize=None)
def camera_set() -> Set:
    """Rows: cam[10], pixel index bits.  Rows [0, 4 * 216): the recorded cameras x cam_idx."""
    K = kat()
    S = Set(11)
    rows = []
    for cam in K["cams"]:
        for i in K["cam_idx"]:
            rows.append(np.concatenate([cam.astype(F32), from_bits([int(i)])]))
    S.add("kat", np.array(rows))
    for w in CAM_WIDTHS:
        h = 3 if w <= 3 else w
        rows = []
        for fi, fov in enumerate(CAM_FOVS):
            for ai, rx in enumerate(ANGLES):
                for bi, ry in enumerate(ANGLES):
                    for ci, rz in enumerate(ANGLES):
                        pix = cam_pixels(w, h)
                        # every pixel for the axis-aligned third of the rotations, two of them for the rest
                        if (ai + bi + ci) % 3:
                            j = (ai + 2 * bi + 3 * ci + fi)
                            pix = [pix[j % len(pix)], pix[(j + 1) % len(pix)]] if len(pix) > 1 else pix
                        pos = (0.5, -3.5, 0.25) if (ai + bi) % 2 else (0.0, 0.0, 0.0)
                        for p in pix:
                            rows.append(np.concatenate([np.array([*pos, rx, ry, rz, w, h, 1.0, fov], dtype=F32),
                                                        from_bits([p])]))
        S.add(f"width_{w}", np.array(rows))
    S.items
    return S


@functools.lru_cache(maxsize=None)
def sun_set() -> Set:
    """Rows: env[5] (sun angles x, y, z in degrees, sun power, IBL power)."""
    S = Set(5)
    rows = [(a, b, c, 1.0, 0.5) for a in ANGLES for b in ANGLES for c in ANGLES]
    S.add("angles", np.array(rows))
    rng = np.random.default_rng(41)
    S.add("random", np.concatenate([rng.uniform(-400, 400, (200, 3)), np.ones((200, 2))], axis=1))
    S.items
    return S


# ---- Moller-Trumbore ------------------------------------------------------------------------------------------
def mt_records(tri9_ray6) -> np.ndarray:
    """tri9 (a, b, c), ray6 (dir, origin) -> rt_debug_fn's 24 floats: a.p | 0, e1 | 0, e2 | 0 with e1 = b - a
    and e2 = c - a formed in float32 as scene_pack.cpp forms them, dir, origin, 6 unused."""
    x = np.ascontiguousarray(tri9_ray6, dtype=F32)
    r = np.zeros((len(x), 24), dtype=F32)
    r[:, 0:3] = x[:, 0:3]
    r[:, 4:7] = x[:, 3:6] - x[:, 0:3]
    r[:, 8:11] = x[:, 6:9] - x[:, 0:3]
    r[:, 12:18] = x[:, 9:15]
    return r


@functools.lru_cache(maxsize=None)
def mt_set() -> Set:
    """Rows: a.xyz, b.xyz, c.xyz, dir.xyz, origin.xyz (oracle.intersect's arguments).  Rows [0, 4000): the
    recorded vectors."""
    K = kat()
    S = Set(15)
    S.add("kat", K["intersect_in"])
    A, B, C = (0, 0, 0), (1, 0, 0), (0, 1, 0)
    unit = [*A, *B, *C]
    down = (0, 0, -1)

    def row(tri, d, o):
        return np.array([*tri, *d, *o], dtype=F32)

    g = np.arange(0, 65, 4) / 64.0
    # a 1/64 grid of rays straight down on the unit triangle: u = x, v = y exactly, so u == 0, v == 0 and
    # u + v == 1 occur exactly, with points on either side
    S.add("grid_down", np.array([row(unit, down, (x, y, 1)) for x in g for y in g]))
    S.add("grid_up_k_negative", np.array([row(unit, (0, 0, 1), (x, y, 1)) for x in g[::4] for y in g[::4]]))
    verts, edges = [], []
    for d in ((0, 0, -1), (0, 0, -0.25), (0.25, 0, -1), (0, -0.5, -1), (0.25, 0.25, -0.5)):
        d = np.array(d, dtype=np.float64)
        for p in (A, B, C):
            verts.append(row(unit, d, np.array(p) - d))            # through the vertex at k = 1
        for p, q in ((A, B), (B, C), (C, A)):
            for s in (0.25, 0.5, 0.75):
                m = np.array(p) * (1 - s) + np.array(q) * s
                edges.append(row(unit, d, m - d))                  # through a point of the edge
    S.add("through_vertex", np.array(verts))
    S.add("through_edge", np.array(edges))
    inplane = []
    for p, q in ((A, B), (B, C), (C, A)):
        p, q = np.array(p, dtype=np.float64), np.array(q, dtype=np.float64)
        inplane.append(row(unit, q - p, p - (q - p)))              # along the edge, in the plane
        inplane.append(row(unit, p - q, q + 2 * (q - p)))
    inplane.append(row(unit, (1, 1, 0), (-1, -1, 0)))
    inplane.append(row(unit, (1, 0.5, 0), (-1, 0.1, 0)))
    inplane.append(row(unit, (1, 0.5, 0), (-1, 0.1, 1e-3)))        # parallel, off the plane
    S.add("in_plane", np.array(inplane))
    # a = e1 . (d x e2) = -d.z on the unit triangle: |a| on both sides of EPSILON = 1e-7f = 0x33D6BF95
    eps = from_bits(np.arange(0x33D6BF92, 0x33D6BF99, dtype=U32))
    S.add("a_at_epsilon", np.array([row(unit, (0, 0, sg * e), (0.25, 0.25, -sg * 1.0)) for e in eps for sg in (1, -1)] +
                                   [row(unit, (0.5, 0.25, sg * e), (0.25, 0.25, -sg * e)) for e in eps for sg in (1, -1)]))
    # k = origin.z for rays straight down: both sides of 1e-7f (the hit's own threshold) and 1e-4f = 0x38D1B717
    ks = np.concatenate([eps, from_bits(np.arange(0x38D1B714, 0x38D1B71B, dtype=U32)), np.array([0.0, -1e-7], dtype=F32)])
    S.add("k_at_thresholds", np.array([row(unit, down, (0.25, 0.5, k)) for k in ks]))
    deg = []
    for tri in ([*A, *A, *C], [*A, *B, *B], [*C, *B, *C], [*A, *A, *A], [0, 0, 0, 1, 1, 0, 2, 2, 0],
                [0, 0, 0, 0.5, 0, 0, 1, 0, 0], [-1, 2, 3, 0, 2, 3, 3, 2, 3]):
        for d, o in ((down, (0.25, 0.25, 1)), (down, (0, 0, 1)), ((1, 1, -1), (-1, -1, 1)), ((0, 0, 1), (0.5, 2, 0))):
            deg.append(row(tri, d, o))
    S.add("degenerate", np.array(deg))
    # seeded triangles and rays on the 1/64 grid (exact edge vectors and barycentric numerators), some hit
    rng = np.random.default_rng(51)
    n = 3000
    tri = rng.integers(-128, 129, (n, 9)) / 64.0
    tgt = rng.integers(-128, 129, (n, 3)) / 64.0
    w = rng.integers(0, 9, (n, 3))
    w[w.sum(1) == 0] = 1
    inside = (tri.reshape(n, 3, 3) * (w / w.sum(1, keepdims=True))[:, :, None]).sum(1)
    tgt[: n // 2] = np.round(inside[: n // 2] * 64) / 64.0
    org = rng.integers(-256, 257, (n, 3)) / 64.0
    d = tgt - org
    d[np.abs(d).sum(1) == 0] = (0, 0, 1)
    S.add("grid_random", np.concatenate([tri, d, org], axis=1))
    S.items
    return S


# ---- boxes ----------------------------------------------------------------------------------------------------
def slab32(ray6, box6):
    """slab() of rt_device.h in float32: (b - o) * (1.0f / d), the kernels' nesting of fmin / fmax.  Finite
    rays and boxes; a zero direction component gives an infinite inverse as on the device."""
    r, b = np.ascontiguousarray(ray6, dtype=F32), np.ascontiguousarray(box6, dtype=F32)
    with np.errstate(all="ignore"):
        inv = F32(1) / r[:, 0:3]
        t0 = (b[:, 0:3] - r[:, 3:6]) * inv
        t1 = (b[:, 3:6] - r[:, 3:6]) * inv
    lo, hi = np.fmin(t0, t1), np.fmax(t0, t1)
    tmin = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
    tmax = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
    return tmin, tmax


def slab64(ray6, box6):
    """The same expression evaluated in float64 from the float32 differences b - o and the float32 d."""
    r, b = np.ascontiguousarray(ray6, dtype=F32), np.ascontiguousarray(box6, dtype=F32)
    with np.errstate(all="ignore"):
        inv = 1.0 / r[:, 0:3].astype(np.float64)
        t0 = (b[:, 0:3] - r[:, 3:6]).astype(np.float64) * inv
        t1 = (b[:, 3:6] - r[:, 3:6]).astype(np.float64) * inv
    lo, hi = np.fmin(t0, t1), np.fmax(t0, t1)
    tmin = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
    tmax = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
    return tmin, tmax


def box_fast_reference(items13):
    """(decision, near_tie) of box_hit's predicate max(tmin, 0) <= min(tmax, cull) in float64.  near_tie: the
    two sides lie within 4 float32 ulps of the larger magnitude -- each product (b - o) * fl(1 / d) is within
    1.5 ulp of the exact quotient, so tmin and tmax are each off by at most 2 ulp and only there may the float32
    decision differ."""
    x = np.ascontiguousarray(items13, dtype=F32)
    tmin, tmax = slab64(x[:, 0:6], x[:, 6:12])
    lhs = np.fmax(tmin, 0.0)
    rhs = np.fmin(tmax, x[:, 12].astype(np.float64))
    with np.errstate(all="ignore"):
        big = np.maximum(np.abs(lhs), np.abs(rhs))
        ulp = np.spacing(np.where(np.isfinite(big), big, 0.0).astype(F32)).astype(np.float64)
        tie = np.abs(lhs - rhs) <= 4.0 * ulp
        tie |= np.isnan(lhs) | np.isnan(rhs) | ((lhs == rhs))
    return lhs <= rhs, tie


# classes of box_set() whose items are ties of the predicate by construction (both sides are the same slab value):
# a ray through a flat box has tmin == tmax, a ray leaving from the boundary has tmax == 0 == max(tmin, 0), and a
# cull at tmin or one ulp from it is the tie itself.  The
# float64 comparison says nothing about them; box_hit's decision there is checked exactly, against the slab
# values the device returns.
BOX_TIE_CLASSES = ("boundary_leaving", "flat_through", "cull_at_tmin")


@functools.lru_cache(maxsize=None)
def box_set() -> Set:
    """Rows: dir.xyz, origin.xyz, lo.xyz, hi.xyz, cull.  Rows [0, 4000): the recorded vectors (cull = +inf)."""
    K = kat()
    S = Set(13)
    inf = F32(np.inf)

    def with_cull(r12, cull):
        r12 = np.ascontiguousarray(r12, dtype=F32).reshape(-1, 12)
        return np.concatenate([r12, np.broadcast_to(np.asarray(cull, dtype=F32), (len(r12),)).reshape(-1, 1)], axis=1)

    S.add("kat", with_cull(K["box_in"], inf))
    box = (-1, -0.5, 0.25, 1, 1.5, 2.25)
    lo, hi = np.array(box[:3]), np.array(box[3:])
    dirs = [(1, 0.5, 0.25), (-1, 0.5, 0.25), (0.3, -1, 0.2), (-0.3, -0.2, -1), (1, 1, 1), (-1, -1, -1), (0.1, 0.9, -0.4),
            (1, 2, 3), (-3, 1, 2)]
    mid = (lo + hi) / 2
    face, edge, corner = [], [], []
    for d in dirs:
        for ax in range(3):
            for side in (lo, hi):
                o = mid.copy()
                o[ax] = side[ax]
                face.append([*d, *o, *box])
                o2 = o.copy()
                o2[(ax + 1) % 3] = side[(ax + 1) % 3]
                edge.append([*d, *o2, *box])
        for cx in (lo[0], hi[0]):
            for cy in (lo[1], hi[1]):
                for cz in (lo[2], hi[2]):
                    corner.append([*d, cx, cy, cz, *box])
    # a ray that leaves the box from its boundary has tmax = 0 = max(tmin, 0): a tie of the predicate (a class of
    # its own, BOX_TIE_CLASSES); the rays that enter, or run along a face, stay in the three classes
    leaving = []
    for name, rows in (("origin_on_face", face), ("origin_on_edge", edge), ("origin_on_corner", corner)):
        rows = with_cull(rows, inf)
        tie = box_fast_reference(rows)[1]
        S.add(name, rows[~tie])
        leaving.append(rows[tie][::4])
    S.add("boundary_leaving", np.concatenate(leaving))
    behind = []
    for d in dirs:
        dd = np.array(d, dtype=np.float64)
        for s in (2.0, 5.0, 40.0):
            behind.append([*d, *(mid + s * dd), *box])     # the whole box lies behind the origin
    S.add("behind", with_cull(behind, inf))
    rng = np.random.default_rng(61)
    flat_through, flat_miss = [], []
    for k in range(24):
        ax = k % 3
        b_lo, b_hi = lo.copy(), hi.copy()
        b_hi[ax] = b_lo[ax]
        if k % 4 == 3:
            b_hi = b_lo.copy()                              # a point: flat on three axes
        tgt = (b_lo + b_hi) / 2
        d = rng.uniform(-1, 1, 3)
        d[ax] = (1 if k % 2 else -1) * rng.uniform(0.3, 1)
        flat_through.append([*d, *(tgt - 2.5 * d), *b_lo, *b_hi])
        off = np.zeros(3)
        off[(ax + 1) % 3] = 5.0
        flat_miss.append([*d, *(tgt - 2.5 * d + off), *b_lo, *b_hi])
    S.add("flat_through", with_cull(flat_through, inf))
    S.add("flat_miss", with_cull(flat_miss, inf))
    zero = []
    for ax in range(3):
        for d in dirs[:6]:
            d = np.array(d, dtype=np.float64)
            d[ax] = 0.0
            for sgn0 in (0.0, -0.0):
                d[ax] = sgn0
                for where in ("inside", "below", "above"):
                    o = mid - 3.0 * np.where(d != 0, d, 0)
                    o[ax] = {"inside": mid[ax] + 0.125, "below": lo[ax] - 0.5, "above": hi[ax] + 0.75}[where]
                    zero.append([*d, *o, *box])
        d2 = np.zeros(3)
        d2[ax] = 1.0                                        # two zero components
        for o in (mid - 4 * d2, mid - 4 * d2 + np.roll([5.0, 0, 0], ax + 1)):
            zero.append([*d2, *o, *box])
    S.add("zero_component", with_cull(zero, inf))
    # seeded rays at seeded boxes, half aimed into the box; finite culls around the interval
    n = 5000
    c = rng.uniform(-4, 4, (n, 3))
    ext = rng.uniform(0.05, 2, (n, 3))
    b6 = np.concatenate([c - ext, c + ext], axis=1)
    o = rng.uniform(-8, 8, (n, 3))
    aim = c + rng.uniform(-1, 1, (n, 3)) * ext * np.where(np.arange(n)[:, None] % 2 == 0, 0.9, 2.5)
    d = aim - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r12 = np.concatenate([d, o, b6], axis=1).astype(F32)
    S.add("random", with_cull(r12, inf))
    tmin, tmax = slab32(r12[:, :6], r12[:, 6:])
    ok = (tmin > 0) & (tmax >= tmin)
    r_ok, tn, tx = r12[ok][:1500], tmin[ok][:1500], tmax[ok][:1500]
    fr = np.array([0.5, 0.9, 1.1, 2.0], dtype=F32)[np.arange(len(tn)) % 4]
    S.add("cull_around_tmin", np.concatenate([r_ok, (tn * fr).reshape(-1, 1)], axis=1))
    S.add("cull_around_tmax", np.concatenate([r_ok, ((tn + (tx - tn) * fr)).astype(F32).reshape(-1, 1)], axis=1))
    ties = []
    for i in range(10):
        for st in (0, -1, 1):
            ties.append([*r_ok[i], ulp_step(tn[i], st)[0]])
    S.add("cull_at_tmin", np.array(ties))
    S.items
    return S

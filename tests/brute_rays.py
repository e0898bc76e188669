"""Rays aimed at the guards of the clustered brute-force trace (rt_device.h trace_brute_compact<false, true>: the
shell's face tests, kNearFloor, the one queue step and quad_pick's kQuadBand, kQuadGraze and kQuadDirMax), the small
scenes they are aimed in, and the reference they are judged by.  Plain numpy, no GPU: tests/test_brute_rays.py keeps
the families honest on the host, tests/test_gpu_brute_rays.py puts them through the compiled function
(rt_debug_trace_clustered).

The reference uses no box, shell, floor or line: for every ray it is the minimum, over all records of the scene, of
the key (k bits, record rank) that the trace's run_batch folds with atomicMin -- Moller-Trumbore from
tests/query_ref.py, the trace's acceptance 0.0001f < k < 1000.0f, the triangle read from the winning record.  It
judges every finite ray that no box test decides (judged: `decided`).  The renderer this one reproduces, and so every
engine here, tests a triangle only behind its leaf box, and for a ray through the very edge or corner of a box, or
inside a box's bounding plane (0 * inf), that test and Moller-Trumbore part ways; there the judge is the same minimum
over the records whose own leaf box passes slab() and box_hit() (reference(boxes=True)), which holds on every finite
ray.

Targets, origins and near-wall rays come from the generators of tests/test_brute_quad.py (_plane_points, _towards,
_interior_rays, _boundary_origins) and tests/test_brute_near.py (near_rays, _ulp_step); what is added here is where
they are pointed."""
import functools

import numpy as np

from ensem3a_openclraytracer_amd import _native
from tests import nonfinite_rays as NR
from tests import query_ref as QR
from tests import test_brute_near as N
from tests import test_brute_quad as Q
from tests.test_brute_shell import wall_box

F32 = np.float32
M, G, DMAX, T = Q.M, Q.G, Q.DMAX, N.T
C = N.C                                   # the hit condition's k > 0.0001f
HORIZON = F32(1000.0)
FAMILIES = ("band", "graze", "scale", "floor", "nonfinite")     # ("logged" is built on the GPU, in the test)
N_WALL = 3072                             # rays per face of the box in band and graze (+ 1 in 20); scale 2 x, floor 1.5 x


def _coincident():
    from tests.test_gpu_brute_hitword import coincident
    return coincident()


# name -> (builder, options the scene needs on top of the defaults to be clustered at all)
SCENES = {
    "cornell": (Q.SCENES["cornell"], {}),
    "six_face_room": (Q.SCENES["six_face_room"], {}),
    "reversed_room": (Q.reversed_room, {}),
    "mixed_room": (Q.mixed_room, {}),
    "one_record_room": (Q.one_record_room, {}),
    "thin_room": (N.thin_room, {}),
    "skinny_room": (N.skinny_room, {}),
    "off_plane_room": (N.off_plane_room, {}),
    "one_ulp_room": (Q.SCENES["one_ulp_room"], {}),
    "far_room": (Q.far_room, {}),
    "small_room": (Q.SCENES["small_room"], {}),
    "big_room": (Q.SCENES["big_room"], {}),
    "moved_room": (lambda: Q.moved_room((30000.0, 0.0, 0.0)), {}),
    # three triangles, two boxes: no SAH subtree the automatic rule would cluster, and no wall
    "coincident": (_coincident, {"brute_cluster": 1}),
}


class Case:
    """A scene with what the packer makes of it (host calls only) and its rays."""

    def __init__(self, name):
        build, self.options = SCENES[name]
        self.name = name
        self.sc = sc = build()
        args = N._args(sc)
        cluster = self.options.get("brute_cluster", -1)
        self.shell = _native.brute_shell(*args, cluster)
        self.quad = _native.brute_quad(*args, cluster)
        _, self.floor, _ = _native.brute_near(*args, cluster)
        self.nclusters = len(_native.brute_clusters(*args, cluster)[1])
        self.tri9 = QR.triangles9(sc)
        vp = np.asarray(sc.V_p, F32).reshape(-1, 3)
        # the box the rays are aimed in: the shell's, or the vertices' where there is none
        self.box = (self.shell["box"] if self.shell is not None else
                    np.stack([vp.min(0), vp.max(0)], axis=1).reshape(6)).astype(F32)
        self.present = (self.shell["faces"][:, 0] >= 0) if self.shell is not None else np.zeros(6, bool)
        self.split = self.quad["split"] & self.present
        self.order = record_order(sc)
        self._rays = {}
        self._judged = {}

    def line(self, f):
        """The line of face f: the packer's where the wall is split, else the diagonal of the box's face scaled as
        the packer scales it (sigma = +-1 at the far corners), so that every face gets the same targets."""
        if self.split[f]:
            return self.quad["lines"][f]
        S = self.box.astype(np.float64)
        u, v = [k for k in range(3) if k != f // 2]
        ln = np.zeros(4)
        ln[u], ln[v] = 1.0 / (S[2 * u + 1] - S[2 * u]), -1.0 / (S[2 * v + 1] - S[2 * v])
        ln[3] = -(ln[u] * 0.5 * (S[2 * u] + S[2 * u + 1]) + ln[v] * 0.5 * (S[2 * v] + S[2 * v + 1]))
        return ln.astype(F32)

    def info(self, quad=-1, near=-1, shell=-1):
        """What rt_debug_trace_clustered's info[1..3] must read with these options: the host's own predictions."""
        has = shell != 0 and self.shell is not None
        return [int(has), int(has and near != 0 and self.floor != 0), int(has and quad != 0 and self.quad["nsplit"] > 0)]

    def rays(self, family):
        if family not in self._rays:
            rng = np.random.default_rng(7000 + 13 * list(SCENES).index(self.name) + FAMILIES.index(family))
            r, tag = getattr(Families, family)(self, rng)
            r = np.ascontiguousarray(r, F32)
            if family != "nonfinite":
                # The trace takes its one queue step, and asks quad_pick, only in a wave none of whose lanes passes two
                # faces; one ray from an edge, a corner or outside sends its whole wave through the face-by-face
                # path.  So the rays that pass several faces (as the numpy face test sees them) stand behind the
                # others, in waves of their own; the wave test of tests/test_gpu_brute_rays.py mixes them again
                several = guards(self, r)[0] == -2
                order = np.argsort(several, kind="stable")
                r, tag = np.ascontiguousarray(r[order]), tag[order]
            r.setflags(write=False)
            self._rays[family] = (r, tag)
        return self._rays[family]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---- the reference --------------------------------------------------------------------------------------------------
def record_order(sc):
    """The triangles in record order: the rank of scene_pack.cpp, pre-order over the exported tree with the right
    child first (nodes of 9 floats: left, right, min.xyz, max.xyz, triangle or -1)."""
    nodes = np.asarray(sc.BVH.exportArray, F32).reshape(-1, 9)
    out, stack = [], [0]
    while stack:
        n = stack.pop()
        left, right, t = int(nodes[n, 0]), int(nodes[n, 1]), int(nodes[n, 8])
        if t >= 0:
            out.append(t)
        if left >= 0:
            stack.append(left)
        if right >= 0:
            stack.append(right)
    return np.array(out, np.int64)


NOKEY = (np.uint64(HORIZON.view(np.uint32)) << np.uint64(32)) | np.uint64(0xffffffff)


def leaf_boxes(sc, order):
    """The leaf box of every record, lo.x hi.x lo.y hi.y lo.z hi.z, from the exported tree."""
    nodes = np.asarray(sc.BVH.exportArray, F32).reshape(-1, 9)
    leaf = nodes[nodes[:, 8] >= 0]
    by_tri = np.zeros((int(leaf[:, 8].max()) + 1, 6), F32)
    by_tri[leaf[:, 8].astype(np.int64)] = leaf[:, [2, 5, 3, 6, 4, 7]]
    return by_tri[order]


def reference(c, rays, boxes=False, chunk=8192):
    """(k float32[n] -- 1000 on a miss --, tri int32[n] -- -1 on a miss --, tie bool[n]: another record is accepted at
    the winner's k) for rays [n, 6] in Case c, over every record and nothing else.

    boxes: only the records whose own leaf box the ray passes (slab() and box_hit() with the horizon's cull, as
    tests/nonfinite_rays.py restates them) -- what the reference renderer and every engine here compute, which test a
    triangle only behind its box.  The two differ where the box test and Moller-Trumbore round a ray through an
    edge of a box differently, and where a ray runs inside a box's bounding plane (0 * inf)."""
    rays = np.asarray(rays, F32).reshape(-1, 6)
    tri9 = c.tri9[c.order]
    lb = leaf_boxes(c.sc, c.order) if boxes else None
    k_out, t_out, tie = np.empty(len(rays), F32), np.empty(len(rays), np.int32), np.empty(len(rays), bool)
    rank = np.arange(len(tri9), dtype=np.uint64)
    for b in range(0, len(rays), chunk):
        r = rays[b:b + chunk]
        hit, k, _, _ = QR.mt(tri9[None, :, :], r[:, None, :])
        with np.errstate(all="ignore"):
            acc = hit & (k > C) & (k < HORIZON)
            if boxes:
                acc &= NR.slab_pass(lb, r)
        kb = np.ascontiguousarray(k).view(np.uint32).astype(np.uint64)
        key = np.where(acc, (kb << np.uint64(32)) | rank[None, :], NOKEY)
        best = key.min(axis=1)
        won = best != NOKEY
        k_out[b:b + chunk] = np.where(won, (best >> np.uint64(32)).astype(np.uint32).view(F32), HORIZON)
        t_out[b:b + chunk] = np.where(won, c.order[(best & np.uint64(0xffffffff)).astype(np.int64) % len(tri9)], -1)
        tie[b:b + chunk] = won & ((acc & ((key >> np.uint64(32)) == (best >> np.uint64(32))[:, None])).sum(axis=1) > 1)
    return k_out, t_out, tie


def finite(rays):
    return np.isfinite(rays).all(axis=1)


def judged(c, family_or_rays):
    """The two references of a family's rays (or of rays given), computed once: dict of k, tri, tie (no boxes), kb,
    trib, tieb (behind the leaf boxes), finite, and decided -- finite rays on which the two agree bit for bit.  The
    reference without boxes is what a trace must return on the decided rays; on the others a box test, which that
    reference does not have, decides, and the one behind the leaf boxes is what every engine computes."""
    rays = c.rays(family_or_rays)[0] if isinstance(family_or_rays, str) else np.asarray(family_or_rays, F32)
    key = family_or_rays if isinstance(family_or_rays, str) else None
    if key is not None and key in c._judged:
        return c._judged[key]
    k, tri, tie = reference(c, rays)
    kb, trib, tieb = reference(c, rays, boxes=True)
    fin = finite(rays)
    out = dict(k=k, tri=tri, tie=tie, kb=kb, trib=trib, tieb=tieb, finite=fin,
               decided=fin & (bits(k) == bits(kb)) & (tri == trib))
    if key is not None:
        c._judged[key] = out
    return out


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- where a ray stands against the guards (the numpy restatements of tests/test_brute_quad.py) -----------------------
def guards(c, rays, floor=None):
    """Per ray: the face whose test it passes (-1: none, -2: more than one), and for that face quad_pick's
    conditions one by one -- inside (tin <= 0), ahead (T >= 0), steep (|d_a| >= g max|d|), short (max|d| <=
    kQuadDirMax), out (|sigma~| >= kQuadBand), positive (sigma~ >= 0)."""
    n = len(rays)
    face = np.full(n, -1)
    cond = {k: np.zeros(n, bool) for k in ("inside", "ahead", "steep", "short", "out", "positive")}
    floor = c.floor if floor is None else floor
    for f in range(6):
        ok, mn, mx = Q.face_pass(c.box, f, rays, floor)
        face = np.where(ok, np.where(face == -1, f, -2), face)
        _, sg = Q.quad_pick(c.line(f), f, rays, mn, mx)
        d = rays[:, 0:3]
        with np.errstate(all="ignore"):
            tin = np.fmax(np.fmax(mn[:, 0], mn[:, 1]), mn[:, 2])
            tex = np.fmin(np.fmin(mx[:, 0], mx[:, 1]), mx[:, 2])
            dm = np.fmax(np.fmax(np.abs(d[:, 0]), np.abs(d[:, 1])), np.abs(d[:, 2]))
            vals = dict(inside=tin <= 0, ahead=tex >= 0, steep=np.abs(d[:, f // 2]) >= G * dm, short=dm <= DMAX,
                        out=np.abs(sg) >= M, positive=sg >= 0)
        for k, v in vals.items():
            cond[k] = np.where(ok, v, cond[k])
    for k in cond:
        cond[k] = cond[k] & (face >= 0)
    return face, cond


def clean_waves(face):
    """Per ray: no ray of its wave (64 consecutive rays, as rt_debug_trace_clustered lays them out) passes several
    faces, so the wave takes the one queue step and quad_pick is asked."""
    wave = np.arange(len(face)) // 64
    dirty = np.zeros(int(wave.max()) + 1, bool)
    np.logical_or.at(dirty, wave, face == -2)
    return ~dirty[wave]


def sure(cond, but=None):
    """quad_pick's `sure`; but = a condition's name: every other condition holds and that one does not."""
    names = ("inside", "ahead", "steep", "short", "out")
    out = np.ones(len(cond["inside"]), bool)
    for k in names:
        out &= ~cond[k] if k == but else cond[k]
    return out


# ---- the families ---------------------------------------------------------------------------------------------------
def _interior(S, rng, n):
    return Q._interior_rays(S, rng, n)[:, 3:6].astype(np.float64)


def _back_along(S, P, d, rng, part=(0.05, 0.95)):
    """Origins for rays along d through the points P of the box S: back from P, a random part of the way to where
    the line leaves the box."""
    S, dd = np.asarray(S, np.float64), d.astype(np.float64)
    with np.errstate(all="ignore"):
        room = [np.where(dd[:, k] > 0, (P[:, k] - S[2 * k]) / dd[:, k],
                         np.where(dd[:, k] < 0, (P[:, k] - S[2 * k + 1]) / dd[:, k], np.inf)) for k in range(3)]
    back = np.minimum(np.minimum(room[0], room[1]), room[2]) * rng.uniform(part[0], part[1], len(P))
    return P - back[:, None] * dd


def _origins(c, f, P, rng):
    """Origins for rays aimed at the points P of face f, by turns: interior points (2 of 10), back from the target
    along a direction within 45 degrees of the wall's normal (1: the only rays a wall of a thin room is sure of), a
    point on another wall as a bounce ray has it (2), within 64 ulps of a wall (1), on the box's faces, edges and
    corners (1), one ulp outside the box on one axis (2: tin > 0 and nothing else keeps the lane from being sure),
    ten box widths outside (1)."""
    S = c.box
    n = len(P)
    o = _interior(S, rng, n)
    kind = np.arange(n) % 10
    # (a room so thin along the face's axis that an interior point is almost never within 45 degrees of the target
    # -- the thin room's x walls, 1.5e-4 apart -- gets such origins 7 times in 10, from the far third of the room:
    # nearer ones leave through the wall below the floor, and its test does not pass)
    width = (S[1::2] - S[0::2]).astype(np.float64)
    thin = width[f // 2] * 64 < np.delete(width, f // 2).min()
    steep = (kind < 7) if thin else (kind == 2)
    d = rng.uniform(-1.0, 1.0, (n, 3))
    d[:, f // 2] = 1.0 if f % 2 == 1 else -1.0
    o[steep] = _back_along(S, P[steep], d[steep], rng, (0.7, 0.98) if thin else (0.05, 0.95))
    kind = np.where(steep, 2, kind)
    g = (f + 1 + rng.integers(0, 5, n)) % 6                      # another face
    a = g // 2
    on =(kind == 3) | (kind == 4)
    o[on, a[on]] = S[g[on]]
    near = kind == 5
    for gg in range(6):
        pick = near & (g == gg)
        if pick.any():
            o[pick] = N.near_rays(wall_box(S, gg), rng, int(pick.sum()))[:, 3:6]
    edge = kind == 6
    o[edge] = Q._boundary_origins(S, rng, int(edge.sum()))
    ulp = (kind == 7) | (kind == 8)
    outward = np.where(g % 2 == 0, -1, 1)
    o[ulp, a[ulp]] = N._ulp_step(S[g], outward).astype(np.float64)[ulp]
    far = kind == 9
    o[far, a[far]] = (S[g] + outward * 10.0 * width[a])[far]
    return o.astype(F32)


def _targets(c, f, rng):
    """_plane_points on face f, thinned: of the points at the band's edge every one inside the band and three in five of
    those outside, a third of the unconstrained ones, and one in 24 of those on the line, on an edge and at a
    corner -- a ray through one of these hits two records at one distance, and the share of such ties stays under the
    2 % that tests/test_brute_rays.py allows.  About 1.35 N_WALL points."""
    n = N_WALL * 3
    line = c.line(f)
    P = Q._plane_points(c.box.astype(np.float64), f, line, rng, n)
    kind, turn = np.arange(n) % 8, np.arange(n) // 8
    inside = np.abs(P @ line[:3].astype(np.float64) + float(line[3])) < float(M)
    keep = np.where(kind < 4, inside | (turn % 5 < 3), np.where(kind == 7, turn % 3 == 0, turn % 24 == 0))
    return P[keep]


class Families:
    @staticmethod
    def band(c, rng):
        """Targets at sigma = +-kQuadBand (1 + j 2^-22), on the line, on the edges and at the corners of every face of
        the box (a split wall's own line, else the face's diagonal), from _origins.  tag: the face aimed at."""
        rays, tag = [], []
        for f in range(6):
            P = _targets(c, f, rng)
            r = Q._towards(P, _origins(c, f, P, rng))
            # No ray runs inside the plane of a face it starts on (a target on the edge that two walls share, from
            # the other wall): its slab distances there are 0 * inf, and the box tests, not Moller-Trumbore, decide
            # what it hits -- the reference here has no box.  Such a ray starts from an interior point instead; the
            # nonfinite family has the class (zero_dir_on_bound), compared among the device's forms
            flat = ((r[:, 0:3] == 0) & ((r[:, 3:6] == c.box[0::2]) | (r[:, 3:6] == c.box[1::2]))).any(axis=1)
            r[flat] = Q._towards(P[flat], _interior(c.box, rng, int(flat.sum())).astype(F32))
            rays.append(r)
            tag.append(np.full(len(P), f))
            if c.split[f]:
                # ... and the first of them moved onto the band's edge in float32 (_to_band_edge: pairs of rays one ulp
                # of an origin coordinate apart, |sigma~| >= kQuadBand for one and not for the other) -- far from the
                # origin a target placed in float64 lands anywhere within the coordinates' rounding of the edge
                edge, _ = Q._to_band_edge(c.box, f, c.line(f), r[:N_WALL // 3].copy())
                rays.append(edge)
                tag.append(np.full(len(edge), f))
        return np.concatenate(rays), np.concatenate(tag)

    @staticmethod
    def graze(c, rng):
        """Through the same targets from inside the box, the direction's component along the wall's axis set to
        kQuadGraze max|d| (1 + j 2^-23), j in [-4, 4], after the fact: the origin is moved back along the new
        direction, a random part of the way to where it would leave the box."""
        S = c.box.astype(np.float64)
        rays, tag = [], []
        for f in range(6):
            a = f // 2
            P = _targets(c, f, rng)
            n = len(P)
            d = Q._towards(P, _interior(S, rng, n).astype(F32))[:, 0:3]
            d[:, a] = 0
            dm = np.abs(d).max(axis=1)
            d[dm == 0, (a + 1) % 3] = F32(1.0)
            dm = np.abs(d).max(axis=1).astype(np.float64)
            j = rng.integers(-4, 5, n)
            da = (float(G) * dm * (1.0 + j * 2.0 ** -23)).astype(F32)
            d[:, a] = da if f % 2 == 1 else -da                      # towards the face
            o = _back_along(S, P, d, rng)
            rays.append(np.concatenate([d, o.astype(F32)], axis=1))
            tag.append(np.full(n, f))
        return np.concatenate(rays), np.concatenate(tag)

    @staticmethod
    def scale(c, rng):
        """The band rays twice, their directions multiplied: five in eight so that max|d| = kQuadDirMax (1 + j 2^-23),
        j in [-4, 4] (the largest component is set to that float itself), the others by 2^-20, 3 and 2^20."""
        rays, tag = c.rays("band")
        rays, tag = np.concatenate([rays, rays]), np.concatenate([tag, tag])
        n = len(rays)
        d = rays[:, 0:3].astype(np.float64)
        dm = np.abs(d).max(axis=1)
        kind = np.where(np.arange(n) < n // 2, 0, 4 + rng.permutation(n) % 4)
        j = rng.integers(-4, 5, n)
        want = float(DMAX) * (1.0 + j * 2.0 ** -23)
        with np.errstate(all="ignore"):
            s = np.where(kind < 5, want / dm, np.choose(np.clip(kind - 5, 0, 2), [2.0 ** -20, 3.0, 2.0 ** 20]))
        s = np.where(np.isfinite(s), s, 1.0)
        out = (d * s[:, None]).astype(F32)
        top = np.abs(d).argmax(axis=1)
        fix = (kind < 5) & (dm > 0)
        rows = np.flatnonzero(fix)
        out[rows, top[rows]] = (np.sign(d[rows, top[rows]]) * want[rows]).astype(F32)
        rays[:, 0:3] = out
        return rays, tag

    @staticmethod
    def floor(c, rng):
        """near_rays on every face of the box, by turns: as they are (within 64 ulps of the wall, 2 % parallel to
        it); the direction's normal component set so that the wall's plane lies kNearFloor (1 + j 2^-23) along the
        ray, or 0.0001 (1 + j 2^-23); on the wall itself with a normal component of exactly 0."""
        rays, tag = [], []
        for f in range(6):
            a = f // 2
            n = N_WALL * 3 // 2
            r = N.near_rays(wall_box(c.box, f), rng, n)
            kind = np.arange(n) % 8
            gap = c.box[f].astype(np.float64) - r[:, 3 + a].astype(np.float64)       # exact: the origin is ulps away
            j = rng.integers(-4, 5, n)
            t = np.where(kind < 3, float(T), float(C)) * (1.0 + j * 2.0 ** -23)
            aimed = (kind < 6) & (gap != 0)
            with np.errstate(all="ignore"):
                r[aimed, a] = (gap / t).astype(F32)[aimed]
            flat = kind == 6
            r[flat, 3 + a] = c.box[f]
            r[flat, a] = F32(0.0)
            rays.append(r)
            tag.append(np.full(n, f))
        return np.concatenate(rays), np.concatenate(tag)

    @staticmethod
    def nonfinite(c, rng):
        """tests/nonfinite_rays.py ray_classes from the box's centre and from an interior point: NaN, +-inf, zeros of
        either sign and denormals in the direction, NaN, +-inf and huge values in the origin."""
        nodes = np.asarray(c.sc.BVH.exportArray, F32).reshape(-1, 9)
        leaves = nodes[nodes[:, 8] >= 0][:, 2:8]
        S = c.box.astype(np.float64)
        out = []
        with np.errstate(all="ignore"):
            for seed, o in enumerate((0.5 * (S[0::2] + S[1::2]), _interior(c.box, rng, 1)[0])):
                out += list(NR.ray_classes(o, leaves, seed=100 * seed + len(c.name), per_class=48).values())
        rays = np.concatenate(out).astype(F32)
        return rays, np.full(len(rays), -1)

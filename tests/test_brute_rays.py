"""tests/brute_rays.py on the host alone: its reference is the CPU oracle's trace wherever a ray's hit is unique, and its
families stand where they claim to -- on either side of kQuadBand, kQuadGraze, kQuadDirMax and kNearFloor, per split wall
and per side of its line, as the numpy restatements of tests/test_brute_quad.py (face_pass, quad_pick) see them.  These
are conditions on the inputs of tests/test_gpu_brute_rays.py: a family that misses one is mended, not the bound.

The rooms at 2^-20 and 2^20 are exempt from the counts, as they are in tests/test_brute_quad.py: a unit direction
leaves the small room after 2^-19, below the floor, so no face test passes at all, and crosses the big one in 2^21, past
the horizon's 1000, unless it starts within 1000 of the wall it leaves through.  Their rays are traced all the same."""
import numpy as np
import pytest

import oracle.oracle as O
from ensem3a_openclraytracer_amd import workloads as W
from tests import brute_rays as R
from tests import test_brute_quad as Q

F32 = np.float32
COUNTED = [n for n in R.SCENES if n not in ("small_room", "big_room", "coincident")]
MIN = 200


def _split_faces(c):
    return [int(f) for f in np.flatnonzero(c.split)]


@pytest.mark.parametrize("name", list(R.SCENES))
def test_the_reference_is_the_oracles_trace_where_the_hit_is_unique(name):
    c = R.case(name)
    sc = c.sc
    osc = O.OracleScene.from_scene(sc, W.ibl_preview())
    face = np.asarray(sc.faceData, np.int32).reshape(-1, 10)
    vn = np.asarray(sc.V_n, F32).reshape(-1, 3)
    nodes = np.asarray(sc.BVH.exportArray, F32).reshape(-1, 9)
    parent = np.full(len(nodes), -1)
    for n in range(len(nodes)):
        for ch in nodes[n, 0:2].astype(int):
            if ch >= 0:
                parent[ch] = n
    leaf_of = {int(nodes[n, 8]): n for n in range(len(nodes)) if nodes[n, 8] >= 0}

    def oracle_boxes_reject(t, ray):
        """The oracle walks the exported tree: does its own box test fail on a node from triangle t's leaf up?"""
        n = leaf_of[int(t)]
        while n >= 0:
            if not O.box(ray, nodes[n, 2:8]):
                return True
            n = parent[n]
        return False

    for family in ("band", "floor"):
        rays, _ = c.rays(family)
        assert R.finite(rays).all()
        j = R.judged(c, family)
        k, tri, tie, decided = j["k"], j["tri"], j["tie"], j["decided"]
        want = np.stack([O.trace(osc, r) for r in rays])
        ok = ~tie & decided
        hit = tri >= 0
        same = ((want[:, 5] == 1) == hit) & (~hit | (R.bits(want[:, 3]) == R.bits(k)))
        # the oracle names its triangle by the first vertex's normal and the material
        same &= ~hit | ((R.bits(want[:, 0:3]) == R.bits(vn[face[np.maximum(tri, 0), 4]])).all(axis=1) &
                        (want[:, 4] == face[np.maximum(tri, 0), 0]))
        # What is left: the oracle's box test (the reference renderer's, which divides where the kernels multiply by a
        # reciprocal) fails on the winner's own path where the kernels' passes -- a ray through the very edge of a box.
        # Then the oracle sees a farther hit or none
        other = np.flatnonzero(ok & ~same)
        for i in other:
            assert hit[i] and oracle_boxes_reject(tri[i], rays[i]), (name, family, rays[i].tolist(), k[i], tri[i], want[i].tolist())
            assert want[i, 5] == 0 or want[i, 3] >= k[i], (name, family, i)
        print("%s %s: %d rays, %d hits, ties %.2f %%, decided by a box test %.2f %%, the oracle's box test differs %.2f %%" % (
            name, family, len(rays), hit.sum(), 100.0 * tie.mean(), 100.0 * (~decided).mean(), 100.0 * len(other) / len(rays)))
        if name != "coincident":
            assert tie.mean() <= 0.02, (name, family, tie.mean())
        # the rays a box test decides: in `floor` one ray in eight lies in its wall's plane and 2 % of the others are
        # parallel to it; in `band` only rays through an edge or a corner of a box
        assert (~decided).mean() <= (0.16 if family == "floor" else 0.01), (name, family)
        assert len(other) <= 0.005 * len(rays), (name, family, len(other))
        assert name == "small_room" or (ok & same & hit).sum() >= 500, (name, family)


def _per_side(face, cond, f):
    for side in (True, False):
        yield side, (face == f) & (cond["positive"] == side)


@pytest.mark.parametrize("name", COUNTED)
def test_band_rays_stand_on_both_sides_of_the_band_on_every_split_wall(name):
    c = R.case(name)
    rays, _ = c.rays("band")
    face, cond = R.guards(c, rays)
    # (only rays that the reference judges and whose wave takes the one queue step are counted)
    dec = R.judged(c, "band")["decided"] & R.clean_waves(face)
    sure, inside_band, only_tin = R.sure(cond) & dec, R.sure(cond, "out") & dec, R.sure(cond, "inside") & dec
    print("%s band: %d rays, one face %.1f %%, several %.1f %%, sure %.1f %%, in the band %.1f %%, tin > 0 alone %.1f %%" % (
        name, len(rays), 100.0 * (face >= 0).mean(), 100.0 * (face == -2).mean(), 100.0 * sure.mean(),
        100.0 * inside_band.mean(), 100.0 * only_tin.mean()))
    for f in _split_faces(c):
        for side, m in _per_side(face, cond, f):
            assert (sure & m).sum() >= MIN and (inside_band & m).sum() >= MIN, (name, f, side, (sure & m).sum(), (inside_band & m).sum())
    # (the skinny room's shell has no floor: a ray from outside passes the face it enters through as well as the one it
    # leaves through, so its faces are queued one by one and quad_pick is not asked)
    assert only_tin.sum() >= (0 if name == "skinny_room" else 100), (name, only_tin.sum())
    assert (face == -2).sum() >= 100                      # ... and the faces are queued one by one for some


@pytest.mark.parametrize("name", COUNTED)
@pytest.mark.parametrize("family,guard", [("graze", "steep"), ("scale", "short")])
def test_graze_and_scale_rays_stand_on_both_sides_of_their_guard(name, family, guard):
    c = R.case(name)
    rays, _ = c.rays(family)
    face, cond = R.guards(c, rays)
    dec = R.judged(c, family)["decided"] & R.clean_waves(face)
    sure, beyond = R.sure(cond) & dec, R.sure(cond, guard) & dec
    print("%s %s: %d rays, one face %.1f %%, sure %.1f %%, not sure for the guard alone %.1f %%" % (
        name, family, len(rays), 100.0 * (face >= 0).mean(), 100.0 * sure.mean(), 100.0 * beyond.mean()))
    for f in _split_faces(c):
        for side, m in _per_side(face, cond, f):
            # (the thin room's x walls are 1.5e-4 apart: a ray with max|d| = 2 leaves through one within 0.75e-4, under
            # the floor, so its test never passes: no ray there stands at this guard, on either side)
            if (name, family, f // 2) == ("thin_room", "scale", 0):
                continue
            assert (sure & m).sum() >= MIN and (beyond & m).sum() >= MIN, (name, family, f, side, (sure & m).sum(), (beyond & m).sum())


@pytest.mark.parametrize("name", [n for n in COUNTED if n != "skinny_room"])
def test_floor_rays_stand_on_both_sides_of_the_floor_on_every_face(name):
    c = R.case(name)
    rays, _ = c.rays("floor")
    assert c.floor == R.T and R.case("skinny_room").floor == 0          # (the one shell without a floor)
    dec = R.judged(c, "floor")["decided"]
    for f in np.flatnonzero(c.present):
        at0, _, mx = Q.face_pass(c.box, f, rays, 0.0)
        atT, _, _ = Q.face_pass(c.box, f, rays, R.T)
        with np.errstate(all="ignore"):
            tx = np.fmin(np.fmin(mx[:, 0], mx[:, 1]), mx[:, 2])
            dropped = at0 & ~atT & dec
            kept = atT & (tx <= R.T * F32(1.0 + 2.0 ** -20)) & dec
            at_hit = atT & (np.abs(tx / R.C - F32(1.0)) <= F32(2.0 ** -20)) & dec
        assert not (atT & ~at0).any()
        assert dropped.sum() >= MIN and kept.sum() >= MIN and at_hit.sum() >= MIN, (name, f, dropped.sum(), kept.sum(), at_hit.sum())
    at0, _ = R.guards(c, rays, 0.0)
    atT, _ = R.guards(c, rays)
    print("%s floor: %d rays, one face at the floor %.1f %%, at 0 %.1f %%, several %.1f %%" % (
        name, len(rays), 100.0 * (atT >= 0).mean(), 100.0 * (at0 >= 0).mean(), 100.0 * (atT == -2).mean()))


def test_nonfinite_rays_have_every_class_and_the_reference_reads_them():
    c = R.case("six_face_room")
    rays, _ = c.rays("nonfinite")
    assert np.isnan(rays).any(axis=1).sum() >= 300 and np.isinf(rays).any(axis=1).sum() >= 100
    assert (np.signbit(rays) & (rays == 0)).any() and R.finite(rays).sum() >= 300
    k, tri, _ = R.reference(c, rays)
    assert ((tri >= 0) == (k < R.HORIZON)).all() and (tri[~R.finite(rays)] >= -1).all()


def test_record_order_is_the_packers():
    """The rank restated in record_order against the records the packer lists for the shell's faces."""
    c = R.case("mixed_room")
    for f in range(6):
        for t in range(2):
            rec = c.shell["faces"][f, t]
            p0, e1, e2 = c.quad["recs"][f, t]
            tri = c.tri9[c.order[rec]].reshape(3, 3)
            assert (tri[0] == p0).all() and (tri[1] - tri[0] == e1).all() and (tri[2] - tri[0] == e2).all(), (f, t)

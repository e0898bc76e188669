"""The clustered form of the brute-force boxes (rt_debug_brute_clusters, option "brute_cluster"; scene_pack.cpp
build_clusters, rt_device.h trace_brute_compact), on the host alone: the table partitions the real slots of
rt_debug_brute_layout's array, every index the kernel forms from it is in range, and a ray that passes a
member box passes its cluster's union -- for the non-finite ray classes too -- so the union test skips nothing
the lock-step loop would have queued."""
import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from tests import nonfinite_rays as NR
from tests.test_malformed_inputs import BRUTE_SCENES, _brute_scene

SLOTS = 8            # rt_layout.h kClusterSlots
LOCK_NUM = 4         # rt_layout.h kClusterLockNum: more than LOCK_NUM / 8 of the tracing lanes -> lock-step
# the soups the GPU test renders with brute_cluster = 1 (tests/test_gpu_brute_cluster.py)
GPU_SOUPS = [(9, 33), (11, 23), (5, 50)]
MODES = {"auto": -1, "force": 1}


def _args(sc):
    return sc.V_p, sc.V_n, sc.faceData, sc.materialData, sc.BVH.exportArray


def _tables(which, mode):
    sc = _brute_scene(which)
    base, nbox, nbrute = _native.brute_layout(*_args(sc))
    slots, rows, nsingle = _native.brute_clusters(*_args(sc), MODES[mode])
    return sc, base, nbox, nbrute, slots, rows, nsingle


def _row_ints(rows):
    ints = rows[:, 6:8].copy().view(np.int32)
    return ints[:, 0], ints[:, 1]


def _key(slot):
    return slot.tobytes()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", BRUTE_SCENES + GPU_SOUPS, ids=str)
def test_cluster_table_partitions_the_real_slots(which, mode):
    sc, base, nbox, nbrute, slots, rows, nsingle = _tables(which, mode)
    if len(rows) == 0:                      # not clustered: both arrays empty, the kernel keeps brute_box
        assert len(slots) == 0 and nsingle == 0
        return
    first, count = _row_ints(rows)
    ns4 = -(-nsingle // 4) * 4
    assert len(slots) == ns4 + SLOTS * len(rows)
    # counts and first slots in range: clusters follow the padded singles, SLOTS slots each
    assert ((count >= 2) & (count <= SLOTS)).all(), count
    assert first.tolist() == [ns4 + SLOTS * c for c in range(len(rows))]
    real = np.zeros(len(slots), bool)
    real[:nsingle] = True
    for f, n in zip(first, count):
        real[f:f + n] = True
    # every real slot of brute_box is in exactly one cluster or is single, bit for bit
    assert sorted(_key(s) for s in slots[real]) == sorted(_key(s) for s in base[:nbox])
    assert nsingle + count.sum() == nbox
    # padding: the point at 1e30 listing record 0 alone; every slot lists valid records
    ids = slots[:, 6:8].copy().view(np.int32)
    assert (slots[~real, :6] == np.float32(1e30)).all() and (ids[~real, 0] == 0).all() and (ids[~real, 1] == -1).all()
    assert ((ids[:, 0] >= 0) & (ids[:, 0] < nbrute)).all()
    assert ((ids[:, 1] == -1) | ((ids[:, 1] >= 0) & (ids[:, 1] < nbrute))).all()
    # an owner-list entry keeps the first slot above bit 8 of a 32-bit word; the LDS copy holds every slot
    assert len(slots) < (1 << 24)
    # each union contains its members: the componentwise min / max, bitwise one of the members' bounds
    for r, f, n in zip(rows, first, count):
        mem = slots[f:f + n, :6]
        assert np.isfinite(mem).all()
        want = np.where(np.arange(6) % 2 == 1, mem.max(0), mem.min(0)).astype(np.float32)
        out = np.where(np.arange(6) % 2 == 1, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        # ... or one ulp outside it (where a member is flat on the axis at that bound, build_clusters)
        assert ((r[:6] == want) | (r[:6] == np.nextafter(want, out))).all(), (r[:6], want)
        assert (r[0:6:2] <= mem[:, 0::2]).all() and (r[1:6:2] >= mem[:, 1::2]).all()


def test_cornell_auto_clusters_the_two_blocks():
    sc, base, nbox, nbrute, slots, rows, nsingle = _tables("cornell", "auto")
    first, count = _row_ints(rows)
    assert nbox == 22 and nsingle == 6 and count.tolist() == [8, 8] and len(slots) == 24
    # the singles are the five walls and the light: each spans the room in two axes, or is the light's quad
    room = base[:nbox, :6]
    ext = room[:, 1::2] - room[:, 0::2]
    full = (ext >= 0.99 * ext.max(0)).sum(1)
    single_ext = slots[:nsingle, 1:6:2] - slots[:nsingle, 0:6:2]
    assert ((single_ext >= 0.99 * ext.max(0)).sum(1) >= 2).sum() == 5
    assert (full >= 2).sum() == 5
    # the clusters' unions are well inside the room
    uext = rows[:, 1:6:2] - rows[:, 0:6:2]
    assert (uext[:, :2] < 0.5 * ext.max(0)[:2]).all()


def test_off_and_unknown_modes():
    sc = _brute_scene("cornell")
    slots, rows, nsingle = _native.brute_clusters(*_args(sc), 0)
    assert len(slots) == 0 and len(rows) == 0 and nsingle == 0
    with pytest.raises(_native.NativeError):
        _native.brute_clusters(*_args(sc), 2)
    from tests.test_gpu_parity import _random_scene
    big = _random_scene(8, 65)              # the tree walk renders it: nothing to cluster
    slots, rows, nsingle = _native.brute_clusters(*_args(big), 1)
    assert len(slots) == 0 and len(rows) == 0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", BRUTE_SCENES + GPU_SOUPS, ids=str)
def test_passing_member_implies_passing_union(which, mode):
    """slab() + box_hit() in numpy (tests/nonfinite_rays.py) over every ray class: wherever a member slot
    passes, its cluster's union passes, at the cull of a ray with no hit and at a near one; NaN rays pass every
    union (their wave takes the lock-step branch: every tracing lane passes, above any threshold)."""
    sc, base, nbox, nbrute, slots, rows, nsingle = _tables(which, mode)
    if len(rows) == 0:
        return
    first, count = _row_ints(rows)
    leaf = sc.BVH.exportArray.reshape(-1, 9)
    leaf = leaf[leaf[:, 8] >= 0][:, 2:8]
    classes = NR.ray_classes([0.0, -3.5, 0.0], leaf, seed=2)
    rng = np.random.default_rng(5)
    lo, hi = leaf[:, :3].min(0), leaf[:, 3:].max(0)
    inside = np.concatenate([NR.unit_dirs(rng, 512), rng.uniform(lo, hi, (512, 3)).astype(np.float32)], axis=1)
    classes["inside_scene"] = inside.astype(np.float32)
    for cull in (NR.CULL, np.float32(0.75)):
        for name, rays in classes.items():
            u = NR.slab_pass(rows[:, :6], rays, cull)              # (rays, clusters)
            m = NR.slab_pass(slots[:, :6], rays, cull)             # (rays, slots)
            for c, (f, n) in enumerate(zip(first, count)):
                # the whole group of SLOTS slots, padding included: a passing padding slot queues record 0
                # only where the union passed too, or not at all -- either is the lock-step result
                bad = m[:, f:f + n].any(1) & ~u[:, c]
                assert not bad.any(), (name, c, rays[bad][:3])
            if name in ("nan_all", "nan_origin_all", "nan_dir_all"):
                assert u.all(), name


def _soup_camera_rays():
    """The primary rays of the GPU test's soup camera (tests/test_gpu_nonfinite.py SOUP_CAM: 32 x 32 pixels from
    (0, -3.5, 0), 25 degrees, turned 16 and 12 degrees about x and y), to float rounding: a wave holds 64
    consecutive pixels, two rows."""
    f = 1.0 / (2.0 * np.tan(0.5 * 25.0 * 3.14 / 180))
    i = np.arange(32 * 32)
    py, px = (i + 1) % 32, (i - (i + 1) % 32) // 32
    d = np.stack([py / 32.0 - 0.5, np.full(i.size, f), 0.5 - px / 32.0], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ax, ay = 16.0 * 3.14 / 180, 12.0 * 3.14 / 180
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    d = d @ rx.T @ ry.T
    return np.concatenate([d, np.tile([0.0, -3.5, 0.0], (i.size, 1))], axis=1).astype(np.float32)


@pytest.mark.parametrize("which", GPU_SOUPS, ids=str)
def test_gpu_soups_reach_both_branches(which):
    """The soups of the GPU test, forced: cluster sizes that are no multiple of 8 (padding slots inside the
    item index), and -- over simulated waves of 64 primary or bounce rays -- clusters whose union some but
    at most LOCK_NUM / 8 of the lanes pass (compacted items) and clusters that more pass (lock-step)."""
    sc, base, nbox, nbrute, slots, rows, nsingle = _tables(which, "force")
    first, count = _row_ints(rows)
    assert len(rows) >= 2 and (count % SLOTS != 0).any(), count
    assert nbrute <= 64
    leaf = sc.BVH.exportArray.reshape(-1, 9)
    leaf = leaf[leaf[:, 8] >= 0][:, 2:8]
    # primary rays (coherent: whole waves inside a union) and bounce-like rays from random points of the scene
    rng = np.random.default_rng(9)
    lo, hi = leaf[:, :3].min(0), leaf[:, 3:].max(0)
    bounce = np.concatenate([NR.unit_dirs(rng, 64 * 32), rng.uniform(lo, hi, (64 * 32, 3)).astype(np.float32)], axis=1)
    rays = np.concatenate([_soup_camera_rays(), bounce.astype(np.float32)])
    u = NR.slab_pass(rows[:, :6], rays).reshape(-1, 64, len(rows)).sum(1)   # (waves, clusters)
    lock = 64 * LOCK_NUM // 8
    assert ((u > 0) & (u <= lock)).any() and (u > lock).any(), (u.min(), u.max())

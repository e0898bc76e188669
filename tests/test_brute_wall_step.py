"""The shell's one queue step (rt_device.h trace_brute_compact, the block under `if (S.shell)`): when no lane of the
wave passes two of the six face tests, the passes of all faces are queued in one step; otherwise face by face.

What the step rests on, checked here on the CPU with the float32 face test of tests/test_brute_near.py
(slab_pass_floor: slab()'s nests and box_hit() with the shell's floor):
  * a ray that starts on a wall or inside the room passes at most one face, so waves of such rays take the one step;
  * a ray from outside the room, or one with a non-finite component, can pass two or more: those waves queue face
    by face (tests/test_gpu_brute_wall_step.py renders both kinds);
and a model of the step itself: the (owner, record) pairs it writes into the ring are those of the per-face steps,
each once, within the ring's bound."""
import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from tests.test_brute_near import _ulp_step, slab_pass_floor
from tests.test_brute_shell import UNIT, wall_box

F32 = np.float32
T = _native.NEAR_FLOOR
N = 200_000
FACES = [wall_box(UNIT, f) for f in range(6)]


def _passes(rays):
    """(n, 6) bool: the face tests of the unit room's six faces with the floor, nothing found yet (cull at 1000)."""
    return np.stack([slab_pass_floor(b, rays, T)[0] for b in FACES], axis=1)


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def _wall_rays(f, rng, n):
    """n rays that leave face f of the unit room into it: origins on the face, its plane coordinate moved by -1, 0 or
    1 ulp (a hit point is a rounded o + k d), the direction's inward component U(0.001, 1)."""
    a, u, v = f // 2, (f // 2 + 1) % 3, (f // 2 + 2) % 3
    o = np.zeros((n, 3), F32)
    o[:, u], o[:, v] = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    o[:, a] = _ulp_step(np.full(n, UNIT[f], F32), rng.integers(-1, 2, n))
    c = rng.uniform(0.001, 1.0, n) * (1.0 if f % 2 == 0 else -1.0)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - c * c)
    d = np.zeros((n, 3), F32)
    d[:, a], d[:, u], d[:, v] = c, s * np.cos(phi), s * np.sin(phi)
    return np.concatenate([d, o], axis=1).astype(F32)


def test_rays_from_the_walls_and_from_inside_pass_at_most_one_face():
    rng = np.random.default_rng(18)
    counts = np.zeros(7, np.int64)
    for f in range(6):
        rays = _wall_rays(f, rng, N // 6)
        for scale in (F32(1.0), F32(np.sqrt(3.0))):      # unit directions and the sun vector's length
            r = rays.copy()
            r[:, 0:3] *= scale
            counts += np.bincount(_passes(r).sum(axis=1), minlength=7)
    inside = np.concatenate([_unit(rng, N), rng.uniform(-0.999, 0.999, (N, 3)).astype(F32)], axis=1)
    counts += np.bincount(_passes(inside).sum(axis=1), minlength=7)
    total = counts.sum()
    print("faces passed 0..6:", counts.tolist())
    # one face: the one the ray leaves through (the face it starts on is under the floor); two: only through an
    # edge of the room within the rounding of the two plane distances, or from an ulp outside at a grazing angle
    assert counts[1] >= 0.99 * total and counts[2:].sum() <= 1e-3 * total


def test_rays_from_outside_and_non_finite_rays_pass_several_faces():
    rng = np.random.default_rng(19)
    o = np.tile(np.array([0.0, -3.5, 0.0], F32), (N, 1))          # the bench camera: in front of the room
    aim = rng.uniform(-0.9, 0.9, (N, 3)).astype(F32)
    d = aim - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    two = _passes(np.concatenate([d, o], axis=1)).sum(axis=1)
    assert (two == 2).mean() > 0.99                                # in through one face, out through another
    nan_o = np.concatenate([_unit(rng, 1000), np.full((1000, 3), np.nan, F32)], axis=1)
    nan_o[:, 4:6] = rng.uniform(-0.5, 0.5, (1000, 2)).astype(F32)   # origin (NaN, y, z): the x planes drop out
    assert (_passes(nan_o).sum(axis=1) >= 2).any()


def _per_face(passes, q, nact):
    """The per-face steps' ring contents for one wave: passes (lanes, 6), q (6, 2) records (-1: none)."""
    ring = []
    for f in range(6):
        if q[f, 0] < 0:
            continue
        lanes = np.flatnonzero(passes[:, f])
        ring += [(int(l), int(q[f, 0])) for l in lanes]
        if q[f, 1] >= 0:
            ring += [(int(l), int(q[f, 1])) for l in lanes]
    return ring


def _merged(passes, q, tail=0, size=256):
    """The one step: packed words, the select chain, the two ranks; returns the ring's new entries in ring order."""
    pk = np.full(len(passes), 0xffffffff, np.uint64)
    w = (q[:, 0].astype(np.int64) & 0xffffffff) | ((q[:, 1].astype(np.int64) << 16) & 0xffffffff)
    for f in range(6):
        pk = np.where(passes[:, f], np.uint64(w[f]), pk)
    p1, p2 = pk != 0xffffffff, pk < 0xffff0000
    ring = {}
    r1 = tail + np.cumsum(p1) - p1
    r2 = tail + p1.sum() + np.cumsum(p2) - p2
    for l in np.flatnonzero(p1):
        assert int(r1[l]) % size not in ring
        ring[int(r1[l]) % size] = (int(l), int(pk[l]) & 0xffff)
    for l in np.flatnonzero(p2):
        assert int(r2[l]) % size not in ring
        ring[int(r2[l]) % size] = (int(l), int(pk[l]) >> 16)
    n = int(p1.sum() + p2.sum())
    assert sorted(ring) == sorted((tail + i) % size for i in range(n))      # dense behind the tail
    return [ring[(tail + i) % size] for i in range(n)]


@pytest.mark.parametrize("q", [
    [[3, 4], [5, 6], [-1, -1], [7, 8], [0, 1], [9, 10]],        # Cornell's form: the front is open
    [[3, -1], [5, 6], [2, -1], [7, 8], [0, 1], [9, -1]],        # faces of one record
    [[-1, -1]] * 6])
def test_the_one_step_queues_the_pairs_of_the_per_face_steps(q):
    rng = np.random.default_rng(20)
    q = np.array(q, np.int64)
    for trial in range(200):
        lanes = int(rng.integers(1, 65))
        face = rng.integers(-1, 6, lanes)                          # each lane passes one face or none
        passes = face[:, None] == np.arange(6)[None, :]
        tail = int(rng.integers(0, 1 << 20))
        got = _merged(passes, q, tail)
        assert sorted(got) == sorted(_per_face(passes, q, lanes))
        assert len(got) <= 2 * lanes                               # the ring's bound: at most two per lane

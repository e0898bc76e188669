"""The reference of the ray-query tests: Moller-Trumbore exactly as rt_device.h mt_test evaluates it, in float32
numpy, operation by operation (rtm.h: rtm_dot is fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), rtm_cross is
fma(a.y, b.z, -(a.z * b.y)) per component; the build has no contraction, so every other operation rounds once).

tests/test_query_api.py checks the restatement against oracle.intersect (hit flag and the bits of k on every pair of
Cornell's triangles with seeded rays); that licenses its u, v as the expected barycentrics of a query's rt_hit, which
the oracle does not return.
"""
import numpy as np

F32 = np.float32
EPS = F32(0.0000001)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to
    odd there (TwoSum's error term says which neighbour), and 53 bits rounded to odd round correctly to 24."""
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        ok = np.isfinite(s) & np.isfinite(err) & (err != 0)
        bits = np.ascontiguousarray(s).view(np.int64)
        toward = np.where((err > 0) == (s > 0), 1, -1)
        bits = np.where(ok & ((bits & 1) == 0), bits + toward, bits)
        return bits.view(np.float64).astype(F32)


def dot(a, b):
    with np.errstate(all="ignore"):
        return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def cross(a, b):
    with np.errstate(all="ignore"):
        return np.stack([fma32(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])),
                         fma32(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                         fma32(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], axis=-1)


def mt(tri9, ray6):
    """mt_test on broadcastable float32 arrays tri9 [..., 9] (a.p, b.p, c.p) and ray6 [..., 6] (dir, origin).
    Returns (hit, k, u, v); k, u, v are the values computed, whatever the flag."""
    t = np.asarray(tri9, F32)
    r = np.asarray(ray6, F32)
    shape = np.broadcast_shapes(t.shape[:-1], r.shape[:-1])
    t, r = np.broadcast_to(t, shape + (9,)), np.broadcast_to(r, shape + (6,))
    p0 = t[..., 0:3]
    d, o = r[..., 0:3], r[..., 3:6]
    with np.errstate(all="ignore"):
        e1 = t[..., 3:6] - p0
        e2 = t[..., 6:9] - p0
        h = cross(d, e2)
        a = dot(e1, h)
        f = F32(1.0) / a
        s = o - p0
        u = f * dot(s, h)
        q = cross(s, e1)
        v = f * dot(d, q)
        k = f * dot(e2, q)
        miss = ((a > -EPS) & (a < EPS)) | (u < 0) | (u > 1) | (v < 0) | (u + v > 1) | ~(k > EPS)
    return ~miss, k.astype(F32), u.astype(F32), v.astype(F32)


def triangles9(sc):
    """[T, 9] float32: the three vertex positions of every row of faceData."""
    vp = np.asarray(sc.V_p, F32).reshape(-1, 3)
    f = np.asarray(sc.faceData, np.int32).reshape(-1, 10)
    return np.concatenate([vp[f[:, 7]], vp[f[:, 8]], vp[f[:, 9]]], axis=1)

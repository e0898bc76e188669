"""The numpy restatement of lens_ray(cam, lens, i, s) (include/rt_api.h, "Lens frames"): the uniforms exactly, in
uint32 arithmetic, and the ray in float64 (or any dtype: the float32 evaluation is the yardstick the tests' tolerance
was measured against).  Vectorised over pixels ``i`` and sample indices ``s`` of one shape.
"""
import numpy as np

RAD = np.float32(3.14) / np.float32(180.0)   # the reference's degrees to radians, the fp32 constant


def h(x):
    """The uniforms' hash, modulo 2^32."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xffffffff)
    m = np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def uniforms(seed, i, s):
    """u_0 .. u_3 of pixel ``i``, sample ``s``: float32 ``[..., 4]``, each in [0, 1), exact."""
    i, s = np.broadcast_arrays(np.asarray(i, np.int64), np.asarray(s, np.int64))
    hs = h(np.uint32(int(seed) & 0xffffffff))
    base = (h(hs ^ (i & 0xffffffff).astype(np.uint32)).astype(np.uint64) + 4 * (s.astype(np.uint64) & 0xffffffff))
    k = np.arange(4, dtype=np.uint64)
    bits = h((base[..., None] + k) & np.uint64(0xffffffff)) >> np.uint32(8)
    u = bits.astype(np.float32) * np.float32(2.0 ** -24)
    assert ((u >= 0) & (u < 1)).all()
    return u


def _rotate(angle, axis, v):
    """Rodrigues' rotation of the rows of ``v`` about the unit ``axis`` (rotateVec's q v q^-1)."""
    c, s = np.cos(angle), np.sin(angle)
    a = np.asarray(axis, v.dtype)
    return v * c + np.cross(a, v) * s + a * (v @ a)[..., None] * (1 - c)


def rotate_cam(cam, v):
    """genCameraRay's three rotations, about x by cam[3], y by cam[4], z by cam[5] (degrees), in that order."""
    dt = v.dtype
    for ang, axis in ((cam[3], (1, 0, 0)), (cam[4], (0, 1, 0)), (cam[5], (0, 0, 1))):
        v = _rotate(dt.type(np.float32(ang) * RAD), axis, v)
    return v


def focal_distance(cam, dtype=np.float64):
    return dtype(1.0) / (dtype(2.0) * np.tan(dtype(np.float32(cam[9])) / dtype(2.0)))


def lens_ray(cam, jitter, aperture, focus, seed, i, s, dtype=np.float64):
    """``(origin [..., 3], direction [..., 3])`` in ``dtype``, evaluated in the order rt_api.h writes."""
    cam = np.asarray(cam, np.float32)
    f = dtype
    i, s = np.broadcast_arrays(np.asarray(i, np.int64), np.asarray(s, np.int64))
    u = uniforms(seed, i, s).astype(f)
    W = int(cam[6])
    pixelY = (i + 1) % W
    q = i - pixelY
    pixelX = np.sign(q) * (np.abs(q) // W)   # C's division: towards zero (pixel 0 has q = -1)
    pas = f(1.0) / f(cam[6])
    position = np.array([cam[0], cam[1], cam[2]], f)
    focal = np.array([cam[0], f(cam[1]) - focal_distance(cam, f), cam[2]], f)
    jx = (u[..., 0] - f(0.5)) * f(np.float32(jitter))
    jy = (u[..., 1] - f(0.5)) * f(np.float32(jitter))
    pc = np.stack([(pixelY.astype(f) + jx) * pas - f(0.5), np.zeros(i.shape, f),
                   -(pixelX.astype(f) + jy) * pas + f(0.5)], -1)
    d = (position + pc) - focal
    d = d / np.linalg.norm(d, axis=-1, keepdims=True).astype(f)
    if np.float32(aperture) == 0:
        return np.broadcast_to(position, d.shape).copy(), rotate_cam(cam, d)
    r = np.sqrt(u[..., 2]) * f(np.float32(aperture))
    ang = f(np.float32(6.2831855)) * u[..., 3]
    lens = np.stack([r * np.cos(ang), np.zeros(i.shape, f), r * np.sin(ang)], -1).astype(f)
    t = f(np.float32(focus)) / d[..., 1]
    d = d * t[..., None] - lens
    d = d / np.linalg.norm(d, axis=-1, keepdims=True).astype(f)
    return position + rotate_cam(cam, lens), rotate_cam(cam, d)


def focus_point(cam, focus, i):
    """The point of the plane in focus that pixel ``i`` sees through the lens's centre (``jitter = 0``), float64."""
    _, d = lens_ray(cam, 0.0, 0.0, 1.0, 0, i, 0)
    axis = rotate_cam(cam, np.array([[0.0, 1.0, 0.0]]))[0]
    position = np.asarray(cam, np.float32)[:3].astype(np.float64)
    return position + d * (np.float64(np.float32(focus)) / (d @ axis))[..., None], axis

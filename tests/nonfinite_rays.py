"""Rays the kernels' box tests do not handle like ordinary ones: NaN, infinite, zero and denormal
components, far-away origins.  Shared by the host-only layout tests (test_malformed_inputs.py) and
the GPU tests (test_gpu_nonfinite.py).

slab() and box_hit() of rt_device.h use fminf / fmaxf, which return the other operand when one is NaN:
an axis whose two slab distances are NaN drops out of the test, and a ray whose every distance is NaN
passes every box (box_hit(NaN, NaN, cull) is 0 <= cull).  ``slab_pass`` restates them in numpy.
"""
import numpy as np

CULL = np.float32(1000.0) * (np.float32(1.0) + np.float32(2.0 ** -12))   # best.k * CULL_MARGIN with no hit yet


def slab_pass(boxes, rays, cull=CULL):
    """rt_device.h slab() + box_hit() in float32 numpy.  boxes: (B, 6) lo.x hi.x lo.y hi.y lo.z hi.z
    (the brute_box slot order); rays: (R, 6) dir.xyz, origin.xyz.  Returns bool (R, B)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 6)
    r = np.asarray(rays, np.float32).reshape(-1, 6)
    with np.errstate(all="ignore"):
        inv = (np.float32(1.0) / r[:, 0:3])[:, None, :]                # (R, 1, 3)
        o = r[:, None, 3:6]
        t0 = (b[None, :, 0::2] - o) * inv                              # (R, B, 3)
        t1 = (b[None, :, 1::2] - o) * inv
        near, far = np.fmin(t0, t1), np.fmax(t0, t1)
        tmin = np.fmax(np.fmax(near[..., 0], near[..., 1]), near[..., 2])
        tmax = np.fmin(np.fmin(far[..., 0], far[..., 1]), far[..., 2])
        return np.fmax(tmin, np.float32(0.0)) <= np.fmin(tmax, np.float32(cull))


def unit_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def ray_classes(origin, leaf_boxes, seed=0, per_class=6):
    """{class name: (n, 6) float32 rays (dir.xyz, origin.xyz)}.  origin: where valid camera rays of the
    scene start; leaf_boxes: (L, 6) lo.xyz hi.xyz of the scene's leaves (BVH export columns 2..7), used by
    the zero-direction classes, whose origins lie on a leaf box's bound along the zero axis (0 * inf)."""
    rng = np.random.default_rng(4000 + seed)
    o = np.asarray(origin, np.float32)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    lb = np.asarray(leaf_boxes, np.float32).reshape(-1, 6)
    out = {}

    def rays(d, og):
        d = np.asarray(d, np.float32).reshape(-1, 3)
        og = np.broadcast_to(np.asarray(og, np.float32), d.shape)
        return np.concatenate([d, og], axis=1).astype(np.float32)

    def per_axis(name, make, vals=(nan,)):
        rows = []
        for a in range(3):
            for v in vals:
                d = unit_dirs(rng, max(1, per_class // 3))
                og = np.tile(o, (len(d), 1))
                make(d, og, a, v)
                rows.append(rays(d, og))
        out[name] = np.concatenate(rows)

    # ordinary rays, towards leaf centres (so that some hit)
    pick = lb[rng.integers(len(lb), size=per_class)]
    tgt = 0.5 * (pick[:, :3] + pick[:, 3:])
    aim = np.where(np.isfinite(tgt - o).all(1, keepdims=True), tgt - o, unit_dirs(rng, per_class)).astype(np.float64)
    aim[np.linalg.norm(aim, axis=1) == 0] = [0.0, 1.0, 0.0]
    out["finite"] = rays((aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(np.float32), o)
    out["nan_all"] = rays(np.full((per_class, 3), nan), np.full(3, nan))
    out["nan_origin_all"] = rays(unit_dirs(rng, per_class), np.full(3, nan))
    out["nan_dir_all"] = rays(np.full((per_class, 3), nan), o)
    per_axis("nan_origin_1", lambda d, og, a, v: og.__setitem__((slice(None), a), v))
    per_axis("nan_dir_1", lambda d, og, a, v: d.__setitem__((slice(None), a), v))
    per_axis("inf_origin_1", lambda d, og, a, v: og.__setitem__((slice(None), a), v), (inf, -inf))
    per_axis("inf_dir_1", lambda d, og, a, v: d.__setitem__((slice(None), a), v), (inf, -inf))
    out["zero_dir"] = rays(np.zeros((per_class, 3)), o + rng.uniform(-0.5, 0.5, (per_class, 3)).astype(np.float32))
    # one or two exact zeros (both signs of zero), the origin's coordinate on each zero axis a leaf box's
    # lo or hi bound: (bound - o) * (1 / 0) is 0 * inf = NaN for that bound and +-inf for the other
    rows = []
    for i in range(2 * per_class):
        zero_axes = [(i % 3,), (i % 3, (i + 1) % 3)][(i // 3) % 2]
        box = lb[int(rng.integers(len(lb)))]
        og = o.copy()
        # from the camera's coordinates on the other axes towards the leaf's centre, in the plane of its face
        d = (0.5 * (box[:3] + box[3:]) - og).astype(np.float32)
        if not np.isfinite(d).all() or not np.abs(d).max() > 0:
            d = unit_dirs(rng, 1)[0]
        d = (d / np.linalg.norm(d)).astype(np.float32)
        for a in zero_axes:
            d[a] = np.float32(0.0) if i % 2 else np.float32(-0.0)
            og[a] = box[a] if (i // 2) % 2 else box[3 + a]
        rows.append(rays(d, og))
    out["zero_dir_on_bound"] = np.concatenate(rows)
    d = unit_dirs(rng, 2 * per_class)
    for i in range(len(d)):
        d[i, i % 3] = np.float32([1e-40, -1e-40, 1.4e-45, -1e-38][i % 4])   # denormal (and the smallest normal's side)
        if i >= per_class:
            d[i, (i + 1) % 3] = np.float32(3e-42)
    out["denormal_dir"] = rays(d, o)
    og = np.tile(o, (2 * per_class, 1))
    for i in range(len(og)):
        og[i, i % 3] = np.float32(3e38 if i % 2 else -3e38)
        if i >= per_class:
            og[i] = np.float32(3e38 if i % 2 else -3e38)
    out["huge_origin"] = rays(unit_dirs(rng, 2 * per_class), og)
    out["far_origin_1e30"] = rays(unit_dirs(rng, 2 * per_class), np.full(3, 1e30, np.float32))
    return out


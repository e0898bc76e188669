"""The reference's own device functions (oracle/refcpu.py: its kernel text compiled for the host) on the item
sets of tests/device_fn_inputs.py, in the layout rt_debug_fn returns.  Shared by tests/test_reference_cpu.py, which
holds the oracle's functions to them, and tests/test_gpu_reference.py, which holds the kernels' to them.  Needs
oracle/_ref/librefcpu.so; no GPU."""
import numpy as np

import oracle.refcpu as R
from tests import device_fn_inputs as D

F32 = np.float32


def camera(items) -> np.ndarray:
    """genCameraRay's direction per row (cam[10], pixel index bits): float32 [n, 3]."""
    it = np.ascontiguousarray(items, dtype=F32)
    out = np.zeros((len(it), 3), F32)
    cams, inv = np.unique(D.bits(it[:, :10]), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    bounds = np.searchsorted(inv[order], np.arange(len(cams) + 1))
    for c in range(len(cams)):
        rows = order[bounds[c]:bounds[c + 1]]
        out[rows] = R.kat_camera(cams[c].view(F32), D.bits(it[rows, 10]).astype(np.int32))[:, :3]
    return out


def hemi(items) -> np.ndarray:
    """rand_hemi_cosine on the type-1 rows, rand_hemi_uniform on the type-2 rows (n.xyz, type, seed0 bits, seed1
    bits): float32 [n, 6] = dir.xyz, invPdf, the seeds after as bits."""
    it = np.ascontiguousarray(items, dtype=F32)
    out = np.zeros((len(it), 6), F32)
    t1 = it[:, 3] == 1
    for kind, rows in ((1, t1), (2, ~t1)):
        if rows.any():
            d, st = R.kat_hemi(kind, it[rows, :3], D.bits(it[rows, 4:6]))
            out[rows, :4] = d
            out[rows, 4:6] = D.from_bits(st.reshape(-1)).reshape(-1, 2)
    return out


def ggx(items) -> np.ndarray:
    """BRDF_GGX per row (colour.rgb, roughness, v, l, n): float32 [n, 3]."""
    it = np.ascontiguousarray(items, dtype=F32)
    x = np.zeros((len(it), 15), F32)
    x[:, 0], x[:, 1:5], x[:, 5], x[:, 6:15] = 2.0, it[:, 0:4], 1.5, it[:, 4:13]
    return R.kat_ggx(x)


def mt(items) -> np.ndarray:
    """intersect per row (a, b, c, dir, origin): float32 [n, 2] = k, hit."""
    return R.kat_intersect(np.ascontiguousarray(items, dtype=F32)[:, :15])


def box(items) -> np.ndarray:
    """intersectBox per row (dir, origin, lo, hi, ...): float32 [n, 1] = 0 or 1."""
    return R.kat_box(np.ascontiguousarray(items, dtype=F32)[:, :12]).astype(F32).reshape(-1, 1)

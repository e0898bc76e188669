"""The oracles of the denoised previews (helpers of tests/test_gpu_denoise.py and tests/test_denoise_api.py).

``denoise`` restates the filter of include/rt_api.h in numpy float32, operation by operation: the definition
uses only IEEE + - * /, max, min and abs in a fixed order, so the restatement is exact and every comparison
against it is bitwise.  ``guides`` builds the guide buffers from the CPU oracle's camera ray and trace.
"""
import numpy as np

import oracle.oracle as O

F = np.float32
K = (F(0.375), F(0.25), F(0.0625))
DEFAULTS = dict(passes=5, normal_squarings=5, sigma_c=1.5, sigma_p=0.02)


def split(guides):
    """(n, k, P, f, a, m) of a [npix, 12] guide array."""
    g = np.ascontiguousarray(guides, F).reshape(-1, 12)
    return (g[:, 0:3], g[:, 3], g[:, 4:7], g[:, 7].copy().view(np.int32), g[:, 8:11],
            g[:, 11].copy().view(np.int32))


def _grid(a, H, W):
    """[npix, ...] -> [H, W, ...], the pixels past npix zero."""
    out = np.zeros((H * W,) + a.shape[1:], a.dtype)
    out[:a.shape[0]] = a
    return out.reshape((H, W) + a.shape[1:])


def denoise(rgb, guides, npix, width, passes=5, normal_squarings=5, sigma_c=1.5, sigma_p=0.02):
    """rt_denoise_device on the host: float32 [npix, 3]."""
    npix, W = int(npix), int(width)
    H = -(-npix // W)
    rgb = np.ascontiguousarray(rgb, F).reshape(-1, 3)[:npix]
    n, k, P, f, a, _ = split(np.ascontiguousarray(guides, F).reshape(-1, 12)[:npix])
    filt = f > 0
    sigma_c, sigma_p = F(sigma_c), F(sigma_p)
    with np.errstate(all="ignore"):
        x = np.where(filt[:, None], rgb / a, rgb).astype(F)                      # 1. demodulate
        xg, ng, Pg, fg = _grid(x, H, W), _grid(n, H, W), _grid(P, H, W), _grid(filt, H, W)
        sg = _grid(f.astype(F), H, W)
        spk = _grid(sigma_p * k, H, W)
        for i in range(int(passes)):                                             # 2. the passes
            step = 1 << i
            sc2 = ((sigma_c * sigma_c) / sg) / F(step * step)
            acc = np.zeros((H, W, 3), F)
            ws = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    h = K[abs(dx)] * K[abs(dy)]
                    oy, ox = dy * step, dx * step
                    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    ps = (slice(y0, y1), slice(x0, x1))
                    qs = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    xp, xq = xg[ps], xg[qs]
                    if dx == 0 and dy == 0:
                        w = np.full(xp.shape[:2], h, F)
                    else:
                        n_p, n_q = ng[ps], ng[qs]
                        t = np.maximum(F(0), (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1])
                                       + n_p[..., 2] * n_q[..., 2])
                        wn = t
                        for _ in range(int(normal_squarings)):
                            wn = wn * wn
                        d = Pg[qs] - Pg[ps]
                        dpl = np.abs((n_p[..., 0] * d[..., 0] + n_p[..., 1] * d[..., 1]) + n_p[..., 2] * d[..., 2])
                        a_ = dpl / spk[ps]
                        wp = F(1) / (F(1) + a_ * a_)
                        dc = xq - xp
                        d2 = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]
                        wc = F(1) / (F(1) + d2 / sc2[ps])
                        w = (h * (wn * wp)) * wc
                    on = fg[ps] & fg[qs]          # (a pixel past npix is not filterable: _grid)
                    acc[ps] = np.where(on[..., None], acc[ps] + w[..., None] * xq, acc[ps])
                    ws[ps] = np.where(on, ws[ps] + w, ws[ps])
            assert acc.dtype == F and ws.dtype == F
            xg = np.where(fg[..., None], acc / ws[..., None], xg).astype(F)
        x = xg.reshape(-1, 3)[:npix]
        out = np.maximum(np.minimum(x * a, F(1)), F(0))                          # 3. remodulate
    return np.where(filt[:, None], out, rgb).astype(F)


def guides(osc, scene, cam, npix, sample_map):
    """The guide buffers by the definition: n, k and the material from the CPU oracle's camera ray and trace
    (oracle.camera_ray, oracle.trace), P, a and f in float32.  [npix, 12] float32."""
    cam = np.ascontiguousarray(cam, F)
    mat = np.ascontiguousarray(scene.materialData, F).reshape(-1)
    g = np.zeros((npix, 12), F)
    gi = g.view(np.int32)
    for i in range(npix):
        ray = O.camera_ray(cam, i)
        tr = O.trace(osc, ray)
        if tr[5] == 0:   # a miss
            g[i] = (0, 0, 0, -1, 0, 0, 0, 0, 1, 1, 1, 0)
            gi[i, 11] = -1
            continue
        d, o, kk = ray[0:3], ray[3:6], F(tr[3])
        m = int(tr[4])
        g[i, 0:3] = tr[0:3]
        g[i, 3] = kk
        g[i, 4:7] = o + d * kk
        gi[i, 11] = m
        if int(mat[6 * m]) in (1, 2):
            gi[i, 7] = int(sample_map[i])
            g[i, 8:11] = np.maximum(mat[6 * m + 1:6 * m + 4], F(0.01))
        else:
            g[i, 8:11] = 1
    return g

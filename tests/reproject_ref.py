"""The oracle of temporal reprojection (helper of tests/test_gpu_reproject.py and tests/test_reproject_api.py).

``reproject`` restates steps 0-6 of include/rt_api.h in numpy float32, operation by operation, starting from the
basis (rt_reproject_basis' 16 floats): the definition uses only IEEE + - * /, floor, min, max, abs and compares in
a fixed order, so the restatement is exact and every comparison against it is bitwise.  ``project`` is steps 1-2
alone, on any points.
"""
import numpy as np

F = np.float32
DEFAULTS = dict(sigma_p=0.02, normal_min=0.9, max_history=64.0, min_weight=0.25)


def _fmin(a, b):
    """rtm.h's fmin: a NaN operand yields the other one."""
    return np.where((a < b) | (b != b), a, b).astype(F)


def _fmax(a, b):
    return np.where((a > b) | (b != b), a, b).astype(F)


def project(basis, P):
    """Steps 1-2 on points P [n, 3]: (l.y, u, vv), float32 [n] each."""
    B = np.ascontiguousarray(basis, F).reshape(16)
    P = np.ascontiguousarray(P, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        vx, vy, vz = P[:, 0] - B[9], P[:, 1] - B[10], P[:, 2] - B[11]
        lx = (B[0] * vx + B[1] * vy) + B[2] * vz
        ly = (B[3] * vx + B[4] * vy) + B[5] * vz
        lz = (B[6] * vx + B[7] * vy) + B[8] * vz
        t = B[12] / ly
        u = (lx * t + F(0.5)) * B[13]
        vv = (F(0.5) - lz * t) * B[13]
    assert u.dtype == F and vv.dtype == F and ly.dtype == F
    return ly, u, vv


def reproject(prev_rgb, prev_guides, basis, cur_rgb, cur_guides, npix, width, sigma_p=0.02, normal_min=0.9,
              max_history=64.0, min_weight=0.25):
    """rt_reproject_device on the host: (out_rgb float32 [npix, 3], out_guides float32 [npix, 12])."""
    npix, W = int(npix), int(width)
    H = -(-npix // W)
    sigma_p, normal_min, max_history, min_weight = F(sigma_p), F(normal_min), F(max_history), F(min_weight)
    prgb = np.ascontiguousarray(prev_rgb, F).reshape(-1, 3)[:npix]
    pg = np.ascontiguousarray(prev_guides, F).reshape(-1, 12)[:npix]
    crgb = np.ascontiguousarray(cur_rgb, F).reshape(-1, 3)[:npix]
    cg = np.ascontiguousarray(cur_guides, F).reshape(-1, 12)[:npix]
    pgi, cgi = pg.view(np.int32), cg.view(np.int32)
    n_p, k_p, P_p, f_p, a_p, m_p = cg[:, 0:3], cg[:, 3], cg[:, 4:7], cgi[:, 7], cg[:, 8:11], cgi[:, 11]
    with np.errstate(all="ignore"):
        ly, u, vv = project(basis, P_p)
        ok = (f_p > 0) & (ly > 0) & (u >= F(-1)) & (u < F(W)) & (vv >= F(-1)) & (vv < F(H))   # steps 0-2
        u, vv = np.where(ok, u, F(0)), np.where(ok, vv, F(0))
        c0, r0 = np.floor(u), np.floor(vv)
        fu, fv = u - c0, vv - r0
        ci, ri = c0.astype(np.int64), r0.astype(np.int64)
        spk = sigma_p * k_p
        acc = np.zeros((npix, 3), F)
        ws = np.zeros(npix, F)
        hs = np.zeros(npix, F)
        for dr, dc in ((0, 0), (0, 1), (1, 0), (1, 1)):                                     # step 3
            c, r = ci + dc, ri + dr
            b = (fu if dc else F(1) - fu) * (fv if dr else F(1) - fv)
            q = (r + 1) * W + c - 1
            inside = ok & (c >= 0) & (c < W) & (r >= 0) & (q < npix)
            qs = np.where(inside, q, 0)
            n_q, P_q, f_q, a_q, m_q = pg[qs, 0:3], pg[qs, 4:7], pgi[qs, 7], pg[qs, 8:11], pgi[qs, 11]
            dot = (n_p[:, 0] * n_q[:, 0] + n_p[:, 1] * n_q[:, 1]) + n_p[:, 2] * n_q[:, 2]
            d = P_q - P_p
            dpl = np.abs((n_p[:, 0] * d[:, 0] + n_p[:, 1] * d[:, 1]) + n_p[:, 2] * d[:, 2])
            valid = inside & (f_q > 0) & (m_q == m_p) & (dot >= normal_min) & (dpl <= spk)
            xq = prgb[qs] / a_q
            acc = np.where(valid[:, None], acc + b[:, None] * xq, acc)
            ws = np.where(valid, ws + b, ws)
            hs = np.where(valid, hs + b * f_q.astype(F), hs)
        assert acc.dtype == F and ws.dtype == F and hs.dtype == F
        hist = ok & (ws >= min_weight) & (ws > 0)                                           # step 4
        hx = acc / ws[:, None]
        hq = hs / ws
        h = np.where(hq < max_history, hq, max_history).astype(F)
        s = f_p.astype(F)                                                                   # step 5
        tot = h + s
        x = (hx * h[:, None] + (crgb / a_p) * s[:, None]) / tot[:, None]
        blended = _fmax(_fmin(x * a_p, F(1)), F(0))
        assert blended.dtype == F and tot.dtype == F
        small = tot < F(2147483648.0)
        f_out = np.where(small, np.where(small & hist, tot, F(0)).astype(np.int32), np.int32(2147483647))
    out_rgb = np.where(hist[:, None], blended, crgb).astype(F)                              # step 6
    out_g = cg.copy()
    out_g.view(np.int32)[:, 7] = np.where(hist, f_out, f_p)
    return out_rgb, out_g

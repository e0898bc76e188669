"""Time temporal reprojection (rt_reproject_device) beside the edge-aware filter (rt_denoise_device) on the same
frames of C2 and C3 (1024 x 1024), in one session: device-resident data, HIP events around one call on one stream,
2 warm-ups and the median of 7 (min and max kept as the session's spread), the launches alternating round by round
(tools/lens_bench.py's protocol).

The previous frame is --prev-spp samples at the config's camera moved by 0.1 in x and turned 2 degrees about z, the
current one --cur-spp samples at the config's camera; the filter runs on the reprojected frame and guides, at its
defaults (five passes).  "bytes" is what the definition moves per frame when every pixel gathers four taps: 60 B
read and 60 B written per pixel plus 4 x 60 B of taps, most of which neighbouring lanes share in cache.

    python tools/reproject_bench.py [--out profiles/NAME.json] [--configs C2,C3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from radiance_bench import RUNS, WARMUP, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--prev-spp", type=int, default=8)
    ap.add_argument("--cur-spp", type=int, default=2)
    args = ap.parse_args()
    import torch
    from ensem3a_openclraytracer_amd import workloads as W
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher

    res = {"tool": "tools/reproject_bench.py", "warmup": WARMUP, "runs": RUNS, "device": torch.cuda.get_device_name(0),
           "prev_spp": args.prev_spp, "cur_spp": args.cur_spp, "frames": {}}
    for name in args.configs.split(","):
        wl = W.CONFIGS[name]
        sc, cam, env, npix, _, mb, ibl = wl.inputs()
        cam = np.asarray(cam, np.float32)
        pcam = cam.copy()
        pcam[0] += np.float32(0.1)
        pcam[5] += np.float32(2.0)
        kl = KernelLauncher(None, None, 0, None)
        kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.BVH.exportArray,
                             cam, env, npix, mb, ibl).close()   # (uploads the scene and the IBL)
        ctx = kl.native
        stream = torch.cuda.Stream()
        s = stream.cuda_stream
        new = lambda k: torch.zeros(k * npix, dtype=torch.float32, device="cuda")   # noqa: E731
        d_prgb, d_pg, d_crgb, d_cg, d_rgb, d_g, d_den = new(3), new(12), new(3), new(12), new(3), new(12), new(3)
        torch.cuda.synchronize()
        for c, spp, rgb, g in ((pcam, args.prev_spp, d_prgb, d_pg), (cam, args.cur_spp, d_crgb, d_cg)):
            ctx.accum_begin_device(c, env, npix, mb, 0, 1)
            ctx.accum_add_device(spp, rgb.data_ptr(), s)
            ctx.accum_guides_device(g.data_ptr(), s)
            stream.synchronize()
        ctx.accum_end()

        def reproject():
            ctx.reproject_device(d_prgb.data_ptr(), d_pg.data_ptr(), pcam, d_crgb.data_ptr(), d_cg.data_ptr(), npix,
                                 wl.width, d_rgb.data_ptr(), d_g.data_ptr(), None, s)

        def denoise():
            ctx.denoise_device(d_rgb.data_ptr(), d_g.data_ptr(), npix, wl.width, d_den.data_ptr(), None, s)

        reproject()
        stream.synchronize()
        fr = {"workload": wl.name, "width": wl.width, "height": wl.height, "npix": npix}
        fr.update(timed(torch, stream, {"reproject": reproject, "denoise_5_passes": denoise}))
        stream.synchronize()
        f0 = d_cg.view(torch.int32)[7::12]
        f1 = d_g.view(torch.int32)[7::12]
        fr["filterable"] = float((f0 > 0).float().mean().item())
        fr["with_history_of_filterable"] = float((f1 > f0).sum().item() / max(int((f0 > 0).sum().item()), 1))
        fr["bytes_own"] = 120 * npix
        fr["bytes_taps"] = 240 * npix
        t = fr["reproject"]["median_ms"] * 1e-3
        fr["reproject"]["own_GBps"] = fr["bytes_own"] / t / 1e9
        fr["reproject"]["own_and_taps_GBps"] = (fr["bytes_own"] + fr["bytes_taps"]) / t / 1e9
        fr["reproject_over_denoise"] = fr["reproject"]["median_ms"] / fr["denoise_5_passes"]["median_ms"]
        kl.close()
        res["frames"][name] = fr
        print(name, json.dumps(fr), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

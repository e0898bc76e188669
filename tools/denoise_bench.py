"""Time the denoised-preview kernels on the frames of C2 (1024 x 1024) and C4 (1920 x 1080), HIP events on one
stream, 2 warm-ups and the median of 4 (min and max kept as the session's spread):

  * the add(8) a viewer's tick runs, and the guide kernel and the filter that would follow it;
  * the filter at 1..5 passes -- the time of pass i is the difference of two totals -- for both values of the
    option "denoise_lds" (1: the pass at step 1 stages its tile in LDS), the baseline being 0;
  * the tap bandwidth of a pass, 25 taps x 48 B x pixels / time.

    python tools/denoise_bench.py [--out profiles/NAME.json] [--configs C2,C4]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WARMUP, RUNS = 2, 4


def timed(torch, stream, fn):
    ms = []
    for k in range(WARMUP + RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if k >= WARMUP:
            ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="C2,C4")
    args = ap.parse_args()
    import torch
    from ensem3a_openclraytracer_amd import _native
    from ensem3a_openclraytracer_amd import workloads as W
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher

    res = {"tool": "tools/denoise_bench.py", "warmup": WARMUP, "runs": RUNS, "device": torch.cuda.get_device_name(0),
           "frames": {}}
    for name in args.configs.split(","):
        wl = W.CONFIGS[name]
        sc, cam, env, npix, _, mb, ibl = wl.inputs()
        kl = KernelLauncher(None, None, 0, None)
        kl.begin_progressive(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.BVH.exportArray,
                             cam, env, npix, mb, ibl).close()   # (uploads the scene and the IBL)
        ctx = kl.native
        stream = torch.cuda.Stream()
        s = stream.cuda_stream
        d_rgb = torch.zeros(3 * npix, dtype=torch.float32, device="cuda")
        d_g = torch.zeros(12 * npix, dtype=torch.float32, device="cuda")
        d_out = torch.zeros(3 * npix, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.accum_begin_device(cam, env, npix, mb, 0, 1)
        ctx.accum_add_device(8, d_rgb.data_ptr(), s)
        fr = {"width": wl.width, "height": wl.height, "npix": npix}
        fr["add8"] = timed(torch, stream, lambda: ctx.accum_add_device(8, d_rgb.data_ptr(), s))
        fr["guides"] = timed(torch, stream, lambda: ctx.accum_guides_device(d_g.data_ptr(), s))
        stream.synchronize()
        f = d_g.view(torch.int32)[7::12]
        fr["filterable"] = float((f > 0).float().mean().item())
        fr["denoise"] = {}
        keep = None
        for mask in (0, 1):
            ctx.set_option("denoise_lds", mask)
            rows = []
            for passes in (1, 2, 3, 4, 5):
                P = _native.DenoiseParams(passes=passes)
                t = timed(torch, stream, lambda: ctx.denoise_device(d_rgb.data_ptr(), d_g.data_ptr(), npix, wl.width,
                                                                    d_out.data_ptr(), P, s))
                t["passes"] = passes
                rows.append(t)
            for k in range(1, 5):   # pass k + 1 alone (step 1 << k): the difference of two totals
                dt = rows[k]["median_ms"] - rows[k - 1]["median_ms"]
                rows[k]["last_pass_ms"] = dt
                rows[k]["last_pass_tap_GBps"] = 25 * 48 * npix / (dt * 1e-3) / 1e9 if dt > 0 else None
            fr["denoise"]["lds_%d" % mask] = rows
            got = d_out.clone()
            if keep is None:
                keep = got
            fr["denoise"]["lds_%d_same_bits" % mask] = bool(torch.equal(keep.view(torch.int32), got.view(torch.int32)))
        ctx.set_option("denoise_lds", -1)
        ctx.accum_end()
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

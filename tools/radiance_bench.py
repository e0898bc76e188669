"""Time the radiance queries (rt_radiance_device) beside the render of the same frame, on the scenes of C2, C3 and C5:
device-resident camera rays (rt_camera_rays_device), HIP events on one stream, 2 warm-ups and the median of 7 (min and
max kept as the session's spread), the three launches alternating in one session on the same build:

  (a) the frame's camera rays in pixel order;
  (b) the same rays (with their seeds) in a seeded random permutation;
  (c) rt_render_device of the frame, at the same spp and max_bounce.

C2 and C3 run at their configs' spp; C5 at a few spp only (--c5-spp): the query walks its BVH2 nodes, the render its
4-wide layout.  "ratio" is a query's median over the render's.  "same_frame" says that clamp(sum / n) of (a), and of
(b) put back in pixel order, is the render's frame, bit for bit.

    python tools/radiance_bench.py [--out profiles/NAME.json] [--configs C2,C3,C5] [--c5-spp 4]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WARMUP, RUNS = 2, 7


def timed(torch, stream, launches):
    """{name: median / min / max ms}, the launches alternating round by round."""
    ms = {k: [] for k in launches}
    for it in range(WARMUP + RUNS):
        for name, run in launches.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            run()
            b.record(stream)
            b.synchronize()
            if it >= WARMUP:
                ms[name].append(a.elapsed_time(b))
    return {name: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)} for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--c5-spp", type=int, default=4)
    args = ap.parse_args()
    import torch
    from ensem3a_openclraytracer_amd import _native
    from ensem3a_openclraytracer_amd import workloads as W

    res = {"tool": "tools/radiance_bench.py", "warmup": WARMUP, "runs": RUNS, "device": torch.cuda.get_device_name(0),
           "scenes": {}}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")

    for name in args.configs.split(","):
        wl = W.CONFIGS[name]
        sc, cam, env, npix, spp, mb, ibl = wl.inputs()
        if name == "C5":
            spp = args.c5_spp
        cam, env = np.asarray(cam, np.float32), np.asarray(env, np.float32)
        ctx = _native.Context(device_ids=[0])
        ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray)
        ctx.set_env(ibl)
        info = ctx.scene_info()
        stream = torch.cuda.Stream()
        s = stream.cuda_stream
        row = {"workload": wl.name, "triangles": info["tris"], "rays": npix, "spp": spp, "max_bounce": mb,
               "render_engine": "brute force" if info["brute_records"] else "tree walk",
               "query_engine": "brute force" if info["brute_records"] else "BVH2 walk"}

        rays = torch.empty((npix, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.camera_rays_device(0, cam, npix, 0, npix, rays.data_ptr(), s)
        stream.synchronize()
        g = torch.Generator(device="cpu").manual_seed(23)
        perm = torch.randperm(npix, generator=g).cuda()
        shuffled = rays[perm].contiguous()
        st_a = torch.empty((npix, 8), dtype=torch.int32, device="cuda")
        st_b = torch.empty((npix, 8), dtype=torch.int32, device="cuda")
        frame = torch.empty(3 * npix, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        launches = {
            "query_pixel_order": lambda: ctx.radiance_device(0, rays.data_ptr(), npix, env, spp, mb, 0, st_a.data_ptr(), s),
            "query_shuffled": lambda: ctx.radiance_device(0, shuffled.data_ptr(), npix, env, spp, mb, 0, st_b.data_ptr(), s),
            "render": lambda: ctx.render_device(cam, env, npix, spp, mb, 0, 1, frame.data_ptr(), s),
        }
        row.update(timed(torch, stream, launches))
        stream.synchronize()
        for k in ("query_pixel_order", "query_shuffled"):
            row[k]["ratio"] = row[k]["median_ms"] / row["render"]["median_ms"]
            row[k]["Msamples_per_s"] = npix * spp / (row[k]["median_ms"] * 1e-3) / 1e6
        row["render"]["Msamples_per_s"] = npix * spp / (row["render"]["median_ms"] * 1e-3) / 1e6

        def pixels(state):   # Raytracing.cl:211-220: fmax(fmin(sum / n, 1), 0)
            mean = state[:, 0:3].view(torch.float32) / state[:, 7:8].to(torch.float32)
            return torch.fmax(torch.fmin(mean, torch.ones_like(mean)), torch.zeros_like(mean)).reshape(-1)

        back = torch.empty_like(st_b)
        back[perm] = st_b
        want = frame.view(torch.int32)
        row["same_frame"] = bool(torch.equal(pixels(st_a).view(torch.int32), want) and
                                 torch.equal(pixels(back).view(torch.int32), want))
        row["same_records"] = bool(torch.equal(st_a, back))
        ctx.close()
        res["scenes"][name] = row
        print(name, json.dumps(row), flush=True)
        write()
        del rays, shuffled, st_a, st_b, back, frame
        torch.cuda.empty_cache()
    write()


if __name__ == "__main__":
    main()

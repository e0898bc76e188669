"""Time the ray queries (rt_trace_device) on the scenes of C2, C3 and C5: device-resident rays, HIP events on one
stream, 2 warm-ups and the median of 5 (min and max kept as the session's spread), the plain form ("query_engine" 1)
and the persistent form (2) alternating in one session on the same rays:

  (a) the frame's camera rays in pixel order (closest hit);
  (b) the same rays in a seeded random permutation (closest hit);
  (c) any-hit rays of tmax = 5 % of the scene's diagonal, from the camera hits along cosine-distributed
      directions about the facing normal (ambient occlusion's rays).

Beside them the render's own rate on the scene: the rays rt_count_work counts in the config's frame over the frame's
time.  "persistent_wins" applies the rule of DESIGN.md 2.2: the persistent form's median beats the plain form's by more
than the plain form's max - min, on (a) and on (b).

    python tools/query_bench.py [--out profiles/NAME.json] [--configs C2,C3,C5] [--no-render]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WARMUP, RUNS = 2, 5
ENGINES = {"plain": 1, "persistent": 2}


def timed_pair(torch, stream, run, n):
    """{form: median / min / max ms and Mrays/s}, the two forms alternating launch by launch."""
    ms = {k: [] for k in ENGINES}
    for it in range(WARMUP + RUNS):
        for form, engine in ENGINES.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            run(engine)
            b.record(stream)
            b.synchronize()
            if it >= WARMUP:
                ms[form].append(a.elapsed_time(b))
    return {form: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v),
                   "Mrays_per_s": n / (float(np.median(v)) * 1e-3) / 1e6} for form, v in ms.items()}


def wins(t):
    p, q = t["plain"], t["persistent"]
    return bool(p["median_ms"] - q["median_ms"] > p["max_ms"] - p["min_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--no-render", action="store_true", help="skip the render's own rate (a frame and its counted twin)")
    args = ap.parse_args()
    import torch
    from ensem3a_openclraytracer_amd import _native
    from ensem3a_openclraytracer_amd import workloads as W

    res = {"tool": "tools/query_bench.py", "warmup": WARMUP, "runs": RUNS, "device": torch.cuda.get_device_name(0),
           "scenes": {}}
    for name in args.configs.split(","):
        wl = W.CONFIGS[name]
        sc, cam, env, npix, spp, mb, ibl = wl.inputs()
        cam = np.asarray(cam, np.float32)
        ctx = _native.Context(device_ids=[0])
        ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray)
        info = ctx.scene_info()
        stream = torch.cuda.Stream()
        s = stream.cuda_stream
        row = {"workload": wl.name, "triangles": info["tris"], "rays": npix,
               "engine": "brute force" if info["brute_records"] else "tree walk"}

        # (a) the camera rays, from the kernels' own camera_dir (rt_debug_fn), in chunks
        dirs = np.zeros((npix, 3), np.float32)
        for b in range(0, npix, 1 << 20):
            e = min(npix, b + (1 << 20))
            items = np.zeros((e - b, 11), np.float32)
            items[:, :10] = cam[:10]
            items[:, 10] = np.arange(b, e, dtype=np.int32).view(np.float32)
            dirs[b:e] = ctx.debug_fn("camera", items)
        rays = torch.zeros((npix, 8), dtype=torch.float32, device="cuda")
        rays[:, 0:3] = torch.from_numpy(dirs).cuda()
        rays[:, 3:6] = torch.from_numpy(cam[:3].copy()).cuda()
        rays[:, 6] = 1000.0
        out = torch.empty((npix, 4), dtype=torch.float32, device="cuda")
        keep = {}

        def run_on(r, o, mode):
            def run(engine):
                ctx.set_option("query_engine", engine)
                ctx.trace_device(0, r.data_ptr(), r.shape[0], mode, o.data_ptr(), s)
            return run

        torch.cuda.synchronize()
        row["camera_pixel_order"] = timed_pair(torch, stream, run_on(rays, out, _native.RT_QUERY_CLOSEST), npix)
        for form, engine in ENGINES.items():
            run_on(rays, out, _native.RT_QUERY_CLOSEST)(engine)
            stream.synchronize()
            keep[form] = out.clone()
        row["same_bits"] = bool(torch.equal(keep["plain"].view(torch.int32), keep["persistent"].view(torch.int32)))
        hits = keep["plain"]
        tri = hits[:, 1].view(torch.int32)
        row["camera_hit_share"] = float((tri >= 0).float().mean().item())

        # (b) the same rays, shuffled
        g = torch.Generator(device="cpu").manual_seed(16)
        perm = torch.randperm(npix, generator=g).cuda()
        shuffled = rays[perm].contiguous()
        row["camera_shuffled"] = timed_pair(torch, stream, run_on(shuffled, out, _native.RT_QUERY_CLOSEST), npix)

        # (c) ambient-occlusion rays from the camera hits
        vp = torch.from_numpy(np.asarray(sc.V_p, np.float32).reshape(-1, 3)).cuda()
        face = torch.from_numpy(np.asarray(sc.faceData, np.int32).reshape(-1, 10)).cuda().long()
        diag = float(np.linalg.norm(np.ptp(np.asarray(sc.V_p, np.float32).reshape(-1, 3), axis=0)))
        idx = torch.nonzero(tri >= 0).squeeze(1)
        t = tri[idx].long()
        a, b_, c = vp[face[t, 7]], vp[face[t, 8]], vp[face[t, 9]]
        nrm = torch.nn.functional.normalize(torch.cross(b_ - a, c - a, dim=1), dim=1)
        d0 = rays[idx, 0:3]
        nrm = torch.where((nrm * d0).sum(1, keepdim=True) > 0, -nrm, nrm)
        p = rays[idx, 3:6] + d0 * hits[idx, 0:1] + 1e-3 * nrm
        g2 = torch.Generator(device="cuda").manual_seed(17)
        u1 = torch.rand(len(idx), generator=g2, device="cuda")
        u2 = torch.rand(len(idx), generator=g2, device="cuda")
        r, phi = torch.sqrt(u1), 2 * np.pi * u2
        helper = torch.where(nrm[:, 0:1].abs() < 0.9, torch.tensor([[1.0, 0, 0]], device="cuda"),
                             torch.tensor([[0, 1.0, 0]], device="cuda"))
        tx = torch.nn.functional.normalize(torch.cross(helper.expand_as(nrm), nrm, dim=1), dim=1)
        ty = torch.cross(nrm, tx, dim=1)
        dirs_ao = (r * torch.cos(phi))[:, None] * tx + (r * torch.sin(phi))[:, None] * ty + torch.sqrt(1 - u1)[:, None] * nrm
        ao = torch.zeros((len(idx), 8), dtype=torch.float32, device="cuda")
        ao[:, 0:3], ao[:, 3:6], ao[:, 6] = dirs_ao, p, 0.05 * diag
        out_ao = torch.empty((len(idx), 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        row["ao_any_hit"] = timed_pair(torch, stream, run_on(ao, out_ao, _native.RT_QUERY_ANY), len(idx))
        row["ao_rays"], row["ao_tmax"] = int(len(idx)), 0.05 * diag
        occl = {}
        for form, engine in ENGINES.items():
            run_on(ao, out_ao, _native.RT_QUERY_ANY)(engine)
            stream.synchronize()
            occl[form] = out_ao[:, 1].view(torch.int32) >= 0
        row["ao_occluded_share"] = float(occl["plain"].float().mean().item())
        row["ao_same_flags"] = bool(torch.equal(occl["plain"], occl["persistent"]))
        row["persistent_wins"] = wins(row["camera_pixel_order"]) and wins(row["camera_shuffled"])
        ctx.set_option("query_engine", 0)

        if not args.no_render:   # the render's own rate: counted rays of the config's frame over its time
            ctx.set_env(ibl)
            frame = torch.empty(3 * npix, dtype=torch.float32, device="cuda")
            ms = []
            for k in range(3):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                ctx.render_device(cam, env, npix, spp, mb, 0, 1, frame.data_ptr(), s)
                b.record(stream)
                b.synchronize()
                if k:
                    ms.append(a.elapsed_time(b))
            n_rays = ctx.count_work(cam, env, npix, spp, mb)["rays"]
            row["render"] = {"spp": spp, "frame_ms": float(np.median(ms)), "rays": int(n_rays),
                             "Mrays_per_s": n_rays / (float(np.median(ms)) * 1e-3) / 1e6}
        ctx.close()
        res["scenes"][name] = row
        print(name, json.dumps(row), flush=True)
        del rays, shuffled, out, ao, out_ao, keep
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

"""Time the lens frames (rt_lens_radiance_device) beside the radiance query of the same frame's camera rays, on the
scenes of C2, C3 and C5: device-resident data, HIP events around one launch on one stream, 2 warm-ups and the median
of 7 (min and max kept as the session's spread), the variants alternating round by round on the same build:

  (a) rt_radiance_device of the frame's camera rays (rt_camera_rays_device): the baseline, one ray per pixel;
  (b) the degenerate lens (jitter 0, aperture 0): the same records, every sample through the per-sample machinery;
  (c) jitter 1, a pinhole;
  (d) jitter 1 with a lens (--aperture, --focus).

C2 and C3 run at their configs' spp; C5 at a few spp only (--c5-spp).  "ratio" is a variant's median over (a)'s.
"expected_c_over_a" is the counter-based expectation for (c): the new mode traces one more primary ray per sample and
does nothing else new, so about (rays + samples) / rays with rt_count_work_detail's counters [2] and [14] of the frame
("expected_exact" takes off the one camera ray per pixel that (a) traces too).  "same_records" says that (b)'s records
are (a)'s in all 32 bytes.

    python tools/lens_bench.py [--out profiles/NAME.json] [--configs C2,C3,C5] [--c5-spp 4]
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
    ap.add_argument("--configs", default="C2,C3,C5")
    ap.add_argument("--c5-spp", type=int, default=4)
    ap.add_argument("--aperture", type=float, default=0.05)
    ap.add_argument("--focus", type=float, default=3.5)
    args = ap.parse_args()
    import torch
    from ensem3a_openclraytracer_amd import _native
    from ensem3a_openclraytracer_amd import workloads as W

    res = {"tool": "tools/lens_bench.py", "warmup": WARMUP, "runs": RUNS, "device": torch.cuda.get_device_name(0),
           "lens": {"aperture": args.aperture, "focus": args.focus}, "scenes": {}}

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
        counts = ctx.count_work_detail(cam, env, npix, spp, mb)
        row = {"workload": wl.name, "triangles": info["tris"], "pixels": npix, "spp": spp, "max_bounce": mb,
               "engine": "brute force" if info["brute_records"] else "BVH2 walk",
               "frame_rays": counts["rays"], "frame_samples": counts["samples"],
               "expected_c_over_a": (counts["rays"] + counts["samples"]) / counts["rays"],
               "expected_exact": (counts["rays"] + counts["samples"] - npix) / counts["rays"]}

        rays = torch.empty((npix, 8), dtype=torch.float32, device="cuda")
        states = {k: torch.empty((npix, 8), dtype=torch.int32, device="cuda") for k in "abcd"}
        torch.cuda.synchronize()
        ctx.camera_rays_device(0, cam, npix, 0, npix, rays.data_ptr(), s)
        stream.synchronize()
        lenses = {"b": _native.Lens(0.0, 0.0, 1.0, 23), "c": _native.Lens(1.0, 0.0, 1.0, 23),
                  "d": _native.Lens(1.0, args.aperture, args.focus, 23)}
        names = {"a": "a_query_camera_rays", "b": "b_degenerate_lens", "c": "c_jitter", "d": "d_jitter_and_lens"}

        def lens_launch(k):
            return lambda: ctx.lens_radiance_device(0, cam, env, lenses[k], npix, 0, npix, spp, mb, 0,
                                                    states[k].data_ptr(), s)

        launches = {names["a"]: lambda: ctx.radiance_device(0, rays.data_ptr(), npix, env, spp, mb, 0,
                                                            states["a"].data_ptr(), s)}
        launches.update({names[k]: lens_launch(k) for k in "bcd"})
        row.update(timed(torch, stream, launches))
        stream.synchronize()
        base = row[names["a"]]["median_ms"]
        for k in "abcd":
            row[names[k]]["ratio"] = row[names[k]]["median_ms"] / base
            row[names[k]]["Msamples_per_s"] = npix * spp / (row[names[k]]["median_ms"] * 1e-3) / 1e6
        row["same_records"] = bool(torch.equal(states["a"], states["b"]))
        row["jitter_changes_the_frame"] = bool(not torch.equal(states["b"][:, 0:3], states["c"][:, 0:3]))
        ctx.close()
        res["scenes"][name] = row
        print(name, json.dumps(row), flush=True)
        write()
        del rays, states
        torch.cuda.empty_cache()
    write()


if __name__ == "__main__":
    main()

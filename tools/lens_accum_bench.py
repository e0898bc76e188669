"""Time the adds of a lens accumulation (rt_accum_begin_lens_device) beside the lens frame they are made of
(rt_lens_radiance_device), on the scenes of C2 and C3 at 1024 x 1024 with the lens (jitter 1, aperture 0, focus 1):
tools/lens_bench.py's protocol -- one session, device-resident records, HIP events around one launch on one stream, 2
warm-ups and the median of 7 (min and max kept as the session's spread), the launches alternating round by round:

  (a) rt_lens_radiance_device with RT_RADIANCE_RESUME over the whole frame at spp: the baseline, the contiguous mapping;
  (b) rt_accum_add_device(spp) on a lens accumulation of the same frame: the tile mapping, then the resolve pass;
  (c) rt_accum_add_selected_device(spp) over rt_accum_select_all: the listed mapping, then the resolve pass;
  (r) rt_radiance_resolve_device over (a)'s records: what a resolve pass costs, for reading (b) and (c);
  (d) the first rt_accum_guides_device of an accumulation -- the centre-hit pass included -- beside a later one; every
      round opens a fresh accumulation and gives it one sample, so the first call is timed 7 times.

"ratio" is a launch's median over (a)'s.  "same_records" says that a fresh accumulation's records after one add of spp
are those of a fresh lens frame at spp, in all 32 bytes (both computed again, untimed, at the end).

    python tools/lens_accum_bench.py [--out profiles/NAME.json] [--configs C2,C3]
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
    args = ap.parse_args()
    import torch
    from ensem3a_openclraytracer_amd import _native
    from ensem3a_openclraytracer_amd import workloads as W

    res = {"tool": "tools/lens_accum_bench.py", "warmup": WARMUP, "runs": RUNS, "device": torch.cuda.get_device_name(0),
           "lens": {"jitter": 1.0, "aperture": 0.0, "focus": 1.0}, "scenes": {}}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")

    for name in args.configs.split(","):
        wl = W.CONFIGS[name]
        sc, cam, env, npix, spp, mb, ibl = wl.inputs()
        cam, env = np.asarray(cam, np.float32), np.asarray(env, np.float32)
        lens = _native.Lens(1.0, 0.0, 1.0, 23)
        ctx = _native.Context(device_ids=[0])
        ctx.set_scene(sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.BVH.exportArray)
        ctx.set_env(ibl)
        info = ctx.scene_info()
        stream = torch.cuda.Stream()
        s = stream.cuda_stream
        row = {"workload": wl.name, "triangles": info["tris"], "pixels": npix, "spp": spp, "max_bounce": mb,
               "engine": "brute force" if info["brute_records"] else "BVH2 walk"}

        state = torch.empty((npix, 8), dtype=torch.int32, device="cuda")
        rgb = torch.empty(3 * npix, dtype=torch.float32, device="cuda")
        out = torch.empty(3 * npix, dtype=torch.float32, device="cuda")
        guides = torch.empty(12 * npix, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        # (a) resumes resident records; (b) and (c) add to one accumulation, whose pixels stay at one count
        ctx.lens_radiance_device(0, cam, env, lens, npix, 0, npix, spp, mb, 0, state.data_ptr(), s)
        ctx.accum_begin_lens_device(cam, env, lens, npix, mb, 0, 1)
        ctx.accum_add_device(spp, out.data_ptr(), s)
        ctx.accum_select_all_device(s)
        stream.synchronize()
        names = {"a": "a_lens_frame_resume", "b": "b_accum_add", "c": "c_accum_add_selected_all", "r": "r_resolve_pass"}
        launches = {
            names["a"]: lambda: ctx.lens_radiance_device(0, cam, env, lens, npix, 0, npix, spp, mb,
                                                         _native.RT_RADIANCE_RESUME, state.data_ptr(), s),
            names["b"]: lambda: ctx.accum_add_device(spp, out.data_ptr(), s),
            names["c"]: lambda: ctx.accum_add_selected_device(spp, out.data_ptr(), s),
            names["r"]: lambda: ctx.radiance_resolve_device(0, state.data_ptr(), npix, rgb.data_ptr(), s),
        }
        row.update(timed(torch, stream, launches))
        stream.synchronize()
        base = row[names["a"]]["median_ms"]
        for k in "abc":
            row[names[k]]["ratio"] = row[names[k]]["median_ms"] / base
            row[names[k]]["Msamples_per_s"] = npix * spp / (row[names[k]]["median_ms"] * 1e-3) / 1e6
        row["samples_per_pixel_at_the_end"] = ctx.accum_samples()

        # (d) the first guides call of an accumulation and the one after it
        ms = {"d_first_guides_with_centre_pass": [], "d_later_guides": []}
        for it in range(WARMUP + RUNS):
            ctx.accum_begin_lens_device(cam, env, lens, npix, mb, 0, 1)
            ctx.accum_add_device(1, out.data_ptr(), s)
            stream.synchronize()
            for key in ms:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                ctx.accum_guides_device(guides.data_ptr(), s)
                b.record(stream)
                b.synchronize()
                if it >= WARMUP:
                    ms[key].append(a.elapsed_time(b))
        row.update({k: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()})

        # the same records: a fresh accumulation's one add of spp against a fresh lens frame at spp
        ctx.accum_begin_lens(cam, env, lens, npix, mb)
        ctx.accum_add(spp, out=np.zeros(3 * npix, np.float32))
        got = ctx.debug_accum_state()
        ctx.lens_radiance_device(0, cam, env, lens, npix, 0, npix, spp, mb, 0, state.data_ptr(), s)
        stream.synchronize()
        want = state.cpu().numpy().view(np.uint32)
        row["same_records"] = bool((got.view(np.uint32).reshape(npix, 8) == want).all())
        ctx.accum_end()
        ctx.close()
        res["scenes"][name] = row
        print(name, json.dumps(row), flush=True)
        write()
        del state, rgb, out, guides
        torch.cuda.empty_cache()
    write()


if __name__ == "__main__":
    main()

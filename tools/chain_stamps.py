"""Where a wave of the clustered one-lane product kernel spends its cycles, section by section (rt_device.h
RT_CHAIN_STAMPS, kStamp*): one frame of a config on a library built with the define.

    python tools/variants.py build stamps=RT_CHAIN_STAMPS=1          (here)
    ENSEM3A_RT_LIB=.../lib/variants/libstamps.so python tools/chain_stamps.py [CONFIG] [OUT.json NAME]

The wave's first active lane reads the wave clock at each border and adds the advance to the section that ends there;
the stamps themselves cost cycles (about a tenth), so the shares are what to read, not the sums.  With OUT.json and
NAME the result is stored under NAME in that file."""
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SECTIONS = ["loop head -> trace entry (shading, hand-out)", "trace entry -> after the shell step", "non-face singles",
            "cluster loop with its item batches", "MT batches (all)", "tail batches and epilogue",
            "trace exit -> loop head (and iterations without a trace)"]


def main():
    from ensem3a_openclraytracer_amd import _native
    from ensem3a_openclraytracer_amd import workloads as W
    from ensem3a_openclraytracer_amd.KernelLauncher import KernelLauncher
    cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
    lib = _native.lib()
    stamped = hasattr(lib, "rt_debug_chain_stamps")   # (a library without the define: the frame's digest alone)
    sc, cam, env, npix, spp, mb, ibl = W.CONFIGS[cfg].inputs()
    kl = KernelLauncher(None, None, 0, None)
    out = np.zeros(3 * npix, np.float32)
    sums = (ctypes.c_ulonglong * 7)()
    args = (out, sc.V_p, sc.V_n, sc.V_uv, sc.faceData, sc.materialData, sc.lightData, sc.BVH.exportArray, cam, env,
            npix, spp, mb, ibl)
    kl.launch_Raytracing(*args)           # warm-up; its sums are read and dropped
    assert not stamped or lib.rt_debug_chain_stamps(sums) == 0
    t0 = time.perf_counter()
    kl.launch_Raytracing(*args)           # (blocking: the frame with its copy to the host)
    ms = (time.perf_counter() - t0) * 1e3
    ll = _native.last_launch()
    assert not stamped or lib.rt_debug_chain_stamps(sums) == 0
    kl.close()
    v = [int(x) for x in sums]
    tot = max(sum(v), 1)
    # the frame's digest: a stamped build must render the product build's frame (compare the two runs' fields)
    res = {"config": cfg, "lib": os.path.basename(os.environ.get("ENSEM3A_RT_LIB", "product")), "brute": ll["brute"],
           "frame_ms_with_copy": round(ms, 2), "frame_sha256": hashlib.sha256(out.tobytes()).hexdigest(),
           "cycles": dict(zip(SECTIONS, v)), "share": {k: round(x / tot, 4) for k, x in zip(SECTIONS, v)},
           "trace_share": round(sum(v[1:6]) / tot, 4)}
    print(json.dumps(res))
    if len(sys.argv) > 3:
        path, name = sys.argv[2], sys.argv[3]
        d = json.load(open(path)) if os.path.exists(path) else {}
        d[name] = res
        json.dump(d, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()

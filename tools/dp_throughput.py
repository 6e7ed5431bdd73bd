#!/usr/bin/env python3
"""tools/dp_throughput.py — what a double-precision context costs against fp32, in one process on one device.

For each grid (a cavity as bench.py builds it: walls on the four edges) it times, with HIP events only (run_timed), --steps
steps after a warm-up run of the same length, --reps times, alternating the forms so that drift hits all alike:

  fp64 step    lbm_amd.LBMDouble, "multistep" 0: d2q9_dp_step, one step per launch, 144 B per lattice update
  fp64 lds     "multistep" 8: d2q9_dp_multi (LDS tiles, 8 steps per launch) — grids up to 1024 x 1024 only
  fp64 auto    the library's own choice
  fp32 step    lbm_amd.LBM, "fuse" 0, "multistep" 0, "resident" 0: d2q9_step, 72 B per lattice update
  fp32 auto    the library's own choice

and prints one JSON line: median MLUPS per form and grid, the float4 copy bandwidth of the device (lbm_copy_bandwidth, the
roofline denominator), each step kernel's share of it, and their ratio (fp64 share over fp32 share).

    python tools/dp_throughput.py                          # 128, 256, 1024, 4096, 8192 squared, 400 steps, 3 repeats
    python tools/dp_throughput.py --sizes 128,256 --forms fp64_lds,fp64_step
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ["fp64_step", "fp64_lds", "fp64_auto", "fp32_step", "fp32_auto"]
LDS_MAX = 1024 * 1024


def cavity(nx, ny):
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0, :] = ob[-1, :] = 1
    ob[:, 0] = ob[:, -1] = 1
    return ob


def open_form(lbm_amd, form, n, ob, max_iters):
    if form.startswith("fp64"):
        sim = lbm_amd.LBMDouble(lbm_amd.make_dparams(n, n, max_iters, obstacles=ob), ob)
        if form == "fp64_step":
            sim.set_option("multistep", 0)
        elif form == "fp64_lds":
            sim.set_option("multistep", 8)
    else:
        sim = lbm_amd.LBM(lbm_amd.make_params(n, n, max_iters, obstacles=ob), ob)
        if form == "fp32_step":
            for k in ("fuse", "multistep", "resident"):
                sim.set_option(k, 0)
    return sim


def measure(lbm_amd, n, forms, steps, reps):
    ob = cavity(n, n)
    out = {}
    ms = {f: [] for f in forms}
    for _ in range(reps):
        for f in forms:
            # one context at a time: 8192 x 8192 in fp64 holds 9.7 GB of grids
            with open_form(lbm_amd, f, n, ob, 2 * steps) as sim:
                sim.upload(None)
                sim.run_timed(steps)
                ms[f].append(sim.run_timed(steps))
    for f in forms:
        med = statistics.median(ms[f])
        out[f] = {"mlups": round(n * n * steps / (med * 1e-3) / 1e6, 1), "us_per_step": round(med * 1e3 / steps, 2),
                  "spread_us": [round(min(ms[f]) * 1e3 / steps, 2), round(max(ms[f]) * 1e3 / steps, 2)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,1024,4096,8192")
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import lbm_amd
    lbm_amd.load_library()
    forms = a.forms.split(",")
    res = {"library": lbm_amd.load_library().lbm_version().decode(), "lib_file": os.path.basename(lbm_amd.LIB_PATH),
           "steps": a.steps, "reps": a.reps, "copy_gbps": round(lbm_amd.copy_bandwidth_gbps(), 1), "grids": {}}
    for n in (int(s) for s in a.sizes.split(",")):
        fs = [f for f in forms if f != "fp64_lds" or n * n <= LDS_MAX]
        g = measure(lbm_amd, n, fs, a.steps, a.reps)
        for f, bytes_per in (("fp64_step", 144), ("fp32_step", 72)):
            if f in g:
                g[f]["share_of_copy_bw"] = round(g[f]["mlups"] * 1e6 * bytes_per / 1e9 / res["copy_gbps"], 3)
        if "fp64_step" in g and "fp32_step" in g:
            g["fp64_over_fp32_share"] = round(g["fp64_step"]["share_of_copy_bw"] / g["fp32_step"]["share_of_copy_bw"], 3)
        res["grids"]["%dx%d" % (n, n)] = g
    print(json.dumps(res))


if __name__ == "__main__":
    main()

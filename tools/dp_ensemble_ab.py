#!/usr/bin/env python3
"""tools/dp_ensemble_ab.py — is a double-precision ensemble worth having?  tools/ensemble_ab.py for fp64: times, in one
process on one device, N members of a shipped input

  (a) as a double-precision ensemble (lbm_amd.EnsembleDouble.run_timed: HIP events around the step loop), and
  (b) the best the existing interface offers: N double-precision contexts (lbm_amd.LBMDouble) with library defaults, every
      run issued before the first sync, wall clock around issue + sync,

for --steps steps after a warm-up run of both, --reps times, alternating a and b so that clock drift of the box hits both
alike; every repeat starts from the rest state (same work).  Member 0 carries the shipped constants, the others sweep omega
from 1.0 up to the shipped value.  Prints one JSON line: per case the median / min / max microseconds per step of both sides,
their ratio (b over a: how many times faster the ensemble is), the same ratio for the slowest ensemble repeat against the
fastest contexts repeat, and the aggregate MLUPS (members x cells x steps / time).

    python tools/dp_ensemble_ab.py                       # 64 x 128x128 and 16 x 256x256, 2000 steps, 5 repeats
    python tools/dp_ensemble_ab.py --cases 128x128:8 --steps 4000

Tile A/B of d2q9_dp_ensemble: a measurement build forces one shape (Makefile, LBM_DENS_FLAGS); link it under another
name beside the library and name it in LBM_LIB.  Several processes in one shell line: give each its own time limit and chain
them with &&, so that nothing starts after one has failed:

    timeout -k 10 300 env LBM_LIB=liblbm_hip_a.so python tools/dp_ensemble_ab.py && \\
    timeout -k 10 300 env LBM_LIB=liblbm_hip_b.so python tools/dp_ensemble_ab.py
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(us):
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}


def measure(size, members, steps=2000, reps=5, warmup=200, contexts=True):
    import lbm_amd
    inputs = os.path.join(ROOT, "inputs")
    p, obst = lbm_amd.read_inputs_double(os.path.join(inputs, "input_%s.params" % size),
                                         os.path.join(inputs, "obstacles_%s.dat" % size))
    p.max_iters = max(steps, warmup)
    omegas = [p.omega] + [float(v) for v in np.linspace(1.0, p.omega, members)[:members - 1]]
    params = lbm_amd.sweep_dparams(p, omega=omegas)
    ens = lbm_amd.EnsembleDouble(params, obst)
    ctxs = [lbm_amd.LBMDouble(pm, obst) for pm in params] if contexts else []

    def run_ensemble(n):
        ens.upload(None)
        t0 = time.perf_counter()
        ms = ens.run_timed(n)
        return ms * 1e3 / n, (time.perf_counter() - t0) * 1e6 / n

    def run_contexts(n):
        for c in ctxs:
            c.upload(None)
        t0 = time.perf_counter()
        for c in ctxs:
            c.run(n)
        for c in ctxs:
            c.sync()
        return (time.perf_counter() - t0) * 1e6 / n

    run_ensemble(warmup)
    if contexts:
        run_contexts(warmup)
    a_dev, a_wall, b_wall = [], [], []
    for _ in range(reps):
        dev, wall = run_ensemble(steps)
        a_dev.append(dev)
        a_wall.append(wall)
        if contexts:
            b_wall.append(run_contexts(steps))
    cells = members * p.nx * p.ny
    a = spread(a_dev)
    out = {"size": size, "members": members, "steps": steps, "reps": reps,
           "ensemble_us_per_step": a, "ensemble_wall_us_per_step": spread(a_wall),
           "ensemble_mlups": round(cells / a["median"], 1)}
    if contexts:
        b = spread(b_wall)
        out.update({"contexts_us_per_step": b, "contexts_multistep": ctxs[0].get_option("multistep"),
                    "speedup": round(b["median"] / a["median"], 3),
                    "speedup_worst_case": round(b["min"] / a["max"], 3),   # slowest ensemble repeat against fastest contexts repeat
                    "intervals_disjoint": a["max"] < b["min"],
                    "contexts_mlups": round(cells / b["median"], 1)})
    for c in ctxs:
        c.close()
    ens.close()
    return out


def device_name():
    """marketing name of device 0, or its architecture where the runtime has no name for it"""
    hip = ctypes.CDLL("libamdhip64.so")
    buf = ctypes.create_string_buffer(256)
    if hip.hipDeviceGetName(buf, 256, 0) == 0 and buf.value:
        return buf.value.decode()
    out = subprocess.run(["rocm_agent_enumerator"], capture_output=True, text=True).stdout.split()
    return next((a for a in out if a != "gfx000"), "?")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", default="128x128:64,256x256:16", help="size:members, comma-separated (shipped input sizes)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ensemble-only", action="store_true", help="skip side (b): the tile A/B of measurement builds")
    args = ap.parse_args()
    import lbm_amd
    out = {"tool": "dp_ensemble_ab", "library": lbm_amd.load_library().lbm_version().decode(),
           "lib_file": os.path.basename(lbm_amd.LIB_PATH), "device": device_name(), "cases": []}
    for case in args.cases.split(","):
        size, members = case.split(":")
        out["cases"].append(measure(size, int(members), args.steps, args.reps, contexts=not args.ensemble_only))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

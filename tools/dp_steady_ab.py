#!/usr/bin/env python3
"""tools/dp_steady_ab.py — what does stopping every member on the device buy in double precision?  tools/steady_ab.py for
fp64: times, in one process on one device, a sweep of N members of a shipped input over omega (the input read as its fp64
ancestor read it), from the rest state to every member's own steady state,

  (a) with lbm_amd.EnsembleDouble.run_until (lbm_dsteady_run: legs of --window steps, a member stops when its av_vels
      record has changed by less than --rel-tol over one window), and
  (b) the only way without it: lbm_amd.EnsembleDouble.run (lbm_dens_run) to the SLOWEST member's count (taken from a),
      every member advanced for all of it,

wall clock around the call plus its sync, --reps times, alternating a and b so that clock drift of the box hits both alike,
after one warm-up of both.  Prints one JSON line: the members' stop counts, the share of the member-steps of (b) that (a)
still computes, the median / min / max milliseconds of both sides and their ratio (b over a: how many times faster run_until
gets every member to its steady state).

One process on one device; give it a time limit of its own:

    timeout -k 10 300 python tools/dp_steady_ab.py     # 64 x 128x128, omega 1.0 ... the input's own, window 64, rel_tol 1e-4
    timeout -k 10 300 python tools/dp_steady_ab.py --window 16 --rel-tol 1e-5
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def measure(size, members, max_steps, window, rel_tol, reps=5):
    import lbm_amd
    inputs = os.path.join(ROOT, "inputs")
    p, obst = lbm_amd.read_inputs_double(os.path.join(inputs, "input_%s.params" % size),
                                         os.path.join(inputs, "obstacles_%s.dat" % size))
    p.max_iters = max_steps
    omegas = [float(v) for v in np.linspace(1.0, float(p.omega), members)]
    ens = lbm_amd.EnsembleDouble(lbm_amd.sweep_dparams(p, omega=omegas), obst)

    def run_until():
        ens.upload(None)
        t0 = time.perf_counter()
        steps, conv = ens.run_until(max_steps, window=window, rel_tol=rel_tol)   # synchronises
        return (time.perf_counter() - t0) * 1e3, steps, conv

    def run_plain(n):
        ens.upload(None)
        t0 = time.perf_counter()
        ens.run(n)
        ens.sync()
        return (time.perf_counter() - t0) * 1e3

    _, steps, conv = run_until()
    slowest = int(steps.max())
    run_plain(slowest)
    a, b = [], []
    for _ in range(reps):
        ms, again, _ = run_until()
        assert again.tolist() == steps.tolist()   # the same work every repeat
        a.append(ms)
        b.append(run_plain(slowest))
    ens.close()
    sa, sb = spread(a), spread(b)
    return {"size": size, "members": members, "max_steps": max_steps, "window": window, "rel_tol": rel_tol, "reps": reps,
            "omega": [round(omegas[0], 4), round(omegas[-1], 4)],
            "stop_steps": {"min": int(steps.min()), "median": int(np.median(steps)), "max": slowest},
            "converged": int(conv.sum()),
            "member_steps_share": round(float(steps.sum()) / (members * slowest), 4),
            "run_until_ms": sa, "run_to_slowest_ms": sb,
            "run_until_us_per_step": round(sa["median"] * 1e3 / slowest, 3),
            "run_to_slowest_us_per_step": round(sb["median"] * 1e3 / slowest, 3),
            "speedup": round(sb["median"] / sa["median"], 3),
            "speedup_worst_case": round(sb["min"] / sa["max"], 3)}   # slowest run_until repeat against fastest plain repeat


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="128x128", help="a shipped input size")
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--max-steps", type=int, default=40000)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--rel-tol", type=float, default=1e-4)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import lbm_amd
    from ensemble_ab import device_name
    out = {"tool": "dp_steady_ab", "library": lbm_amd.load_library().lbm_version().decode(), "device": device_name(),
           "cases": [measure(args.size, args.members, args.max_steps, args.window, args.rel_tol, args.reps)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

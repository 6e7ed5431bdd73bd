#!/usr/bin/env python3
"""tools/scalar_steady_ab.py — what does the scalar's record cost, and what does stopping every member on it buy?
tools/buoy_ab.py's method for lbm_drecord_* and tools/dp_steady_ab.py's for lbm_drecord_steady_run: one process per
measurement on one device,

  ensemble   scalar_ab's double-precision ensemble (64 x 128x128 by default) with a passive scalar, the record off (dp_scalar_step)
             and on (dp_scalar_step_rec and three more reductions a flush), HIP events around the step loop,
  step       one double-precision context of 8192 x 8192 at "multistep" 0 with a passive scalar, the record off and on,
  steady     a sweep of side-heated closed boxes over the Rayleigh number (64 x 128x128, Pr 0.71, omega 1.5, c_ref 0.5, from rest on
             the conduction profile): EnsembleDouble.run_until(on="scalar_flux_x") against the only way without it, run to the
             SLOWEST member's count (taken from run_until), wall clock around the call plus its sync; every repeat restarts flow
             and scalar,

each for --reps repeats after a warm-up of every side, alternated so that clock drift of the box hits all alike.  Each measurement
runs in a child process of its own under a time limit of its own (--timeout seconds): if one runs out the child is killed and the
tool exits 124 with nothing written.  The plain path, with no scalar, against a build of the parent commit is
tools/wall_ab.py --against.

Prints ONE JSON line: per measurement and side the median / min / max.  Nothing gates it.

    timeout -k 10 500 python tools/scalar_steady_ab.py         # all three, written to profiles/scalar_steady_throughput.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from open_ab import alternate, disc_channel       # noqa: E402  (beside this file)
from scalar_ab import D, ensemble, first_field    # noqa: E402
from wall_ab import spread, summary               # noqa: E402

MARK = "---- by hand"
RHO0, OMEGA, PR, C_REF = 0.1, 1.5, 0.71, 0.5


def measure_ensemble(lbm_amd, size, members, steps, reps, warmup):
    sides = {"off": ensemble(lbm_amd, size, members, steps, warmup), "on": ensemble(lbm_amd, size, members, steps, warmup)}
    for sim in sides.values():
        sim.set_scalar(D, first_field(size))
    sides["on"].set_scalar_record(True)
    us = alternate(sides, steps, reps, warmup)
    content = sides["on"].scalar_record()[0]
    extra = {"size": "%dx%d" % (size, size), "members": members, "steps": steps, "reps": reps, "D": D,
             "record_is_finite": bool(content.shape == (members, steps) and np.all(np.isfinite(content)))}
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "ensemble", us, extra)


def measure_step(lbm_amd, size, steps, reps, warmup):
    ob = disc_channel(size)
    p = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.7, obstacles=ob)
    sides = {"off": lbm_amd.LBMDouble(p, ob), "on": lbm_amd.LBMDouble(p, ob)}
    for sim in sides.values():
        sim.set_option("multistep", 0)
        sim.set_scalar(D, first_field(size))
    sides["on"].set_scalar_record(True)
    us = alternate(sides, steps, reps, warmup)
    content = sides["on"].scalar_record()[0]
    extra = {"size": "%dx%d" % (size, size), "steps": steps, "reps": reps, "D": D,
             "record_is_finite": bool(content.shape == (steps,) and np.all(np.isfinite(content)))}
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "step", us, extra)


def measure_steady(lbm_amd, size, members, cap, window, rel_tol, reps):
    """the box of tests/_scalar_record_ref.py at `size`: column 0 held at 1, column size - 1 at 0, rows 0 and size - 1 insulating"""
    H = size - 2
    ob = np.zeros((size, size), dtype=np.int32)
    ob[0] = ob[size - 1] = 1
    ob[:, 0] = ob[:, size - 1] = 1
    nu = (1.0 / OMEGA - 0.5) / 3.0
    kappa = nu / PR
    ras = [float(v) for v in np.geomspace(1e3, 3e4, members)]
    bs = [(0.0, ra * nu * kappa * RHO0 / H ** 3) for ra in ras]
    wall = np.full((size, size), np.nan)
    wall[1:size - 1, 0], wall[1:size - 1, size - 1] = 1.0, 0.0
    c0 = np.broadcast_to(1.0 - (np.arange(size, dtype=np.float64) - 0.5)[None, :] / H, (size, size)).copy()
    p = lbm_amd.make_dparams(size, size, cap, density=RHO0, accel=0.0, omega=OMEGA, obstacles=ob)
    ens = lbm_amd.EnsembleDouble([p] * members, ob)

    def restart():
        ens.upload(None)
        ens.set_scalar(kappa, c0, wall)
        if ens.buoyancy() is None:
            ens.set_buoyancy(bs, C_REF)
            ens.set_scalar_record(True)
        ens.sync()

    def run_until():
        restart()
        t0 = time.perf_counter()
        steps, conv = ens.run_until(cap, window=window, rel_tol=rel_tol, on="scalar_flux_x")   # synchronises
        return (time.perf_counter() - t0) * 1e3, steps, conv

    def run_plain(n):
        restart()
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
    flux_x = ens.scalar_record()[1][:, -1]
    ens.close()
    sa, sb = spread(a), spread(b)
    from dp_ensemble_ab import device_name     # beside this file
    return {"what": "steady", "library": lbm_amd.load_library().lbm_version().decode(), "device": device_name(),
            "size": "%dx%d" % (size, size), "members": members, "Ra": [ras[0], ras[-1]], "max_steps": cap, "window": window,
            "rel_tol": rel_tol, "reps": reps, "stop_steps": {"min": int(steps.min()), "median": int(np.median(steps)), "max": slowest},
            "converged": int(conv.sum()), "member_steps_share": round(float(steps.sum()) / (members * slowest), 4),
            "run_until_ms": sa, "run_to_slowest_ms": sb, "speedup": round(sb["median"] / sa["median"], 3),
            "speedup_worst_case": round(sb["min"] / sa["max"], 3), "record_is_finite": bool(np.all(np.isfinite(flux_x)))}


def child(args):
    sys.path.insert(0, ROOT)
    import lbm_amd
    if args.child == "step":
        out = measure_step(lbm_amd, args.step_size, args.step_steps, args.reps, args.step_warmup)
    elif args.child == "ensemble":
        out = measure_ensemble(lbm_amd, args.size, args.members, args.steps, args.reps, args.warmup)
    else:
        out = measure_steady(lbm_amd, args.size, args.members, args.max_steps, args.window, args.rel_tol, args.reps)
    print(json.dumps(out))
    return 0


def run_child(args, what):
    """one measurement in a process of its own, bounded; its result, or an exit code"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--size", str(args.size), "--members", str(args.members),
           "--steps", str(args.steps), "--reps", str(args.reps), "--warmup", str(args.warmup), "--step-size", str(args.step_size),
           "--step-steps", str(args.step_steps), "--step-warmup", str(args.step_warmup), "--max-steps", str(args.max_steps),
           "--window", str(args.window), "--rel-tol", str(args.rel_tol)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print("scalar_steady_ab: the %s measurement did not end within %d s" % (what, args.timeout), file=sys.stderr)
        return None, 124
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        return None, r.returncode
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]), 0


WHATS = ["ensemble", "step", "steady"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=WHATS, help="one of the three measurements")
    ap.add_argument("--size", type=int, default=128, help="ensemble members are size x size")
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--step-size", type=int, default=8192, help="the context of the step measurement is step-size squared")
    ap.add_argument("--step-steps", type=int, default=100)
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=16000, help="the cap of the steady sweep")
    ap.add_argument("--window", type=int, default=500)
    ap.add_argument("--rel-tol", type=float, default=1e-3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds one measuring child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar_steady_throughput.txt"),
                    help="where the line is written ('' for nowhere)")
    ap.add_argument("--child", choices=WHATS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the parent never opens the device: it starts the measuring children, bounds each, and keeps their results
    result = {"tool": "scalar_steady_ab"}
    for what in ([args.only] if args.only else WHATS):
        result[what], rc = run_child(args, what)
        if rc != 0:
            return rc
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        # what stands below the mark is written by hand (registers, the instruction comparison, the plain path against the parent)
        kept = ""
        if os.path.exists(args.out):
            text = open(args.out).read()
            if MARK in text:
                kept = "\n" + text[text.index(MARK):]
        shown = " ".join(a for a in sys.argv[1:] if not a.startswith("--out") and a != args.out)
        with open(args.out, "w") as f:
            f.write("The scalar's record and steady runs on it (lbm_drecord_*, lbm_drecord_steady_run): tools/scalar_steady_ab.py\n"
                    "on one device.\n\n"
                    "One process per measurement.  Ensemble and step: a passive scalar (D = 0.05) with the record off and on, HIP events\n"
                    "around the step loop, alternated repeats after a warm-up of every side, every repeat restarts the flow from the rest\n"
                    "state; us/step.  Steady: a sweep of side-heated closed boxes over the Rayleigh number, run_until(on=\"scalar_flux_x\")\n"
                    "against run to the slowest member's count, wall clock, ms; every repeat restarts flow and scalar.  Nothing is gated.\n")
            f.write("\n$ python tools/scalar_steady_ab.py %s\n%s\n%s" % (shown, line, kept))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""tools/buoy_ab.py — what does buoyancy cost beside a passive scalar?  tools/scalar_ab.py's method for lbm_dbuoy_*: times, in one
process per measurement on one device, with HIP events around the step loop (run_timed),

  ensemble   scalar_ab's double-precision ensemble (64 x 128x128 by default) with the scalar passive (one dp_scalar_step<false> and
             one LDS-tile launch of depth 1 per step) and with buoyancy on (one dp_scalar_step<true> and one d2q9_dp_buoyant per
             step),
  step       one double-precision context of 8192 x 8192 at "multistep" 0 with no scalar (d2q9_dp_step), with the scalar passive
             and with buoyancy on.  Buoyant less passive plus d2q9_dp_step is what the buoyant pair costs; the pair moves about
             173 + 184 B per lattice update (dp_scalar_step<true>: 72 read from the flow, 40 + 16 + 40 of the scalar, the mask
             bytes; d2q9_dp_buoyant: 72 + 72 of the flow, 40 of the scalar), an estimate from the code, and that is set against
             lbm_copy_bandwidth.  The split between the two kernels is not in these timings: a kernel trace gives it
             (rocprofv3 --kernel-trace --stats -- python tools/buoy_ab.py --child step --step-steps 20 --reps 1),

each for --reps repeats after a warm-up of every side, alternated so that clock drift of the box hits all alike; every repeat
restarts the flow from the rest state (the scalar goes on from where it is).  Each measurement runs in a child process of its own
under a time limit of its own (--timeout seconds): if one runs out the child is killed and the tool exits 124 with nothing written.
The plain path, with no scalar, against a build of the parent commit is tools/wall_ab.py --against.

Prints ONE JSON line: per measurement and side the median / min / max microseconds per step.  Nothing gates it.

    timeout -k 10 330 python tools/buoy_ab.py                  # both, written to profiles/buoy_throughput.txt
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from open_ab import alternate, disc_channel       # noqa: E402  (beside this file)
from scalar_ab import D, ensemble, first_field    # noqa: E402
from wall_ab import spread, summary               # noqa: E402

B, C_REF = (0.0, 1e-5), 1.0
BYTES_SCALAR, BYTES_FLOW = 173.0, 184.0
MARK = "---- by hand"


def measure_ensemble(lbm_amd, size, members, steps, reps, warmup):
    sides = {"passive": ensemble(lbm_amd, size, members, steps, warmup), "buoyant": ensemble(lbm_amd, size, members, steps, warmup)}
    for sim in sides.values():
        sim.set_scalar(D, first_field(size))
    sides["buoyant"].set_buoyancy(B, C_REF)
    us = alternate(sides, steps, reps, warmup)
    cells = members * size * size
    extra = {"size": "%dx%d" % (size, size), "members": members, "steps": steps, "reps": reps, "D": D, "b": B, "c_ref": C_REF,
             "passive_mlups": round(cells / statistics.median(us["passive"]), 1),
             "buoyant_mlups": round(cells / statistics.median(us["buoyant"]), 1),
             "ratio_buoyant_over_passive": round(statistics.median(us["buoyant"]) / statistics.median(us["passive"]), 4),
             "state_is_finite": bool(np.all(np.isfinite(sides["buoyant"].scalar_field())) and
                                     np.all(np.isfinite(sides["buoyant"].final_state()[2])))}
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "ensemble", us, extra)


def measure_step(lbm_amd, size, steps, reps, warmup):
    ob = disc_channel(size)
    p = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.7, obstacles=ob)
    sides = {"off": lbm_amd.LBMDouble(p, ob), "passive": lbm_amd.LBMDouble(p, ob), "buoyant": lbm_amd.LBMDouble(p, ob)}
    for name, sim in sides.items():
        sim.set_option("multistep", 0)
        if name != "off":
            sim.set_scalar(D, first_field(size))
    sides["buoyant"].set_buoyancy(B, C_REF)
    us = alternate(sides, steps, reps, warmup)
    gbps = ctypes.c_double()
    rc = lbm_amd.load_library().lbm_copy_bandwidth(ctypes.c_size_t(1 << 30), 10, ctypes.byref(gbps))
    assert rc == 0, rc
    pair = us["buoyant"]                                                       # dp_scalar_step<true> + d2q9_dp_buoyant per step
    pair_gbps = (BYTES_SCALAR + BYTES_FLOW) * size * size / statistics.median(pair) / 1e3
    alone = [a - b for a, b in zip(us["passive"], us["off"])]                  # dp_scalar_step<false> alone, repeat by repeat
    extra = {"size": "%dx%d" % (size, size), "steps": steps, "reps": reps, "D": D, "b": B, "c_ref": C_REF,
             "ratio_buoyant_over_passive": round(statistics.median(us["buoyant"]) / statistics.median(us["passive"]), 4),
             "passive_scalar_alone_us_per_step": spread(alone), "copy_gbps": round(gbps.value, 1),
             "buoyant_pair_gbps_at_357": round(pair_gbps, 1), "buoyant_pair_over_copy": round(pair_gbps / gbps.value, 4)}
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "step", us, extra)


def child(args):
    sys.path.insert(0, ROOT)
    import lbm_amd
    if args.child == "step":
        out = measure_step(lbm_amd, args.step_size, args.step_steps, args.reps, args.step_warmup)
    else:
        out = measure_ensemble(lbm_amd, args.size, args.members, args.steps, args.reps, args.warmup)
    print(json.dumps(out))
    return 0


def run_child(args, what):
    """one measurement in a process of its own, bounded; its result, or an exit code"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--size", str(args.size), "--members", str(args.members),
           "--steps", str(args.steps), "--reps", str(args.reps), "--warmup", str(args.warmup), "--step-size", str(args.step_size),
           "--step-steps", str(args.step_steps), "--step-warmup", str(args.step_warmup)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print("buoy_ab: the %s measurement did not end within %d s" % (what, args.timeout), file=sys.stderr)
        return None, 124
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        return None, r.returncode
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]), 0


WHATS = ["ensemble", "step"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=WHATS, help="one of the two measurements")
    ap.add_argument("--size", type=int, default=128, help="ensemble members are size x size")
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--step-size", type=int, default=8192, help="the context of the step measurement is step-size squared")
    ap.add_argument("--step-steps", type=int, default=100)
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=150, help="seconds one measuring child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "buoy_throughput.txt"), help="where the line is written ('' for nowhere)")
    ap.add_argument("--child", choices=WHATS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the parent never opens the device: it starts the measuring children, bounds each, and keeps their results
    result = {"tool": "buoy_ab"}
    for what in ([args.only] if args.only else WHATS):
        result[what], rc = run_child(args, what)
        if rc != 0:
            return rc
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        # what stands below the mark is written by hand (registers, the kernel trace, the plain path against the parent): keep it
        kept = ""
        if os.path.exists(args.out):
            text = open(args.out).read()
            if MARK in text:
                kept = "\n" + text[text.index(MARK):]
        shown = " ".join(a for a in sys.argv[1:] if not a.startswith("--out") and a != args.out)
        with open(args.out, "w") as f:
            f.write("Buoyancy (lbm_dbuoy_*): tools/buoy_ab.py on one device.\n\n"
                    "One process per measurement; the scalar passive and with buoyancy on (D = 0.05, b = (0, 1e-5), c_ref = 1, insulating\n"
                    "walls), HIP events around the step loop, alternated repeats after a warm-up of every side, every repeat restarts the\n"
                    "flow from the rest state.  Ensemble: a walled channel with a blocked disc, a sweep over omega, us/step for all members\n"
                    "together; passive is one dp_scalar_step<false> and one LDS-tile launch of depth 1 per step, buoyant one\n"
                    "dp_scalar_step<true> and one d2q9_dp_buoyant.  Step: one context at \"multistep\" 0, with no scalar too; the buoyant\n"
                    "pair against the device's copy rate at 173 + 184 B per lattice update (an estimate from the code).  Nothing is gated.\n")
            f.write("\n$ python tools/buoy_ab.py %s\n%s\n%s" % (shown, line, kept))
    return 0


if __name__ == "__main__":
    sys.exit(main())

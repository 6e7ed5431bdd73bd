#!/usr/bin/env python3
"""tools/scalar_ab.py — what does a passive scalar cost?  tools/drive_ab.py's method for lbm_dscalar_*: times, in one process per
measurement on one device, with HIP events around the step loop (run_timed),

  ensemble   a double-precision ensemble (64 x 128x128 by default: a walled channel with a blocked disc, a sweep over omega from
             1.0 to 1.85) with the scalar off (the launches of a library without it: three steps per launch) and on (D = 0.05,
             insulating walls: one dp_scalar_step and one flow launch per step),
  step       one double-precision context of 8192 x 8192 at "multistep" 0, the bandwidth-bound d2q9_dp_step, off and on; the
             difference per step is dp_scalar_step alone, given as a fraction of lbm_copy_bandwidth at 157 B per lattice update
             (72 read from the flow, 40 + 40 of the scalar, the mask bytes),
  plain      with --parent-root DIR (a checkout of the parent commit with its library built): the ensemble with no scalar on this
             tree and on that one, in alternated processes, one process per repeat,

each for --reps repeats after a warm-up of both sides, alternating off and on so that clock drift of the box hits both alike;
every repeat restarts the flow from the rest state (same work; the scalar goes on from where it is).  Each measurement runs in a
child process of its own under a time limit of its own (--timeout seconds): if one runs out the child is killed and the tool exits
124 with nothing written, so a chain of commands stops there.

Prints ONE JSON line: per measurement and side the median / min / max microseconds per step and the ratio on over off.  The cost
is whatever the run shows; nothing gates it.

    timeout -k 10 330 python tools/scalar_ab.py                # ensemble and step, written to profiles/scalar_throughput.txt
    python tools/scalar_ab.py --parent-root ../parent          # and the plain path against that tree's build
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
from open_ab import alternate, disc_channel     # noqa: E402  (beside this file)
from wall_ab import spread, summary             # noqa: E402

D = 0.05
BYTES_PER_UPDATE = 157.0
MARK = "---- figures of the flows with known answers"


def ensemble(lbm_amd, size, members, steps, warmup):
    ob = disc_channel(size)
    base = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.85, obstacles=ob)
    params = lbm_amd.sweep_dparams(base, omega=[float(v) for v in np.linspace(1.0, 1.85, members)])
    return lbm_amd.EnsembleDouble(params, ob)


def first_field(size):
    y, x = np.mgrid[0:size, 0:size]
    return 1.0 + 0.5 * np.sin(2.0 * np.pi * x / size) * np.cos(2.0 * np.pi * y / size)


def measure_ensemble(lbm_amd, size, members, steps, reps, warmup):
    sides = {"off": ensemble(lbm_amd, size, members, steps, warmup), "on": ensemble(lbm_amd, size, members, steps, warmup)}
    sides["on"].set_scalar(D, first_field(size))
    us = alternate(sides, steps, reps, warmup)
    extra = {"size": "%dx%d" % (size, size), "members": members, "steps": steps, "reps": reps, "D": D,
             "off_mlups": round(members * size * size / statistics.median(us["off"]), 1),
             "on_mlups": round(members * size * size / statistics.median(us["on"]), 1),
             "field_is_finite": bool(np.all(np.isfinite(sides["on"].scalar_field())))}
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "ensemble", us, extra)


def measure_step(lbm_amd, size, steps, reps, warmup):
    ob = disc_channel(size)
    p = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.7, obstacles=ob)
    sides = {"off": lbm_amd.LBMDouble(p, ob), "on": lbm_amd.LBMDouble(p, ob)}
    sides["on"].set_scalar(D, first_field(size))
    for sim in sides.values():
        sim.set_option("multistep", 0)
    us = alternate(sides, steps, reps, warmup)
    gbps = ctypes.c_double()
    rc = lbm_amd.load_library().lbm_copy_bandwidth(ctypes.c_size_t(1 << 30), 10, ctypes.byref(gbps))
    assert rc == 0, rc
    alone = [on - off for on, off in zip(us["on"], us["off"])]              # dp_scalar_step alone, repeat by repeat
    alone_gbps = BYTES_PER_UPDATE * size * size / statistics.median(alone) / 1e3
    extra = {"size": "%dx%d" % (size, size), "kernel": "d2q9_dp_step", "steps": steps, "reps": reps, "D": D,
             "off_gbps_at_144": round(144.0 * size * size / statistics.median(us["off"]) / 1e3, 1),
             "scalar_alone_us_per_step": spread(alone), "scalar_alone_gbps_at_157": round(alone_gbps, 1),
             "copy_gbps": round(gbps.value, 1), "scalar_alone_over_copy": round(alone_gbps / gbps.value, 4)}
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "step", us, extra)


def measure_plain_once(lbm_amd, size, members, steps, warmup):
    """one repeat of the ensemble with no scalar on the tree the child imports: us per step"""
    sim = ensemble(lbm_amd, size, members, steps, warmup)
    us = alternate({"off": sim}, steps, 1, warmup)["off"][0]
    sim.close()
    return {"us_per_step": us, "library": lbm_amd.load_library().lbm_version().decode()}


def child(args):
    sys.path.insert(0, os.path.abspath(args.root) if args.root else ROOT)
    import lbm_amd
    if args.child == "step":
        out = measure_step(lbm_amd, args.step_size, args.step_steps, args.reps, args.step_warmup)
    elif args.child == "plain":
        out = measure_plain_once(lbm_amd, args.size, args.members, args.steps, args.warmup)
    else:
        out = measure_ensemble(lbm_amd, args.size, args.members, args.steps, args.reps, args.warmup)
    print(json.dumps(out))
    return 0


def run_child(args, what, root=None):
    """one measurement in a process of its own, bounded; its result, or an exit code.  root: the tree whose package the child
    imports (None: this one)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--size", str(args.size), "--members", str(args.members),
           "--steps", str(args.steps), "--reps", str(args.reps), "--warmup", str(args.warmup), "--step-size", str(args.step_size),
           "--step-steps", str(args.step_steps), "--step-warmup", str(args.step_warmup)]
    if root:
        cmd += ["--root", root]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print("scalar_ab: the %s measurement did not end within %d s" % (what, args.timeout), file=sys.stderr)
        return None, 124
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        return None, r.returncode
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]), 0


def plain_against_parent(args):
    """the plain path on this build and on the parent's, one process per repeat, alternated"""
    us = {"this": [], "parent": []}
    for _ in range(args.reps):
        for name, root in (("this", None), ("parent", args.parent_root)):
            res, rc = run_child(args, "plain", root)
            if rc != 0:
                return None, rc
            us[name].append(res["us_per_step"])
    out = {"what": "plain", "this_us_per_step": spread(us["this"]),
           "parent_us_per_step": spread(us["parent"]), "this_repeats": [round(v, 3) for v in us["this"]],
           "parent_repeats": [round(v, 3) for v in us["parent"]]}
    out["ratio_this_over_parent"] = round(out["this_us_per_step"]["median"] / out["parent_us_per_step"]["median"], 4)
    lo, hi = min(us["parent"]), max(us["parent"])
    out["this_median_inside_parent_spread"] = bool(lo <= statistics.median(us["this"]) <= hi)
    return out, 0


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
    ap.add_argument("--timeout", type=int, default=100, help="seconds one measuring child may take")
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its library built")
    ap.add_argument("--root", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar_throughput.txt"), help="where the line is written ('' for nowhere)")
    ap.add_argument("--child", choices=WHATS + ["plain"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the parent never opens the device: it starts the measuring children, bounds each, and keeps their results
    result = {"tool": "scalar_ab"}
    for what in ([args.only] if args.only else WHATS):
        result[what], rc = run_child(args, what)
        if rc != 0:
            return rc
    if args.parent_root:
        result["plain"], rc = plain_against_parent(args)
        if rc != 0:
            return rc
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        # what stands below the mark is written by hand (the figures of the tests' flows on the device): keep it
        kept = ""
        if os.path.exists(args.out):
            text = open(args.out).read()
            if MARK in text:
                kept = "\n" + text[text.index(MARK):]
        shown = " ".join(a for a in sys.argv[1:] if not a.startswith("--out") and a != args.out)
        with open(args.out, "w") as f:
            f.write("Passive scalar (lbm_dscalar_*): tools/scalar_ab.py on one device.\n\n"
                    "One process per measurement; the scalar off and on (D = 0.05, insulating walls), HIP events around the step loop,\n"
                    "alternated repeats after a warm-up of both, every repeat restarts the flow from the rest state.  Ensemble: a walled\n"
                    "channel with a blocked disc, a sweep over omega, us/step for all members together; off is three steps per launch,\n"
                    "on is one dp_scalar_step and one flow launch per step.  Step: one context at \"multistep\" 0; on less off is\n"
                    "dp_scalar_step alone, against the device's copy rate at 157 B per lattice update.  Plain: the ensemble with no scalar\n"
                    "on this build and on a build of the parent commit, one process per repeat, alternated.  Nothing is gated.\n")
            f.write("\n$ python tools/scalar_ab.py %s\n%s\n%s" % (shown, line, kept))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""tools/drive_ab.py — what does the body force cost?  tools/les_ab.py's method for lbm_ddrive_*: times, in one process per
measurement on one device, with HIP events around the step loop (run_timed),

  ensemble_bgk   a double-precision ensemble (64 x 128x128 by default: a walled channel with a blocked disc, a sweep over omega
                 from 1.0 to 1.85) with the force off (the instances a library without it launches) and with F = (1e-6, 0) in
                 every member (the DRIVE instances of d2q9_dp_ensemble),
  ensemble_trt   the same with two relaxation times (Lambda = 3/16) on both sides: the source split over the two rates, and
  step           one double-precision context of 8192 x 8192 at "multistep" 0, the bandwidth-bound d2q9_dp_step, off and on, and
                 off once more on a context created after the other two (a control for where a context's arrays lie),

each for --reps repeats after a warm-up of both sides, alternating off and on so that clock drift of the box hits both alike;
every repeat starts from the rest state (same work).  Each measurement runs in a child process of its own under a time limit of
its own (--timeout seconds): if one runs out the child is killed and the tool exits 124 with nothing written, so a chain of
commands stops there.

No comparison with another tree: the instances with the force off are, instruction for instruction, those of a library without
it, which tools/dp_isa_diff.py shows on the two builds' disassembly without a device.

Prints ONE JSON line: per measurement and side the median / min / max microseconds per step and the ratio on over off.  The cost
is whatever the run shows; nothing gates it.

    timeout -k 10 330 python tools/drive_ab.py               # all three, written to profiles/drive_throughput.txt
    python tools/drive_ab.py --only ensemble_bgk --members 16 --size 256
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from open_ab import alternate, disc_channel     # noqa: E402  (beside this file)
from wall_ab import summary                      # noqa: E402

FORCE = (1e-6, 0.0)
MAGIC = 3.0 / 16.0
MARK = "---- resources of the DRIVE instances"


def measure_ensemble(lbm_amd, size, members, steps, reps, warmup, trt):
    ob = disc_channel(size)
    base = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.85, obstacles=ob)
    params = lbm_amd.sweep_dparams(base, omega=[float(v) for v in np.linspace(1.0, 1.85, members)])
    sides = {"off": lbm_amd.EnsembleDouble(params, ob), "on": lbm_amd.EnsembleDouble(params, ob)}
    if trt:
        for sim in sides.values():
            sim.set_trt(MAGIC)
    sides["on"].set_drive(FORCE)
    us = alternate(sides, steps, reps, warmup)
    av_on, av_off = sides["on"].download(cells=False)[1], sides["off"].download(cells=False)[1]
    extra = {"size": "%dx%d" % (size, size), "members": members, "steps": steps, "reps": reps, "force": list(FORCE),
             "operator": "TRT %.4f" % MAGIC if trt else "BGK",
             "off_mlups": round(members * size * size / statistics.median(us["off"]), 1),
             "on_mlups": round(members * size * size / statistics.median(us["on"]), 1),
             "last_member_last_av_vels_off_on": [float(av_off[-1, -1]), float(av_on[-1, -1])]}
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "ensemble_trt" if trt else "ensemble_bgk", us, extra)


def measure_step(lbm_amd, size, steps, reps, warmup):
    ob = disc_channel(size)
    p = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.7, obstacles=ob)
    sides = {"off": lbm_amd.LBMDouble(p, ob), "on": lbm_amd.LBMDouble(p, ob), "off_again": lbm_amd.LBMDouble(p, ob)}
    sides["on"].set_drive(FORCE)
    for sim in sides.values():
        sim.set_option("multistep", 0)
    us = alternate(sides, steps, reps, warmup)
    # 144 B per lattice update: nine doubles read, nine written (dp_kernels.h)
    extra = {"size": "%dx%d" % (size, size), "kernel": "d2q9_dp_step", "steps": steps, "reps": reps, "force": list(FORCE),
             "off_gbps": round(144.0 * size * size / statistics.median(us["off"]) / 1e3, 1),
             "on_gbps": round(144.0 * size * size / statistics.median(us["on"]) / 1e3, 1)}
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "step", us, extra)


def child(args):
    sys.path.insert(0, ROOT)
    import lbm_amd
    if args.child == "step":
        out = measure_step(lbm_amd, args.step_size, args.step_steps, args.reps, args.step_warmup)
    else:
        out = measure_ensemble(lbm_amd, args.size, args.members, args.steps, args.reps, args.warmup, args.child == "ensemble_trt")
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
        print("drive_ab: the %s measurement did not end within %d s" % (what, args.timeout), file=sys.stderr)
        return None, 124
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        return None, r.returncode
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]), 0


WHATS = ["ensemble_bgk", "ensemble_trt", "step"]


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
    ap.add_argument("--timeout", type=int, default=100, help="seconds one measuring child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drive_throughput.txt"), help="where the line is written ('' for nowhere)")
    ap.add_argument("--child", choices=WHATS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the parent never opens the device: it starts the measuring children, bounds each, and keeps their results
    result = {"tool": "drive_ab"}
    for what in ([args.only] if args.only else WHATS):
        result[what], rc = run_child(args, what)
        if rc != 0:
            return rc
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        # the table of the instances' registers below the mark is written by hand from the compiler's remarks: keep it
        kept = ""
        if os.path.exists(args.out):
            text = open(args.out).read()
            if MARK in text:
                kept = "\n" + text[text.index(MARK):]
        shown = " ".join(a for a in sys.argv[1:] if not a.startswith("--out") and a != args.out)
        with open(args.out, "w") as f:
            f.write("Body force (lbm_ddrive_*): tools/drive_ab.py on one device.\n\n"
                    "One process per measurement; the force off and on (F = (1e-6, 0)), HIP events around the step loop, alternated\n"
                    "repeats after a warm-up of both, every repeat from the rest state.  Ensembles: a walled channel with a blocked disc,\n"
                    "a sweep over omega, us/step for all members together, with BGK and with TRT on both sides.  Step: one context at\n"
                    "\"multistep\" 0.  The cost is what the run shows against the same build with the option off, with the spread of the\n"
                    "repeats; it is not gated.\n")
            f.write("\n$ python tools/drive_ab.py %s\n%s\n%s" % (shown, line, kept))
    return 0


if __name__ == "__main__":
    sys.exit(main())

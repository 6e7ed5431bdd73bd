#!/usr/bin/env python3
"""tools/force_ab.py — what does the force record cost?  tools/dp_ensemble_ab.py's method for the option "force": times, in
one process on one device, a double-precision ensemble (lbm_amd.EnsembleDouble.run_timed: HIP events around the step loop)

  (a) with the option "force" off: the kernels a library without the option launches, and
  (b) with it on: the FORCE instances, three values per segment, two more reductions per batch of steps,

for --steps steps after a warm-up run of both, --reps times, alternating a and b so that clock drift of the box hits both
alike; every repeat starts from the rest state (same work).  The members are a walled channel (rows 0 and ny-1 blocked) with
a blocked disc of radius ny/8 a quarter of the way in, a sweep over omega from 1.0 to 1.85: the flow the record is for.
Prints one JSON line: per side the median / min / max microseconds per step for all members together, the ratio on over off
(medians, and slowest off against fastest on), the last step's drag and lift of member 0 as a sanity check, and writes the
same line to profiles/force_throughput.txt (--out).

The measuring runs in a child process under a time limit of its own (--timeout seconds): if it runs out the child is killed
and the tool exits 124 with nothing written, so a chain of commands stops there.

    python tools/force_ab.py                        # 64 x 128x128, 2000 steps, 5 repeats
    python tools/force_ab.py --members 16 --size 256 --steps 1000
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(us):
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}


def disc_channel(n):
    """rows 0 and n-1 blocked, a blocked disc of radius n/8 centred at (n/4, n/2)"""
    ob = np.zeros((n, n), dtype=np.int32)
    ob[0] = ob[n - 1] = 1
    yy, xx = np.mgrid[0:n, 0:n]
    ob[(xx - n // 4) ** 2 + (yy - n // 2) ** 2 <= (n // 8) ** 2] = 1
    return ob


def measure(size, members, steps, reps, warmup):
    import lbm_amd
    from tools.dp_ensemble_ab import device_name
    ob = disc_channel(size)
    base = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.85, obstacles=ob)
    params = lbm_amd.sweep_dparams(base, omega=[float(v) for v in np.linspace(1.0, 1.85, members)])
    sides = {}
    for name, on in (("off", 0), ("on", 1)):
        ens = lbm_amd.EnsembleDouble(params, ob)
        ens.set_option("force", on)
        sides[name] = ens

    def run(ens, n):
        ens.upload(None)
        return ens.run_timed(n) * 1e3 / n

    for ens in sides.values():
        run(ens, warmup)
    us = {"off": [], "on": []}
    for _ in range(reps):
        for name in ("off", "on"):
            us[name].append(run(sides[name], steps))
    fx, fy = sides["on"].force_record()
    _, av_on = sides["on"].download(cells=False)
    _, av_off = sides["off"].download(cells=False)
    off, on = spread(us["off"]), spread(us["on"])
    out = {"tool": "force_ab", "library": lbm_amd.load_library().lbm_version().decode(), "device": device_name(),
           "size": "%dx%d" % (size, size), "members": members, "steps": steps, "reps": reps,
           "off_us_per_step": off, "on_us_per_step": on,
           "ratio_on_over_off": round(on["median"] / off["median"], 4),
           "ratio_worst_case": round(on["max"] / off["min"], 4), "ratio_best_case": round(on["min"] / off["max"], 4),
           "off_mlups": round(members * size * size / off["median"], 1),
           "on_mlups": round(members * size * size / on["median"], 1),
           "member0_last_step_drag_lift": [float(fx[0, -1]), float(fy[0, -1])],
           "av_vels_identical_on_off": bool(np.array_equal(av_on, av_off))}
    for ens in sides.values():
        ens.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=128, help="members are size x size")
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the measuring child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "force_throughput.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.size, args.members, args.steps, args.reps, args.warmup)))
        return 0
    # the parent never opens the device: it starts the measuring child, bounds it, and keeps its one line
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print("force_ab: the measuring run did not end within %d s" % args.timeout, file=sys.stderr)
        return 124
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        return r.returncode
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("The force record (option \"force\" of lbm_dens_* / lbm_dp_*): tools/force_ab.py on one device.\n\n"
                    "One process; a double-precision ensemble of a walled channel with a blocked disc, a sweep over omega, with the\n"
                    "option off and on, HIP events around the step loop, alternated repeats after a warm-up of both, every repeat\n"
                    "from the rest state.  us/step are for all members together.\n\n$ python tools/force_ab.py %s\n%s\n"
                    % (" ".join(a for a in sys.argv[1:] if not a.startswith("--out") and a != args.out), line))
    return 0


if __name__ == "__main__":
    sys.exit(main())

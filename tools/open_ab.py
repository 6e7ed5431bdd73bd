#!/usr/bin/env python3
"""tools/open_ab.py — what do open boundaries cost?  tools/trt_ab.py's method for lbm_dopen_*: times, in one process on one
device, with HIP events around the step loop (run_timed),

  ensemble   a double-precision ensemble (64 x 128x128 by default: a walled channel with a blocked disc, a sweep over omega
             from 1.0 to 1.85) with open boundaries off (periodic and accelerated: the instances a library without them
             launches) and on (a parabolic inlet profile, rho_out = density: the OPEN instances of d2q9_dp_ensemble), and
  step       one double-precision context of 8192 x 8192 at "multistep" 0, the bandwidth-bound d2q9_dp_step, off and on, and
             off once more on a context created after the other two (a control for where a context's arrays lie),

each for --reps repeats after a warm-up of both sides, alternating off and on so that clock drift of the box hits both alike;
every repeat starts from the rest state (same work).  Each of the two measurements runs in a child process of its own under
a time limit of its own (--timeout seconds): if one runs out the child is killed and the tool exits 124 with nothing
written, so a chain of commands stops there.  Prints one JSON line per measurement: per side the median / min / max
microseconds per step and the ratio on over off.

With --against DIR (a built checkout of another commit, e.g. the parent) the tool instead compares the SETTING-OFF path of
this tree with that of DIR: processes alternate between the two trees, --rounds each, every process imports its own tree's
binding and library and times the off side alone; one JSON line per process.

    python tools/open_ab.py                              # both measurements, written to profiles/open_throughput.txt
    python tools/open_ab.py --only ensemble --members 16 --size 256
    python tools/open_ab.py --against ../parent --rounds 2
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_MAX = 0.05


def spread(us):
    return {"median": round(statistics.median(us), 3), "min": round(min(us), 3), "max": round(max(us), 3)}


def disc_channel(n):
    """rows 0 and n-1 blocked, a blocked disc of radius n/8 centred at (n/4, n/2) (tools/force_ab.py)"""
    ob = np.zeros((n, n), dtype=np.int32)
    ob[0] = ob[n - 1] = 1
    yy, xx = np.mgrid[0:n, 0:n]
    ob[(xx - n // 4) ** 2 + (yy - n // 2) ** 2 <= (n // 8) ** 2] = 1
    return ob


def parabola(n):
    """the inlet profile: 4 U (y - 1/2)(H - (y - 1/2)) / H^2 between the walls on rows 0 and n - 1, H = n - 2"""
    h = float(n - 2)
    y = np.arange(n, dtype=np.float64)
    p = 4.0 * U_MAX * (y - 0.5) * (h - (y - 0.5)) / (h * h)
    p[0] = p[n - 1] = 0.0
    return p


def alternate(sides, steps, reps, warmup):
    """{name: us per step of each repeat}: a warm-up of every side, then the sides in turn, every run from the rest state"""
    def run(sim, n):
        sim.upload(None)
        return sim.run_timed(n) * 1e3 / n

    for sim in sides.values():
        run(sim, warmup)
    us = {name: [] for name in sides}
    for _ in range(reps):
        for name, sim in sides.items():
            us[name].append(run(sim, steps))
    return us


def summary(lbm_amd, what, us, extra):
    from dp_ensemble_ab import device_name     # beside this file
    out = {"tool": "open_ab", "what": what, "library": lbm_amd.load_library().lbm_version().decode(), "device": device_name()}
    out.update(extra)
    for name, v in us.items():
        out[name + "_us_per_step"] = spread(v)
    if "on" in us:
        off, on = out["off_us_per_step"], out["on_us_per_step"]
        out["ratio_on_over_off"] = round(on["median"] / off["median"], 4)
        out["ratio_worst_case"] = round(on["max"] / off["min"], 4)
        out["ratio_best_case"] = round(on["min"] / off["max"], 4)
    return out


def measure_ensemble(lbm_amd, size, members, steps, reps, warmup, off_only):
    ob = disc_channel(size)
    base = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.85, obstacles=ob)
    params = lbm_amd.sweep_dparams(base, omega=[float(v) for v in np.linspace(1.0, 1.85, members)])
    sides = {"off": lbm_amd.EnsembleDouble(params, ob)}
    if not off_only:
        sides["on"] = lbm_amd.EnsembleDouble(params, ob)
        sides["on"].set_open(parabola(size), 0.1)
    us = alternate(sides, steps, reps, warmup)
    extra = {"size": "%dx%d" % (size, size), "members": members, "steps": steps, "reps": reps,
             "off_mlups": round(members * size * size / statistics.median(us["off"]), 1)}
    if not off_only:
        extra["on_mlups"] = round(members * size * size / statistics.median(us["on"]), 1)
        av_on, av_off = sides["on"].download(cells=False)[1], sides["off"].download(cells=False)[1]
        extra["member0_last_av_vels_off_on"] = [float(av_off[0, -1]), float(av_on[0, -1])]
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "ensemble", us, extra)


def measure_step(lbm_amd, size, steps, reps, warmup, off_only):
    ob = disc_channel(size)
    p = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.7, obstacles=ob)
    sides = {"off": lbm_amd.LBMDouble(p, ob)}
    if not off_only:
        sides["on"] = lbm_amd.LBMDouble(p, ob)
        sides["on"].set_open(parabola(size), 0.1)
        # the control: a second periodic context, created last.  What it differs by from the first is what the place of a
        # context's arrays in memory does to this kernel, whichever boundaries it runs with.
        sides["off_again"] = lbm_amd.LBMDouble(p, ob)
    for sim in sides.values():
        sim.set_option("multistep", 0)
    us = alternate(sides, steps, reps, warmup)
    # 144 B per lattice update: nine doubles read, nine written (dp_kernels.h)
    extra = {"size": "%dx%d" % (size, size), "kernel": "d2q9_dp_step", "steps": steps, "reps": reps,
             "off_gbps": round(144.0 * size * size / statistics.median(us["off"]) / 1e3, 1)}
    if not off_only:
        extra["on_gbps"] = round(144.0 * size * size / statistics.median(us["on"]) / 1e3, 1)
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "step", us, extra)


def child(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import lbm_amd
    assert os.path.samefile(lbm_amd.ROOT, args.root), lbm_amd.ROOT
    if args.child == "ensemble":
        out = measure_ensemble(lbm_amd, args.size, args.members, args.steps, args.reps, args.warmup, args.off_only)
    else:
        out = measure_step(lbm_amd, args.step_size, args.step_steps, args.reps, args.step_warmup, args.off_only)
    out["tree"] = args.label
    print(json.dumps(out))
    return 0


def run_child(args, what, root, label, off_only):
    """one measurement in a process of its own, bounded; its JSON line, or an exit code"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--root", root, "--label", label,
           "--size", str(args.size), "--members", str(args.members), "--steps", str(args.steps), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--step-size", str(args.step_size), "--step-steps", str(args.step_steps),
           "--step-warmup", str(args.step_warmup)] + (["--off-only"] if off_only else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print("open_ab: the %s measurement did not end within %d s" % (what, args.timeout), file=sys.stderr)
        return None, 124
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        return None, r.returncode
    return [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1], 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=["ensemble", "step"], help="one of the two measurements")
    ap.add_argument("--size", type=int, default=128, help="ensemble members are size x size")
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--step-size", type=int, default=8192, help="the context of the step measurement is step-size squared")
    ap.add_argument("--step-steps", type=int, default=100)
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--against", help="a built checkout of another commit: compare the setting-off paths of the two trees")
    ap.add_argument("--rounds", type=int, default=2, help="with --against: processes per tree and measurement")
    ap.add_argument("--timeout", type=int, default=150, help="seconds one measuring child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_throughput.txt"),
                    help="where the lines are written ('' for nowhere); with --against they are appended")
    ap.add_argument("--child", choices=["ensemble", "step"], help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--off-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the parent never opens the device: it starts the measuring children, bounds each, and keeps their lines
    whats = [args.only] if args.only else ["ensemble", "step"]
    lines = []
    if args.against:
        for what in whats:
            for _ in range(args.rounds):
                for root, label in ((args.against, "other"), (ROOT, "this")):
                    line, rc = run_child(args, what, root, label, True)
                    if rc != 0:
                        return rc
                    print(line, flush=True)
                    lines.append(line)
    else:
        for what in whats:
            line, rc = run_child(args, what, ROOT, "this", False)
            if rc != 0:
                return rc
            print(line, flush=True)
            lines.append(line)
    if args.out:
        shown = " ".join(a for a in sys.argv[1:] if not a.startswith("--out") and a != args.out)
        with open(args.out, "a" if args.against else "w") as f:
            if not args.against:
                f.write("Open boundaries (lbm_dopen_*): tools/open_ab.py on one device.\n\n"
                        "One process per measurement; open boundaries off (periodic, accelerated) and on (parabolic inlet, rho_out =\n"
                        "density), HIP events around the step loop, alternated repeats after a warm-up of both, every repeat from the rest\n"
                        "state.  Ensemble: a walled channel with a blocked disc, a sweep over omega, us/step for all members together.\n"
                        "Step: one context at \"multistep\" 0.\n")
            f.write("\n$ python tools/open_ab.py %s\n%s\n" % (shown, "\n".join(lines)))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""tools/wall_ab.py — what do moving walls cost?  tools/open_ab.py's method for lbm_dwall_*: times, in one process on one
device, with HIP events around the step loop (run_timed),

  ensemble   a double-precision ensemble (64 x 128x128 by default: a walled channel with a blocked disc, a sweep over omega
             from 1.0 to 1.85) with the disc at rest (no wall velocities: the instances a library without them launches) and
             with the disc spinning (u = Omega x r on its cells, another Omega per member, rim speeds up to 0.05: the WALL
             instances of d2q9_dp_ensemble), and
  step       one double-precision context of 8192 x 8192 at "multistep" 0, the bandwidth-bound d2q9_dp_step, with the lid (the
             wall on row ny - 1) at rest and moving with u_x = 0.05, and at rest once more on a context created after the other
             two (a control for where a context's arrays lie); --step-multistep N runs the same context on the LDS tiles of
             d2q9_dp_multi, N steps per launch (with --step-size 1024 or less),

each for --reps repeats after a warm-up of both sides, alternating rest and motion so that clock drift of the box hits both
alike; every repeat starts from the rest state (same work).  Each measurement runs in a child process of its own under a time
limit of its own (--timeout seconds): if one runs out the child is killed and the tool exits 124 with nothing written, so a
chain of commands stops there.

With --against DIR (a built checkout of another commit, e.g. the parent) the same call then compares the plain path (no wall
velocities) of this tree with that of DIR: processes alternate between the two trees, --rounds each, every process imports
its own tree's binding and library and times the resting side alone.  The two trees agree when their medians over all
repeats differ by no more than the spread (max - min) of the repeats; if they do not, the tool writes its line and exits 1.

Prints ONE JSON line: per measurement and side the median / min / max microseconds per step and the ratio moving over
resting, and with --against the comparison of the two trees.

    python tools/wall_ab.py                              # both measurements, written to profiles/wall_throughput.txt
    python tools/wall_ab.py --only ensemble --members 16 --size 256
    python tools/wall_ab.py --against ../parent --rounds 2
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
from open_ab import alternate, disc_channel, spread     # noqa: E402  (beside this file)

RIM_MAX = 0.05   # the fastest member's rim speed, and the lid's speed


def spinning_disc(n, members):
    """(u_x, u_y) float64[members, n, n]: u = Omega x r on the cells of disc_channel's disc (radius n/8, centre (n/4, n/2)),
    Omega rising with the member to RIM_MAX / radius; zero elsewhere, the walls included"""
    yy, xx = np.mgrid[0:n, 0:n]
    cx, cy, r = n // 4, n // 2, n // 8
    disc = (xx - cx) ** 2 + (yy - cy) ** 2 <= r ** 2
    omegas = RIM_MAX / r * (1.0 + np.arange(members)) / members
    u_x = np.where(disc, -(yy - cy), 0.0)[None] * omegas[:, None, None]
    u_y = np.where(disc, xx - cx, 0.0)[None] * omegas[:, None, None]
    return np.ascontiguousarray(u_x), np.ascontiguousarray(u_y)


def moving_lid(n):
    u_x = np.zeros((n, n), dtype=np.float64)
    u_x[n - 1] = RIM_MAX
    return u_x, np.zeros((n, n), dtype=np.float64)


def summary(lbm_amd, what, us, extra):
    from dp_ensemble_ab import device_name     # beside this file
    out = {"what": what, "library": lbm_amd.load_library().lbm_version().decode(), "device": device_name()}
    out.update(extra)
    for name, v in us.items():
        out[name + "_us_per_step"] = spread(v)
        out[name + "_repeats_us_per_step"] = [round(x, 3) for x in v]
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
    extra = {"size": "%dx%d" % (size, size), "members": members, "steps": steps, "reps": reps}
    if not off_only:
        sides["on"] = lbm_amd.EnsembleDouble(params, ob)
        u_x, u_y = spinning_disc(size, members)
        sides["on"].set_wall(u_x, u_y, 0.1)
        extra["moving_cells_per_member"] = int(np.count_nonzero((u_x[-1] != 0.0) | (u_y[-1] != 0.0)))
        extra["blocked_cells_per_member"] = int(np.count_nonzero(ob))
    us = alternate(sides, steps, reps, warmup)
    extra["off_mlups"] = round(members * size * size / statistics.median(us["off"]), 1)
    if not off_only:
        extra["on_mlups"] = round(members * size * size / statistics.median(us["on"]), 1)
        av_on, av_off = sides["on"].download(cells=False)[1], sides["off"].download(cells=False)[1]
        extra["last_member_last_av_vels_off_on"] = [float(av_off[-1, -1]), float(av_on[-1, -1])]
    for sim in sides.values():
        sim.close()
    return summary(lbm_amd, "ensemble", us, extra)


def measure_step(lbm_amd, size, steps, reps, warmup, off_only, multistep=0):
    ob = disc_channel(size)
    p = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.7, obstacles=ob)
    sides = {"off": lbm_amd.LBMDouble(p, ob)}
    if not off_only:
        sides["on"] = lbm_amd.LBMDouble(p, ob)
        sides["on"].set_wall(*moving_lid(size), 0.1)
        # the control: a second context with every wall at rest, created last.  What it differs by from the first is what the
        # place of a context's arrays in memory does to this kernel, whatever its walls do.
        sides["off_again"] = lbm_amd.LBMDouble(p, ob)
    for sim in sides.values():
        sim.set_option("multistep", multistep)
    us = alternate(sides, steps, reps, warmup)
    # 144 B per lattice update: nine doubles read, nine written (dp_kernels.h)
    extra = {"size": "%dx%d" % (size, size), "kernel": "d2q9_dp_multi" if multistep else "d2q9_dp_step", "multistep": multistep,
             "steps": steps, "reps": reps, "off_gbps": round(144.0 * size * size / statistics.median(us["off"]) / 1e3, 1)}
    if not off_only:
        extra["on_gbps"] = round(144.0 * size * size / statistics.median(us["on"]) / 1e3, 1)
        extra["moving_cells"] = size
        extra["blocked_cells"] = int(np.count_nonzero(ob))
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
        out = measure_step(lbm_amd, args.step_size, args.step_steps, args.reps, args.step_warmup, args.off_only, args.step_multistep)
    out["tree"] = args.label
    print(json.dumps(out))
    return 0


def run_child(args, what, root, label, off_only):
    """one measurement in a process of its own, bounded; its result, or an exit code"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--root", root, "--label", label,
           "--size", str(args.size), "--members", str(args.members), "--steps", str(args.steps), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--step-size", str(args.step_size), "--step-steps", str(args.step_steps),
           "--step-warmup", str(args.step_warmup), "--step-multistep", str(args.step_multistep)] + (["--off-only"] if off_only else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print("wall_ab: the %s measurement did not end within %d s" % (what, args.timeout), file=sys.stderr)
        return None, 124
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        return None, r.returncode
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]), 0


def compare_trees(runs):
    """the plain path of two trees from their children's repeats: medians, spreads and whether the medians differ by no more
    than the repeats spread"""
    pooled = {label: [x for r in runs if r["tree"] == label for x in r["off_repeats_us_per_step"]] for label in ("this", "other")}
    med = {label: statistics.median(v) for label, v in pooled.items()}
    width = {label: max(v) - min(v) for label, v in pooled.items()}
    return {"this_us_per_step": spread(pooled["this"]), "other_us_per_step": spread(pooled["other"]),
            "processes_per_tree": len(runs) // 2, "ratio_this_over_other": round(med["this"] / med["other"], 4),
            "medians_differ_by_us": round(abs(med["this"] - med["other"]), 3), "spread_of_repeats_us": round(max(width.values()), 3),
            "within_spread": abs(med["this"] - med["other"]) <= max(width.values())}


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
    ap.add_argument("--step-multistep", type=int, default=0,
                    help="the step context's \"multistep\": 0 = d2q9_dp_step, 1..8 = d2q9_dp_multi at that depth (grids up to 1024 x 1024)")
    ap.add_argument("--against", help="a built checkout of another commit: also compare the plain paths of the two trees")
    ap.add_argument("--rounds", type=int, default=2, help="with --against: processes per tree and measurement")
    ap.add_argument("--timeout", type=int, default=150, help="seconds one measuring child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wall_throughput.txt"), help="where the line is written ('' for nowhere)")
    ap.add_argument("--child", choices=["ensemble", "step"], help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--off-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the parent never opens the device: it starts the measuring children, bounds each, and keeps their results
    whats = [args.only] if args.only else ["ensemble", "step"]
    result = {"tool": "wall_ab"}
    for what in whats:
        result[what], rc = run_child(args, what, ROOT, "this", False)
        if rc != 0:
            return rc
    agree = True
    if args.against:
        for what in whats:
            runs = []
            for _ in range(args.rounds):
                for root, label in ((args.against, "other"), (ROOT, "this")):
                    out, rc = run_child(args, what, root, label, True)
                    if rc != 0:
                        return rc
                    runs.append(out)
            result[what + "_plain_against_other"] = compare_trees(runs)
            result[what + "_plain_against_other"]["other_library"] = next(r["library"] for r in runs if r["tree"] == "other")
            agree = agree and result[what + "_plain_against_other"]["within_spread"]
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        shown = " ".join(a for a in sys.argv[1:] if not a.startswith("--out") and a != args.out)
        with open(args.out, "w") as f:
            f.write("Moving walls (lbm_dwall_*): tools/wall_ab.py on one device.\n\n"
                    "One process per measurement; wall velocities off (every wall at rest) and on, HIP events around the step loop,\n"
                    "alternated repeats after a warm-up of both, every repeat from the rest state.  Ensemble: a walled channel with a\n"
                    "blocked disc, a sweep over omega, the disc at rest against the disc spinning with another Omega per member, us/step\n"
                    "for all members together.  Step: one context at \"multistep\" 0, the lid at rest against the lid moving.  *_plain_against_other:\n"
                    "the plain path of this tree against that of the tree given with --against, in processes that alternate.\n")
            f.write("\n$ python tools/wall_ab.py %s\n%s\n" % (shown, line))
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""tools/stats_ab.py — what do running statistics cost?  tools/scalar_ab.py's method for lbm_dstats_*: times, in one process per
measurement on one device, with HIP events around the step loop (run_timed),

  ensemble   a double-precision ensemble (64 x 128x128 by default: a walled channel with a blocked disc, a sweep over omega from
             1.0 to 1.85) with the statistics off (the launches of a library without them: three steps per launch) and on at
             every = 1, 3 and 30 (a run cut at its sample points: per cut one dp_stats_sample and one accelerate launch, and
             shallower launches where a piece is no multiple of three),
  step       one double-precision context of 8192 x 8192 at "multistep" 0, the bandwidth-bound d2q9_dp_step, off and on at the
             same three settings; at every = 1 the difference per step is dp_stats_sample (and one accelerate launch of a row)
             alone, given as a fraction of lbm_copy_bandwidth at 169 B per cell and sample (72 of the state, the mask byte,
             48 + 48 of the sums),
  plain      with --parent-root DIR (a checkout of the parent commit with its library built): the ensemble with statistics off
             on this tree and on that one, in alternated processes, one process per repeat,

each for --reps repeats after a warm-up, the four settings in turn within a repeat so that clock drift of the box hits all alike;
every repeat restarts the flow from the rest state, which starts the statistics anew.  One handle serves the four settings of a
measurement: set_stats() between the timed runs allocates and frees the planes.  Each measurement runs in a child process of its
own under a time limit of its own (--timeout seconds): if one runs out the child is killed and the tool exits 124 with nothing
written, so a chain of commands stops there.

Prints ONE JSON line.  The cost is whatever the run shows; nothing gates it.

    timeout -k 10 330 python tools/stats_ab.py                 # ensemble and step, written to profiles/stats_throughput.txt
    python tools/stats_ab.py --parent-root ../parent           # and the plain path against that tree's build
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
from open_ab import disc_channel                # noqa: E402  (beside this file)
from wall_ab import spread                      # noqa: E402

EVERYS = (0, 1, 3, 30)
BYTES_PER_SAMPLE = 169.0
MARK = "---- the kernel and the builds"


def name_of(every):
    return "every_%d" % every if every else "off"


def alternate(sim, steps, reps, warmup):
    """{setting: us per step of each repeat} of one handle: a warm-up, then the settings in turn, every run from the rest state"""
    def run(every, n):
        sim.set_stats(every)
        sim.upload(None)
        return sim.run_timed(n) * 1e3 / n

    for every in EVERYS:
        run(every, warmup)
    us = {name_of(every): [] for every in EVERYS}
    for _ in range(reps):
        for every in EVERYS:
            us[name_of(every)].append(run(every, steps))
            state = sim.stats_state()
            assert state == ((every, 0, steps // every) if every else None), state
    return us


def summary(lbm_amd, what, us, extra):
    from dp_ensemble_ab import device_name      # beside this file
    out = {"what": what, "library": lbm_amd.load_library().lbm_version().decode(), "device": device_name()}
    out.update(extra)
    for name, v in us.items():
        out[name + "_us_per_step"] = spread(v)
        out[name + "_repeats_us_per_step"] = [round(x, 3) for x in v]
    for every in EVERYS[1:]:
        out["ratio_%s_over_off" % name_of(every)] = round(statistics.median(us[name_of(every)]) / statistics.median(us["off"]), 4)
    return out


def ensemble(lbm_amd, size, members, steps, warmup):
    ob = disc_channel(size)
    base = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.85, obstacles=ob)
    params = lbm_amd.sweep_dparams(base, omega=[float(v) for v in np.linspace(1.0, 1.85, members)])
    return lbm_amd.EnsembleDouble(params, ob)


def sample_alone(us, every, cells, copy_gbps):
    """dp_stats_sample from the difference to the run without statistics, repeat by repeat, `every` steps a sample"""
    alone = [(on - off) * every for on, off in zip(us[name_of(every)], us["off"])]
    gbps = BYTES_PER_SAMPLE * cells / statistics.median(alone) / 1e3
    return {"us_per_sample": spread(alone), "gbps_at_169": round(gbps, 1), "over_copy": round(gbps / copy_gbps, 4)}


def copy_rate(lbm_amd):
    gbps = ctypes.c_double()
    rc = lbm_amd.load_library().lbm_copy_bandwidth(ctypes.c_size_t(1 << 30), 10, ctypes.byref(gbps))
    assert rc == 0, rc
    return gbps.value


def measure_ensemble(lbm_amd, size, members, steps, reps, warmup):
    sim = ensemble(lbm_amd, size, members, steps, warmup)
    us = alternate(sim, steps, reps, warmup)
    sim.set_stats(1)
    sim.upload(None)
    sim.run(30)
    finite = bool(np.all(np.isfinite(sim.stats_sums())))
    sim.close()
    copy_gbps = copy_rate(lbm_amd)
    cells = members * size * size
    extra = {"size": "%dx%d" % (size, size), "members": members, "steps": steps, "reps": reps,
             "off_mlups": round(cells / statistics.median(us["off"]), 1), "sums_are_finite": finite, "copy_gbps": round(copy_gbps, 1),
             "cut_from_every_1": sample_alone(us, 1, cells, copy_gbps)}     # a cut: the sample, an accelerate launch, depth 1 for 3
    return summary(lbm_amd, "ensemble", us, extra)


def measure_step(lbm_amd, size, steps, reps, warmup):
    ob = disc_channel(size)
    p = lbm_amd.make_dparams(size, size, max(steps, warmup), density=0.1, accel=0.005, omega=1.7, obstacles=ob)
    sim = lbm_amd.LBMDouble(p, ob)
    sim.set_option("multistep", 0)
    us = alternate(sim, steps, reps, warmup)
    sim.close()
    copy_gbps = copy_rate(lbm_amd)
    cells = size * size
    extra = {"size": "%dx%d" % (size, size), "kernel": "d2q9_dp_step", "steps": steps, "reps": reps,
             "off_gbps_at_144": round(144.0 * cells / statistics.median(us["off"]) / 1e3, 1), "copy_gbps": round(copy_gbps, 1),
             "sample_from_every_1": sample_alone(us, 1, cells, copy_gbps), "sample_from_every_3": sample_alone(us, 3, cells, copy_gbps),
             "sample_from_every_30": sample_alone(us, 30, cells, copy_gbps)}
    return summary(lbm_amd, "step", us, extra)


def measure_plain_once(lbm_amd, size, members, steps, warmup):
    """one repeat of the ensemble without statistics on the tree the child imports (the parent's has no set_stats): us per step"""
    sim = ensemble(lbm_amd, size, members, steps, warmup)
    sim.upload(None)
    sim.run_timed(warmup)
    sim.upload(None)
    us = sim.run_timed(steps) * 1e3 / steps
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
        print("stats_ab: the %s measurement did not end within %d s" % (what, args.timeout), file=sys.stderr)
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
    out = {"what": "plain", "this_us_per_step": spread(us["this"]), "parent_us_per_step": spread(us["parent"]),
           "this_repeats": [round(v, 3) for v in us["this"]], "parent_repeats": [round(v, 3) for v in us["parent"]]}
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
    ap.add_argument("--steps", type=int, default=1800, help="a multiple of 30: every setting ends on a sample point")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=150)
    ap.add_argument("--step-size", type=int, default=8192, help="the context of the step measurement is step-size squared")
    ap.add_argument("--step-steps", type=int, default=60)
    ap.add_argument("--step-warmup", type=int, default=6)
    ap.add_argument("--timeout", type=int, default=100, help="seconds one measuring child may take")
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its library built")
    ap.add_argument("--root", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_throughput.txt"), help="where the line is written ('' for nowhere)")
    ap.add_argument("--child", choices=WHATS + ["plain"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the parent never opens the device: it starts the measuring children, bounds each, and keeps their results
    result = {"tool": "stats_ab"}
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
        # what stands below the mark is written by hand (the kernel's registers, the comparison of the builds): keep it
        kept = ""
        if os.path.exists(args.out):
            text = open(args.out).read()
            if MARK in text:
                kept = "\n" + text[text.index(MARK):]
        shown = " ".join(a for a in sys.argv[1:] if not a.startswith("--out") and a != args.out)
        with open(args.out, "w") as f:
            f.write("Running statistics (lbm_dstats_*): tools/stats_ab.py on one device.\n\n"
                    "One process per measurement; one handle with the statistics off and on at every = 1, 3 and 30, HIP events around\n"
                    "the step loop, the four settings in turn within each repeat after a warm-up, every repeat restarts the flow from\n"
                    "the rest state.  Ensemble: a walled channel with a blocked disc, a sweep over omega, us/step for all members\n"
                    "together; off is three steps per launch, on is a run cut at its sample points.  Step: one context at\n"
                    "\"multistep\" 0; on at every = 1 less off is dp_stats_sample (and one accelerate launch) alone, against the\n"
                    "device's copy rate at 169 B per cell and sample.  Plain: the ensemble without statistics on this build and on a\n"
                    "build of the parent commit, one process per repeat, alternated.  Nothing is gated.\n")
            f.write("\n$ python tools/stats_ab.py %s\n%s\n%s" % (shown, line, kept))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Generates tests/golden/drive.json with the numpy float64 restatement of the body force (tests/_drive_ref.py): the recorded
figures of the three force-driven flows with exact answers, and of the sweep to steady state, that
tests/test_drive_restatement_cpu.py and tests/test_drive_gpu.py gate and compare against.  CPU only; nothing here touches the
library.  All runs start from rest at density 0.1 with accel = 0.

  poiseuille   8x11, walls on rows 0 and 10, periodic in x, F = (1e-6, 0), 20 000 steps: TRT at Lambda = 3/16 and 1/4 at omega
               0.6 / 1.0 / 1.7 / 1.9, BGK at 0.6 / 1.0 / 1.7: deviation from the parabola, density spread, max |u_y|
  hydrostatic  9x12, all four borders blocked, F = (0, -1e-4), 30 000 steps: TRT 3/16 at omega 1.0 and BGK at 1.7: max |u|, the
               largest relative error of a row-to-row density step against 3 F_y
  balance      24x15, walls on rows 0 and 14 and a 4x4 block, F = (2e-6, 0), 30 000 steps: TRT 3/16 at omega 1.0 and BGK at 1.4:
               the momentum-exchange force over all blocked cells against F_x N_fluid; and the TRT case with the force mirrored
  sweep        the balance grid, F_x = 1e-7 .. 8e-7, TRT 3/16 at omega 1.0, each member until
               |A(s) - A(s - 64)| <= 1e-7 |A(s)| on its av_vels at a multiple of 64 steps: the count, the final av_vels, and the
               spread of av_vels / F_x over the members

Usage (from the repository root; the runs are independent processes, about a minute on 8 cores; a second run writes the same
bytes):
    python tests/golden/make_drive.py"""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _drive_ref as ref  # noqa: E402
import _open_ref  # noqa: E402
from _force_ref import restatement  # noqa: E402

BGK_OMEGAS = (0.6, 1.0, 1.7)


def poiseuille_entry(omega, magic, steps=ref.POISEUILLE["steps"]):
    ob = ref.channel_mask(ref.POISEUILLE["nx"], ref.POISEUILLE["ny"])
    drive = ref.POISEUILLE["force"]
    dev, spread, uy = ref.state_figures("poiseuille", ref.run(ob, omega, magic, drive, steps), ob, omega, drive)
    return {"omega": omega, "magic": magic, "deviation": dev, "spread": spread, "uy": uy}


def hydrostatic_entry(omega, magic, steps=ref.HYDROSTATIC["steps"]):
    ob = ref.box_mask(ref.HYDROSTATIC["nx"], ref.HYDROSTATIC["ny"])
    drive = ref.HYDROSTATIC["force"]
    umax, err = ref.state_figures("hydrostatic", ref.run(ob, omega, magic, drive, steps), ob, omega, drive)
    return {"omega": omega, "magic": magic, "umax": umax, "step_error": err}


def balance_entry(omega, magic, sign=1.0, steps=ref.BALANCE["steps"]):
    """the force record's last entry: the force of the step that streams the state after steps - 1 steps"""
    ob = ref.balance_mask()
    drive = (sign * ref.BALANCE["force"][0], 0.0)
    fx, fy = restatement(ref.run(ob, omega, magic, drive, steps - 1), ob)[:2]
    rel, lift = ref.balance_figures(fx, fy, drive[0])
    return {"omega": omega, "magic": magic, "sign": sign, "fx": fx, "fy": fy, "rel": rel, "lift": lift}


def sweep_entry(f_x):
    """one member of the sweep under the av_vels criterion of lbm_dsteady_run, evaluated as the header writes it"""
    s = ref.SWEEP
    ob = ref.balance_mask()
    inv = 1.0 / float(np.count_nonzero(ob == 0))
    f = _open_ref.rest_state(ref.DENSITY, *ob.shape).copy()
    av = []
    while len(av) < s["max_steps"]:
        f, u = ref.step(f, ob, s["omega"], s["magic"], drive=(f_x, 0.0))
        av.append(float(np.sum(u)) * inv)
        n = len(av)
        if n % s["window"] == 0 and n - s["window"] >= 1 and abs(av[n - 1] - av[n - 1 - s["window"]]) <= s["rel_tol"] * abs(av[n - 1]):
            return {"f_x": f_x, "steps": n, "converged": True, "av": av[n - 1]}
    return {"f_x": f_x, "steps": len(av), "converged": False, "av": av[-1]}


def job(spec):
    return globals()[spec[0] + "_entry"](*spec[1:])


def build(workers=None):
    specs = [("poiseuille", w, m) for m in (ref.L316, ref.L14) for w in ref.POISEUILLE["omegas"]]
    specs += [("poiseuille", w, None) for w in BGK_OMEGAS]
    n_p = len(specs)
    specs += [("hydrostatic", w, m) for w, m in ref.HYDROSTATIC["cases"]]
    n_h = len(specs)
    specs += [("balance", w, m) for w, m in ref.BALANCE["cases"]] + [("balance", *ref.BALANCE["cases"][0], -1.0)]
    n_b = len(specs)
    specs += [("sweep", f) for f in ref.SWEEP["forces"]]
    with multiprocessing.Pool(workers or min(len(specs), os.cpu_count() or 1)) as pool:
        res = pool.map(job, specs, chunksize=1)
    balance, mirrored = res[n_h:n_b - 1], res[n_b - 1]
    total = ref.BALANCE["force"][0] * ref.BALANCE["fluid"]
    sweep = res[n_b:]
    ratio = np.array([e["av"] / e["f_x"] for e in sweep])
    return {"poiseuille": dict(ref.POISEUILLE, entries=res[:n_p]),
            "hydrostatic": dict(ref.HYDROSTATIC, entries=res[n_p:n_h]),
            "balance": dict(ref.BALANCE, entries=balance, mirrored=mirrored,
                            mirror_sum=abs(balance[0]["fx"] + mirrored["fx"]) / total),
            "sweep": dict(ref.SWEEP, entries=sweep, spread=float((ratio.max() - ratio.min()) / ratio.mean()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "drive.json"))
    ap.add_argument("--workers", type=int)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        json.dump(build(a.workers), f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates tests/golden/flows.json with the numpy float64 restatement (tests/_open_ref.py on tests/_trt_ref.py): the
recorded figures of the two flows of tests/_flows_ref.py that tests/test_flows_restatement_cpu.py and tests/test_flows_gpu.py
gate and compare against.  CPU only; nothing here touches the library.

  channel   the 32x11 channel, 12 000 steps from rest, omega 0.6 / 1.0 / 1.7 / 1.9 with BGK, Lambda = 3/16 and Lambda = 1/4:
            `shape` and `spread` of _open_ref.channel_figures, twelve entries
  cylinder  Schaefer-Turek 2D-1 with TRT at Lambda = 3/16, at D = 10 (40 000 steps) and D = 20 (until settled, below):
            F_x, F_y and the sum of |link terms| of _open_ref.force every 250 steps (C = coefficients(F) of _flows_ref),
            the figures of the last 6 000 steps taken over every step, and at D = 10 the same of the mirrored case with the
            two differences between a case and its mirror image

Entry t of a force list belongs to the state after t steps: it is what the library's record holds at index t.

D = 20 runs until max - min of C_d over the last 6 000 steps is at most 0.2 % of their mean, looked at every 2 000 steps from
step 20 000 on, and to D20_CAP at the most; the count goes into the fixture as "steps" and the outcome as "settled".

Usage (from the repository root; the runs are independent processes, and the D = 20 run alone, 68 000 steps, takes the eight
to nine minutes that the whole takes on 8 cores; a second run writes the same bytes):
    python tests/golden/make_flows.py [--records DIR]
--records keeps every step's F_x and F_y of the cylinder runs as DIR/cylinder_<D>[_mirrored].npy, for choosing a window."""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _flows_ref as flows  # noqa: E402
import _open_ref  # noqa: E402
import _trt_ref  # noqa: E402

EVERY, TAIL = 250, 6000
D10_STEPS = 40000
D20_FROM, D20_LOOK, D20_CAP, SETTLED = 20000, 2000, 120000, 2e-3
MAGICS = (None, 3.0 / 16.0, 0.25)


def channel_entry(omega, magic, steps=flows.CH_STEPS):
    ob = flows.channel_mask()
    u_in = _open_ref.poiseuille(flows.CH_NY, flows.CH_U)
    om = None if magic is None else _trt_ref.omega_minus(omega, magic)
    f = _open_ref.rest_state(flows.DENSITY, flows.CH_NY, flows.CH_NX).copy()
    with np.errstate(all="ignore"):                       # BGK at omega 1.9 diverges: its figures are NaN
        for _ in range(steps):
            f = _open_ref.step(f, ob, omega, om, u_in, flows.DENSITY)[0]
        spread, shape = _open_ref.channel_figures(f, flows.CH_U)
    fin = np.isfinite(spread) and np.isfinite(shape)
    return {"omega": omega, "magic": magic, "spread": spread if fin else None, "shape": shape if fin else None}


def tail_figures(fx, fy, D, steps):
    """the figures of the record's last TAIL entries, fx[steps - TAIL:steps]"""
    cd, cl = flows.coefficients(fx[steps - TAIL:steps], fy[steps - TAIL:steps], D)
    return {"first": steps - TAIL, "cd_mean": float(cd.mean()), "cd_min": float(cd.min()), "cd_max": float(cd.max()),
            "cl_mean": float(cl.mean()), "cl_min": float(cl.min()), "cl_max": float(cl.max())}


def cylinder_run(D, mirror=False, steps=None, records=None):
    """steps None: until settled.  Returns the fixture's entry; `steps` steps are taken and steps + 1 forces computed, the last
    one what force() gives after the run."""
    case = flows.cylinder_channel(D)
    if mirror:
        case = flows.mirrored(case)
    cap = D20_CAP if steps is None else steps
    fx, fy, mag = np.zeros(cap + 1), np.zeros(cap + 1), np.zeros(cap + 1)
    f = flows.rest(case)
    t, links, settled = 0, 0, None
    while True:
        fx[t], fy[t], links, mag[t] = flows.force(f, case)
        if steps is None and t >= D20_FROM and t % D20_LOOK == 0:
            fig = tail_figures(fx, fy, D, t)
            settled = (fig["cd_max"] - fig["cd_min"]) <= SETTLED * fig["cd_mean"]
            print("D %d step %d: C_d %.4f .. %.4f" % (D, t, fig["cd_min"], fig["cd_max"]), flush=True)
            if settled:
                break
        if t == cap:
            break
        f = flows.step(f, case)
        t += 1
    n = t
    if records:
        np.save(os.path.join(records, "cylinder_%d%s.npy" % (D, "_mirrored" if mirror else "")), np.stack([fx[:n + 1], fy[:n + 1]]))
    at = np.arange(0, n + 1, EVERY)
    out = {"D": D, "nx": case["nx"], "ny": case["ny"], "omega": case["omega"], "steps": n, "every": EVERY, "links": links,
           "fx": fx[at].tolist(), "fy": fy[at].tolist(), "mag": mag[at].tolist(), "tail": tail_figures(fx, fy, D, n)}
    if settled is not None:
        out["settled"] = bool(settled)
    return out


def job(spec):
    t0 = time.time()
    kind, args = spec[0], spec[1:]
    out = channel_entry(*args) if kind == "channel" else cylinder_run(*args)
    print("%s %s: %.0f s" % (kind, args[:2], time.time() - t0), flush=True)
    return out


def build(records=None, workers=None):
    specs = [("cylinder", 20, False, None, records), ("cylinder", 10, False, D10_STEPS, records),
             ("cylinder", 10, True, D10_STEPS, records)]
    specs += [("channel", omega, magic) for omega in flows.CH_OMEGAS for magic in MAGICS]
    with multiprocessing.Pool(workers or min(len(specs), os.cpu_count() or 1)) as pool:
        res = pool.map(job, specs, chunksize=1)
    d20, d10, d10m = res[:3]
    a, b = d10["tail"], d10m["tail"]
    d10["mirrored"] = {"tail": b, "d_cd": abs(a["cd_mean"] - b["cd_mean"]), "d_cl": abs(a["cl_mean"] + b["cl_mean"])}
    return {"channel": {"nx": flows.CH_NX, "ny": flows.CH_NY, "u_max": flows.CH_U, "steps": flows.CH_STEPS, "entries": res[3:]},
            "cylinder": {"10": d10, "20": d20}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records")
    ap.add_argument("--out", default=os.path.join(HERE, "flows.json"))
    ap.add_argument("--workers", type=int)
    a = ap.parse_args()
    if a.records:
        os.makedirs(a.records, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(build(a.records, a.workers), f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

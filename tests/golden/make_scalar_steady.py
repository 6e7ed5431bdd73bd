#!/usr/bin/env python3
"""Writes tests/golden/scalar_steady.json from the numpy restatement (tests/_scalar_record_ref.py): for the two sweeps that the
steady runs of tests/test_scalar_record_gpu.py stop on, the stops that _steady_rule.rule finds on the record of a plain run to the
cap, and the first START entries of the first member's three records, which tests/test_scalar_record_restatement_cpu.py
recomputes; and the convective Nusselt number of _buoy_ref.CAVITY from the last entry of flux_x.  A minute or two of numpy; run
from the repository root:

    python tests/golden/make_scalar_steady.py"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _buoy_ref as bref  # noqa: E402
import _scalar_record_ref as rr  # noqa: E402
import _scalar_ref as sref  # noqa: E402


def sweep(name, settings, values, records_of):
    records = [records_of(v, settings["cap"]) for v in values]
    steps, conv = rr.stops(records, settings)
    out = {"members": list(values), "window": settings["window"], "rel_tol": settings["rel_tol"], "cap": settings["cap"],
           "which": settings["which"], "stops": [int(s) for s in steps], "converged": [bool(c) for c in conv], "start": rr.START,
           "first": {n: [float(v) for v in records[0][i, :rr.START]] for i, n in enumerate(rr.NAMES)},
           "last": [[float(r[i, int(s) - 1]) for i in range(3)] for r, s in zip(records, steps)]}
    print(name, out["stops"], out["converged"])
    return out


def main():
    out = {"box": sweep("box", rr.BOX, rr.BOX["Ras"], rr.box_records),
           "channel": sweep("channel", rr.CHANNEL, rr.CHANNEL["Ds"], rr.channel_records)}
    C = bref.CAVITY
    cs = bref.cavity()
    f, g = cs.f0, sref.init(cs.c0)
    for _ in range(C["steps"] - 1):
        f, g = bref.advance(f, g, cs.s)[:2]
    f, g, rec = rr.buoyant_advance(f, g, cs.s)[:3]
    nu = rr.nusselt_convective(rec[1], cs.s.ob, C["H"], cs.s.D)
    out["cavity"] = {"Ra": C["Ra"], "steps": C["steps"], "flux_x": float(rec[1]), "nusselt": nu, "theory": C["theory"],
                     "deviation": abs(nu / C["theory"] - 1.0), "wall_nusselt": bref.nusselt(sref.field(g, cs.s.ob))}
    print("cavity", out["cavity"])
    with open(rr.GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/buoy.json from the numpy restatement (tests/_buoy_ref.py): the figures of the three flows with known
answers at full length, their histories, and the probes of every flow after _buoy_ref.START steps, which
tests/test_buoy_restatement_cpu.py recomputes.  A few minutes of numpy; run from the repository root:

    python tests/golden/make_buoy.py"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _buoy_ref as bref  # noqa: E402


def main():
    out = {"start": bref.START, "probes": {}}
    for name, make in bref.SHORT.items():
        cs = make()
        f, g, _ = bref.run(cs, bref.START)
        out["probes"][name] = bref.probes(f, g, cs.s)

    L = bref.LAYER
    cs = bref.layer(L["Ra"])
    every = list(range(1000, L["steps"] + 1, 1000))
    _, _, seen = bref.run(cs, L["steps"], every)
    out["rest"] = {"Ra": L["Ra"], "steps": L["steps"], "history": {str(n): bref.max_uy(seen[n][1][1], cs.s.ob) for n in every},
                   "max_uy": bref.max_uy(seen[L["steps"]][1][1], cs.s.ob), "profile": bref.sref.walls_figure(seen[L["steps"]][0])}
    print("rest", out["rest"])

    O = bref.ONSET
    amps = []
    for Ra in O["Ras"]:
        cs = bref.layer(Ra, O["eps"])
        _, _, seen = bref.run(cs, O["steps"], (O["t0"], O["steps"]))
        amps.append([bref.max_uy(seen[n][1][1], cs.s.ob) for n in (O["t0"], O["steps"])])
    r0, r1, ra_c = bref.onset_figures([a[0] for a in amps], [a[1] for a in amps])
    out["onset"] = {"Ras": list(O["Ras"]), "amplitudes": amps, "rates": [r0, r1], "Ra_c": ra_c, "theory": O["theory"],
                    "deviation": abs(ra_c / O["theory"] - 1.0)}
    print("onset", out["onset"])

    C = bref.CAVITY
    cs = bref.cavity()
    every = list(range(2500, C["steps"] + 1, 2500))
    _, _, seen = bref.run(cs, C["steps"], every)
    nu = bref.nusselt(seen[C["steps"]][0])
    out["cavity"] = {"Ra": C["Ra"], "Pr": C["Pr"], "steps": C["steps"], "history": {str(n): bref.nusselt(seen[n][0]) for n in every},
                     "nusselt": nu, "theory": C["theory"], "deviation": abs(nu / C["theory"] - 1.0),
                     "max_u": float(np.max(seen[C["steps"]][1][2]))}
    print("cavity", out["cavity"])

    with open(bref.GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates tests/golden/scalar.json with the numpy float64 restatement of the passive scalar (tests/_scalar_ref.py): the recorded
figures of the flows with known answers that tests/test_scalar_restatement_cpu.py and tests/test_scalar_gpu.py gate and compare
against.  CPU only; nothing here touches the library.  Density 0.1 throughout; the runs are _scalar_ref.RUNS:

  conservation  32x32, periodic, insulating obstacles, accel 0.005, D = 0.05, 200 steps: the largest relative drift of the sum of
                the field over the fluid cells, looked at every 50 steps
  diffusion     32x32 at rest, c0 = 1 + 0.5 sin(kx) cos(ky), 200 steps, D = 0.02 / 0.05 / 0.2: the decay rate fitted to the mode's
                amplitude every 20 steps, against 2 D k^2
  walls         4x18 at rest, rows 0 and 17 held at 1 and 0, D = 0.02 / 0.1 / 1/6 / 0.3, 8 16^2 / D steps: the largest deviation
                from the straight profile
  open          64x4, inlet 0.05 and the uniform equilibrium, c_in = 1, D = 0.01 / 0.05, 6000 steps: max |C - 1|
  taylor        1024x18, TRT at 3/16, a body force for a mean velocity of 0.05, 6000 steps of flow, then a Gaussian (sigma 6) at
                D = 0.08: the effective diffusivity between steps 9600 and 16000 over D (1 + Pe^2 / 210), the speed of the centre
                over 0.05, and the flow's deviation from the parabola at the release

Every entry also holds `start`: _scalar_ref.probe of the field after the first 200 steps of the run's own setup with the scalar on
from step 0 (taylor: from rest, without its spin-up), which the CPU module recomputes.

Usage (from the repository root; the runs are independent processes, a few minutes on 8 cores, the longest is walls at D = 0.02; a
second run writes the same bytes):
    python tests/golden/make_scalar.py"""
import argparse
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _scalar_ref as ref  # noqa: E402


def entry(spec):
    kind, D = spec
    cs = ref.case(kind, D)
    start = ref.probe(ref.run(cs, steps=ref.START, spin_up=0)[2])
    f, seen, _ = ref.run(cs)
    out = dict(ref.figures(kind, cs, seen), kind=kind, D=cs.D, steps=cs.steps, start=start)
    if kind == "taylor":
        # the flow at the release: the state after the spin-up alone
        spun = cs.f0
        for _ in range(cs.spin_up):
            spun = ref.flow_step(ref.streamed(spun, cs.fl), cs.fl)
        u_x, _, _, pressure = ref._drive_ref.fields(spun, cs.ob, ref.DENSITY, cs.fl.drive)
        out["parabola_deviation"] = ref.taylor_parabola_deviation(u_x, pressure)
        out["moments"] = [list(ref.taylor_moments(seen[t], t)) for t in sorted(seen)]
    return out


def build(workers=None):
    with multiprocessing.Pool(workers or min(len(ref.RUNS), os.cpu_count() or 1)) as pool:
        res = pool.map(entry, ref.RUNS, chunksize=1)
    return {"start_steps": ref.START, "entries": res,
            "settings": {"conservation": ref.CONSERVATION, "diffusion": ref.DIFFUSION, "walls": ref.WALLS, "open": ref.OPEN,
                         "taylor": ref.TAYLOR}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "scalar.json"))
    ap.add_argument("--workers", type=int)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        json.dump(build(a.workers), f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

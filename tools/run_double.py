#!/usr/bin/env python3
"""The reference's command line in double precision: `tools/run_double.py <paramfile> <obstaclefile>` runs the input on a
double-precision context (lbm_amd.LBMDouble) and writes av_vels.dat and final_state.dat into the working directory in the
reference's formats, then prints the ==done== block (d2q9-bgk.c:271-275).  `make check`'s comparison (check/check.py)
applies to its files as to the fp32 host's."""
import os
import resource
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv):
    if len(argv) != 3:
        sys.stderr.write("Usage: %s <paramfile> <obstaclefile>\n" % argv[0])
        return 1
    import lbm_amd
    params, obstacles = lbm_amd.read_inputs_double(argv[1], argv[2])
    tic = time.time()
    with lbm_amd.LBMDouble(params, obstacles) as sim:
        sim.upload(None)
        loop_ms = sim.run_timed(params.max_iters)
        reynolds = sim.reynolds()
        sim.write_values("final_state.dat", "av_vels.dat")
    toc = time.time()
    ru = resource.getrusage(resource.RUSAGE_SELF)
    lu = float(params.nx) * params.ny * params.max_iters
    print("==done==")
    print("Reynolds number:\t\t%.12E" % reynolds)
    print("Elapsed time:\t\t\t%.6f (s)" % (toc - tic))
    print("Elapsed user CPU time:\t\t%.6f (s)" % ru.ru_utime)
    print("Elapsed system CPU time:\t%.6f (s)" % ru.ru_stime)
    print("Step loop time:\t\t\t%.6f (s)" % (loop_ms * 1e-3))
    print("MLUPS (step loop, fp64):\t%.1f" % (lu / (loop_ms * 1e-3) / 1e6))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

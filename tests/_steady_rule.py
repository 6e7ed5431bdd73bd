"""The steady-run rule of include/lbm.h in numpy float64 and the channel sweep it is applied to: what tests/test_dp_steady_gpu.py
and every module with a run_until test share.  The wanted stops of a steady run never come from run_until: they are `rule` on
the record of a plain run to the cap."""
import numpy as np

TOL, CAP = 2e-2, 400
OMEGAS = {4: (0.6, 1.0, 1.4, 1.7), 24: tuple(float(v) for v in np.linspace(0.6, 1.7, 24))}


def channel(nx, ny):
    """rows 0 and ny-1 blocked plus a 4x4 block"""
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    ob[ny // 2 - 2:ny // 2 + 2, nx // 4:nx // 4 + 4] = 1
    return ob


def sweep(lbm, nx, ny, omegas, max_iters=CAP):
    ob = channel(nx, ny)
    base = lbm.make_dparams(nx, ny, max_iters, density=0.1, accel=0.005, omega=omegas[0], obstacles=ob)
    return lbm.sweep_dparams(base, omega=list(omegas)), ob


def rule(av, s0, max_steps, window, rel_tol):
    """the header's criterion on a downloaded record av float64[n, >= s0 + max_steps]: (steps, converged)"""
    assert av.dtype == np.float64
    n = av.shape[0]
    steps, conv = np.full(n, s0 + max_steps, dtype=np.int32), np.zeros(n, dtype=bool)
    for m in range(n):
        for s in range(s0 + window, s0 + max_steps + 1, window):
            if s - window < 1:
                continue
            a_now, a_then = av[m, s - 1], av[m, s - window - 1]
            diff = np.abs(a_now - a_then)
            bound = np.float64(rel_tol) * np.abs(a_now)
            if diff <= bound:   # False for a NaN on either side
                steps[m], conv[m] = s, True
                break
    return steps, conv

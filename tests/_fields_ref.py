"""The output stage restated in numpy float64, the states the output-stage tests run on, and their case tables.

fields() is written from the formulas, not from the oracle's C: for a cell with distributions f0..f8

    rho = f0 + ... + f8
    u_x = ((f1 + f5 + f8) - (f3 + f6 + f7)) / rho          u_y = ((f2 + f5 + f6) - (f4 + f7 + f8)) / rho
    u   = sqrt(u_x^2 + u_y^2)                               pressure = rho / 3

a blocked cell reports 0, 0, 0 and density / 3; the mean speed is the sum of u over the free cells divided by their number;
Reynolds number = mean speed * reynolds_dim / viscosity with viscosity = (2 / omega - 1) / 6; the total density is the sum of
all 9 nx ny distributions.  tests/test_output_stage_cpu.py holds it against the fp64 oracle at 1e-13.

state() builds the inputs: the positive perturbed rest state of random_case (tests/test_gpu_parity.py) scaled to the case's
density (20 % perturbation: speeds of order 1e-2), 8 % random obstacles, one fully blocked row, and blocked cells on the first
and the last row of every slab of the case's row partition.

oracle_spreads() measures how far the fp32 oracle's own output arithmetic lands from fields() on a state the fp32 oracle
itself has advanced: that distance, times GATE_FACTOR, is what tests/test_output_stage_gpu.py allows the GPU."""
import numpy as np

W = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float64).reshape(9, 1, 1)
DENSITY, OMEGA, REYNOLDS_DIM, ACCEL = 0.37, 1.4, 7, 0.005      # every case but "... defaults" runs at these
DEFAULTS = dict(density=0.1, omega=1.85, reynolds_dim=10)
GATE_FACTOR = 4.0                 # the margin of the forcing-guard tests (ORACLE_FORMS_FACTOR of tests/test_dp_gpu.py)
RE_FLOOR = 16 * 2.0 ** -24        # Reynolds number: never a gate below this
PRESSURE_F32 = 10 * 2.0 ** -24    # nine fp32 additions and one multiply
PRESSURE_F64 = 10 * 2.0 ** -53
F64_GATE = 1e-12                  # velocities and Reynolds number of the fp64 forms
FIELD_STEPS = 9                   # section (a): steps before the state is downloaded


def fields(cells, obstacles, density, omega, reynolds_dim):
    """dict of u_x, u_y, u, pressure (float64[ny, nx]), mean_u, reynolds, total_density from cells[9, ny, nx]; density and
    omega as the context holds them (an fp32 context: the float32 values)"""
    f = np.asarray(cells, dtype=np.float64)
    free = np.asarray(obstacles) == 0
    rho = f.sum(axis=0)
    safe = np.where(free, rho, 1.0)
    u_x = np.where(free, ((f[1] + f[5] + f[8]) - (f[3] + f[6] + f[7])) / safe, 0.0)
    u_y = np.where(free, ((f[2] + f[5] + f[6]) - (f[4] + f[7] + f[8])) / safe, 0.0)
    u = np.sqrt(u_x * u_x + u_y * u_y)
    pressure = np.where(free, rho / 3.0, float(density) / 3.0)
    nfree = int(np.count_nonzero(free))
    mean_u = float(u[free].sum()) / nfree if nfree else 0.0
    viscosity = (2.0 / float(omega) - 1.0) / 6.0
    return {"u_x": u_x, "u_y": u_y, "u": u, "pressure": pressure, "mean_u": mean_u,
            "reynolds": mean_u * reynolds_dim / viscosity, "total_density": float(f.sum())}


def slab_rows(ny, nslabs, index):
    """(first row, row count) of slab `index`: contiguous rows, sizes differ by at most one (the library's split_rows)"""
    base, rem = divmod(ny, nslabs)
    return index * base + min(index, rem), base + (1 if index < rem else 0)


def state(nx, ny, seed, density=DENSITY, nslabs=1, real=np.float32, blocked=0.08):
    """(obstacles int32[ny, nx], cells real[9, ny, nx])"""
    rng = np.random.default_rng(seed)
    ob = (rng.random((ny, nx)) < blocked).astype(np.int32)
    cells = W * density * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5))
    ob[ny // 2, :] = 1
    for i in range(nslabs):
        y0, rows = slab_rows(ny, nslabs, i)
        for y in (y0, y0 + rows - 1):
            if y != ny // 2:
                ob[y, rng.integers(0, nx, size=max(1, nx // 16))] = 1
    assert 0 < np.count_nonzero(ob) < ob.size
    return ob, np.ascontiguousarray(cells.astype(real))


def case(nx, ny, seed, nslabs=1, density=DENSITY, omega=OMEGA, reynolds_dim=REYNOLDS_DIM, accel=ACCEL):
    return dict(nx=nx, ny=ny, seed=seed, nslabs=nslabs, density=density, omega=omega, reynolds_dim=reynolds_dim, accel=accel)


def inputs(c, real=np.float32):
    return state(c["nx"], c["ny"], c["seed"], c["density"], c["nslabs"], real)


# ---- section (a): fields and Reynolds number ------------------------------------------------------------------------------
# one slab: 3x3, 5x4, 30x17 scalar path; 132x40, 260x7 vector path without wave modes; 256x3, 512x24 wave modes; 1030x511 and
# 1024x520 reach the second trip of the output kernel's grid-stride loop (2048 workgroups of 256: above 524 288 cells)
ONE_SLAB = {
    "3x3": case(3, 3, 1), "5x4": case(5, 4, 2), "30x17": case(30, 17, 3), "132x40": case(132, 40, 4), "260x7": case(260, 7, 5),
    "256x3": case(256, 3, 6), "512x24": case(512, 24, 7), "1030x511": case(1030, 511, 8), "1024x520": case(1024, 520, 9),
    "132x40 defaults": case(132, 40, 10, **DEFAULTS),
}
SLABS = {
    "256x16 / 2": case(256, 16, 11, 2), "256x67 / 4": case(256, 67, 12, 4), "256x50 / 8": case(256, 50, 13, 8),
    "256x128 / 5": case(256, 128, 14, 5), "130x50 / 3": case(130, 50, 15, 3),
}
# ensemble members: constants and obstacle map of their own
MEMBER_CONSTANTS = [(0.37, 1.4, 7), (0.1, 1.85, 10), (0.21, 1.3, 3), (0.5, 1.2, 12), (0.8, 1.0, 5)]
ENSEMBLES = {
    "37x29": [case(37, 29, 20 + m, density=d, omega=o, reynolds_dim=r) for m, (d, o, r) in enumerate(MEMBER_CONSTANTS)],
    "128x128": [case(128, 128, 30 + m, density=d, omega=o, reynolds_dim=r) for m, (d, o, r) in enumerate(MEMBER_CONSTANTS)],
}
DOUBLE = {"127x129": case(127, 129, 40), "1030x511": case(1030, 511, 41)}
DOUBLE_ENSEMBLE = [case(37, 29, 50 + m, density=d, omega=o, reynolds_dim=r) for m, (d, o, r) in enumerate(MEMBER_CONSTANTS[:3])]
# 272x256: 256 x ceil(272 / 16) = 4352 row segments a step, the smallest convenient grid above the 4096 up to which the fp64
# families add a step's segments in one stage: two blocks, then one (section (b) only)
DOUBLE_TWO_STAGE = case(272, 256, 42)
DOUBLE_ENSEMBLE_TWO_STAGE = [case(272, 256, 53 + m, density=d, omega=o, reynolds_dim=r) for m, (d, o, r) in enumerate(MEMBER_CONSTANTS[:2])]
# the ragged ensemble: the channel sweep of tests/test_steady_gpu.py from rest (stops 208 / 304 / 400 / 400 on the fp32 oracle)
RAGGED = dict(nx=48, ny=32, omegas=(0.6, 1.0, 1.4, 1.7), window=16, rel_tol=2e-2, max_steps=400, density=0.1, accel=0.005,
              reynolds_dim=10)

# ---- section (b): the last av_vels entry ---------------------------------------------------------------------------------
# name -> (case, steps of the run, which ends a launch set of the family)
AV_SINGLE = {"512x24": (ONE_SLAB["512x24"], 9), "30x17": (ONE_SLAB["30x17"], 9)}
AV_CASES = {
    "256x37": (case(256, 37, 60), 8),            # fuse 1 / 3 / 4 with chunk 5: 4, 6 and 8 steps
    "512x64": (case(512, 64, 61), 8),            # deep lone and twin, fuse 8
    "1024x50": (case(1024, 50, 62), 5),          # five-step chunk pairs
    "33x17": (case(33, 17, 63), 8), "130x31": (case(130, 31, 64), 8),      # LDS tiles, 8 steps per launch
    "132x64": (case(132, 64, 65), 7), "128x6": (case(128, 6, 66), 7),      # resident
    "256x67 / 4": (SLABS["256x67 / 4"], 8),      # slabs: multi8 (8 steps), fused3 (6), fuse 8 asked for (8)
    "256x64 / 2": (case(256, 64, 67, 2), 8),     # slabs that the deep window kernel takes (32 rows each)
    "127x129": (DOUBLE["127x129"], 8),
}


def ragged_channel(nx, ny):
    """rows 0 and ny-1 blocked plus a 4x4 block (channel() of tests/test_steady_gpu.py)"""
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    ob[ny // 2 - 2:ny // 2 + 2, nx // 4:nx // 4 + 4] = 1
    return ob


def max_speed(ref):
    return float(np.max(ref["u"]))


def field_errors(got, ref, obstacles):
    """(u_x, u_y, u: max absolute error over the largest speed of the case; pressure: max relative error on the free cells)
    of four columns against fields()"""
    top = max_speed(ref)
    free = np.asarray(obstacles) == 0
    out = {k: float(np.max(np.abs(np.asarray(g, dtype=np.float64) - ref[k]))) / top for k, g in zip(("u_x", "u_y", "u"), got)}
    pr = np.asarray(got[3], dtype=np.float64)
    out["pressure"] = float(np.max(np.abs(pr[free] - ref["pressure"][free]) / ref["pressure"][free]))
    return out


def oracle_steps(orc, c, ob, cells0, nsteps):
    """`orc` advanced one step at a time: yields (t, av_vels of step t as the oracle records it, state after t steps)"""
    p = orc.make_params(c["nx"], c["ny"], max(nsteps, 1), c["reynolds_dim"], c["density"], c["accel"], c["omega"])
    orc.set_obstacles(p, ob)
    cells = np.array(cells0, dtype=orc.real, copy=True)
    tmp = np.empty_like(cells)
    for t in range(1, nsteps + 1):
        orc.accelerate_flow(p, cells, ob)
        av = orc.timestep(p, cells, tmp, ob)
        cells, tmp = tmp, cells
        yield t, av, cells


_spreads = {}


def oracle_spreads(oracles, c, nsteps, ob=None, cells0=None, av_window=None):
    """the fp32 oracle's distance from fields() on states it has advanced itself; the largest over `oracles` (its forms) of
         u_x, u_y, u   max |oracle_final_fields - fields| over the case's largest speed, after nsteps
         reynolds      |oracle_calc_reynolds / fields - 1| after nsteps
         av            |av_vels[t - 1] / mean speed of the state after t steps - 1|, the largest over t = 1 .. nsteps
                       (av_window k: over the last k steps only)
    The av_vels entry of a step is the sum over the free cells of |j| / rho before the collision and the state holds the
    distributions after it: the two differ by the rounding of nine stores per cell, and the record is rounded to fp32 once
    more.  One such difference can come out arbitrarily close to zero, so the spread of a case is the largest over its steps
    and over the oracle's forms, never a single sample."""
    key = (tuple(id(o) for o in oracles), tuple(sorted(c.items())), nsteps, av_window, ob is None)
    if key in _spreads and ob is None:
        return _spreads[key]
    if ob is None:
        ob, cells0 = inputs(c)
    out = {"u_x": 0.0, "u_y": 0.0, "u": 0.0, "reynolds": 0.0, "av": 0.0}
    density, omega = np.float32(c["density"]), np.float32(c["omega"])
    for orc in oracles:
        for t, av, cells in oracle_steps(orc, c, ob, cells0, nsteps):
            if av_window is not None and t <= nsteps - av_window:
                continue
            ref = fields(cells, ob, density, omega, c["reynolds_dim"])
            out["av"] = max(out["av"], abs(av / ref["mean_u"] - 1.0))
            if t == nsteps and orc is oracles[0]:      # (the output arithmetic has one form: the other forms restate the step only)
                p = orc.make_params(c["nx"], c["ny"], nsteps, c["reynolds_dim"], c["density"], c["accel"], c["omega"])
                orc.set_obstacles(p, ob)
                last = np.ascontiguousarray(cells)
                err = field_errors(orc.final_fields(p, last, ob), ref, ob)
                for k in ("u_x", "u_y", "u"):
                    out[k] = max(out[k], err[k])
                out["reynolds"] = max(out["reynolds"], abs(orc.reynolds(p, last, ob) / ref["reynolds"] - 1.0))
    if key[-1]:
        _spreads[key] = out
    return out


def gates(spread):
    """what the GPU may differ from fields() by: GATE_FACTOR times the oracle's spread; the Reynolds number's has a floor"""
    g = {k: GATE_FACTOR * spread[k] for k in ("u_x", "u_y", "u", "av")}
    g["reynolds"] = max(GATE_FACTOR * spread["reynolds"], RE_FLOOR)
    return g

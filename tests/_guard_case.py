"""Inputs on which the forcing guard refuses, and an audit of what the oracle's guard decides on them.

accelerate_flow (kernels.cl:24-42) forces a free cell of row ny-2 only if f3 - aw1 > 0, f6 - aw2 > 0 and f7 - aw2 > 0
(aw1 = density*accel/9, aw2 = density*accel/36).  On the states the other tests use, f3 is two hundred times aw1 and the
guard never says no.  guard_case() builds states on which it says no in part of the row at every step:

  * density 0.37, accel 0.2, omega 1.4: three constants off their defaults at once.  The update is homogeneous in f, so the
    density only scales the state; accel 0.2 puts the thresholds at a fifth of the rest values; omega 1.4 keeps the state
    finite for the few dozen steps the tests run (at 1.85 the same states reach 1e5 by step 15);
  * the perturbed rest state of the other tests, multiplied by a smooth dip to a tenth around the forcing row, centred on
    x = nx/2 and on x = 0 across the periodic wrap: inside the dips all three clauses refuse, on their flanks one or two do;
  * overwritten cells of the forcing row with one of f3 / f6 / f7 at half its threshold and the other two at twice theirs
    (each clause refuses alone at step 0), and cells with all three at twice their thresholds (accepted cells inside the dips);
  * pairs of spikes that the first streaming step brings together in a forcing-row cell: 1.4 * f_eq - 0.4 * f is negative
    for f above about 3.5 f_eq, so the cell comes out of the first collision with exactly one of f3 / f6 / f7 below zero and
    that clause refuses alone at step 1 (the opposite spike cancels the momentum that would otherwise lift f_eq with f).

guard_audit() steps an oracle one step at a time and records what its guard decided; tests/test_forcing_guard_cpu.py holds
the conditions every case must meet before a GPU comparison on it means anything (wide margins, the same decisions in every
oracle form), tests/test_forcing_guard_gpu.py runs the kernels on them."""
import numpy as np

W = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float64).reshape(9, 1, 1)
DENSITY, ACCEL, OMEGA = 0.37, 0.2, 1.4
CLAUSES = (3, 6, 7)
# the speed opposite to each guarded one, and where the first pull-stream gathers the pair from: (dx, dy) of the source cell
OPPOSITE = {3: 1, 6: 8, 7: 5}
SOURCE = {1: (-1, 0), 3: (1, 0), 5: (-1, -1), 6: (1, -1), 7: (1, 1), 8: (-1, 1)}
SPIKE = {3: 16.0, 6: 6.0, 7: 6.0}   # 1.4 * (1 + 2 (s - 1) w) - 0.4 s < 0.2 needs s > 10 on the axes (w = 1/9), s > 3.5 on the diagonals


def raised_cosine(d, half):
    return np.where(np.abs(d) < half, 0.5 * (1.0 + np.cos(np.pi * d / half)), 0.0)


def dip(nx, ny, hy=16, hx=48, depth=0.1):
    """the factor field: `depth` at (nx/2, ny-2) and at (0, ny-2), 1 away from them; raised cosines of half-width hy rows
    (on grids of fewer than 24 rows: the same in every row) and hx columns (at most a sixth of the row)"""
    hy, hx = (min(hy, ny // 3) if ny >= 24 else 10 * ny), min(hx, max(4, nx // 6))
    y, x = np.arange(ny), np.arange(nx)
    dy = (y - (ny - 2) + ny // 2) % ny - ny // 2
    dxc = x - nx // 2
    dxw = (x + nx // 2) % nx - nx // 2
    b = raised_cosine(dy, hy)[:, None] * np.maximum(raised_cosine(dxc, hx), raised_cosine(dxw, hx))[None, :]
    return np.exp(np.log(depth) * b)


def thresholds(density, accel, real):
    """aw1, aw2 as the kernels and the oracle form them, in their own precision"""
    d, a = real(density), real(accel)
    return d * a / real(9), d * a / real(36)


def guard_case(nx, ny, seed, blocked=0.08, nsteps=19, real=np.float32, density=DENSITY, accel=ACCEL, omega=OMEGA,
               hy=16, hx=48, walls=False, open_top=False):
    """(density, accel, omega, obstacles int32[ny, nx], cells0 real[9, ny, nx]); nsteps is how long the caller means to run
    the state: it does not shape it, the recipe is only known to live a few dozen steps (the CPU file checks each case).
    walls: columns 0 and nx-1 blocked (a cavity's side walls); open_top: rows ny-4 .. ny-1 free of blocked cells"""
    assert nx >= 24 and ny >= 5 and nsteps <= 32
    rng = np.random.default_rng(seed)
    ob = (rng.random((ny, nx)) < blocked).astype(np.int32)
    cells = W * density * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5)) * dip(nx, ny, hy, hx)[None]
    if open_top:      # no blocked cell in the forcing row and its neighbours: waves there take the obstacle-free collision path
        ob[ny - 4:, :] = 0
    row = ny - 2
    aw1, aw2 = (float(v) for v in thresholds(density, accel, real))
    aw = {3: aw1, 6: aw2, 7: aw2}

    def overwrite(x, low):
        ob[row, x] = 0
        for k in CLAUSES:
            cells[k, row, x] = (0.5 if k == low else 2.0) * aw[k]

    # step 0, each clause alone: one cell left of the wrap, one right of it (the last and the first wave), one in a lane
    # pair with an accepted cell in the middle of the row; accepted cells inside both dips
    left, right, mid = (nx - 2, nx - 3, nx - 4), (1, 2, 3), (nx // 2 + 2, nx // 2 + 4, nx // 2 + 6)
    for i, k in enumerate(CLAUSES):
        overwrite(left[i], k)
        overwrite(right[i], k)
        overwrite(mid[i], k)
        overwrite(mid[i] + 1, None)
    overwrite(nx - 1, None)
    overwrite(0, None)
    overwrite(4, None)
    overwrite(nx - 5, None)
    # step 1, each clause alone: a spike and its opposite, gathered by a free forcing-row cell on the flat part of the state
    quarter = nx // 4
    for i, k in enumerate(CLAUSES):
        for x in (quarter + 3 * i - 3, nx - quarter + 3 * i - 3):
            ob[row, x] = 0
            for s in (k, OPPOSITE[k]):
                dx, dy = SOURCE[s]
                cells[s, (row + dy) % ny, (x + dx) % nx] *= SPIKE[k]
    if walls:
        ob[:, 0] = ob[:, -1] = 1
    return density, accel, omega, ob, np.ascontiguousarray(cells.astype(real))


def guard_audit(oracle, density, accel, omega, obstacles, cells0, nsteps, keep=()):
    """steps `oracle` with accelerate_flow and timestep; per step a dict with
       accepted  bool[nx]   the free forcing-row cells the oracle's accelerate_flow changed
       refused   bool[nx]   the free ones it left alone
       sole      {3: n, 6: n, 7: n}   cells where that clause was the only one to refuse
       margin    min over free cells and clauses of |f - aw| / aw
       finite    whether the state after the step is finite
       peak      max |f| of the state after the step
    then {n: state after n steps, in the oracle's precision} for the step counts in `keep`, and the av_vels record"""
    ny, nx = obstacles.shape
    real = oracle.real
    p = oracle.make_params(nx, ny, nsteps, 10, density, accel, omega)
    oracle.set_obstacles(p, obstacles)
    aw1, aw2 = thresholds(density, accel, real)
    aw = {3: aw1, 6: aw2, 7: aw2}
    row = ny - 2
    free = obstacles[row] == 0
    cells = np.array(cells0, dtype=real, copy=True)
    tmp = np.empty_like(cells)
    steps, states, av = [], {}, []
    with np.errstate(all="ignore"):
        for _ in range(nsteps):
            before = cells[:, row, :].copy()
            oracle.accelerate_flow(p, cells, obstacles)
            changed = cells[1, row, :] != before[1]
            ok = {k: (before[k] - aw[k]) > 0 for k in CLAUSES}
            accepted = free & ok[3] & ok[6] & ok[7]
            assert np.array_equal(changed, accepted), "the oracle's guard and its restatement here disagree"
            sole = {k: int(np.count_nonzero(free & ~ok[k] & np.logical_and.reduce([ok[j] for j in CLAUSES if j != k])))
                    for k in CLAUSES}
            margin = min(float(np.min(np.abs(before[k][free] - aw[k]) / aw[k])) for k in CLAUSES)
            av.append(oracle.timestep(p, cells, tmp, obstacles))
            cells, tmp = tmp, cells
            steps.append({"accepted": accepted, "refused": free & ~accepted, "sole": sole, "margin": margin,
                          "finite": bool(np.all(np.isfinite(cells))), "peak": float(np.max(np.abs(cells)))})
            if len(steps) in keep:
                states[len(steps)] = cells.copy()
    return steps, states, np.array(av, dtype=real)


def oracle_form(out_dir, precision, pairwise, contract):
    """oracle/d2q9_oracle.c built in another honest form (momenta pairwise or left to right, FMA contraction on or off), as
    oracle_fma of test_dp_gpu.py does: the difference between two forms of one precision is the reference's own error"""
    import ctypes
    import os
    import subprocess
    from oracle.oracle import HERE, Oracle
    out = os.path.join(str(out_dir), "liboracle_%s_p%d_%s.so" % (precision, pairwise, contract))
    subprocess.run(["gcc", "-std=c99", "-O3", "-march=native", "-fPIC", "-DREAL=%s" % {"f32": "float", "f64": "double"}[precision],
                    "-DORACLE_PAIRWISE=%d" % pairwise, "-ffp-contract=%s" % contract, "-fopenmp", "-shared",
                    os.path.join(HERE, "d2q9_oracle.c"), "-o", out, "-lm"], check=True)
    o = Oracle(precision, omp=True)
    base = o.lib
    o.lib = ctypes.CDLL(out)
    for name in ("oracle_accelerate_flow", "oracle_timestep", "oracle_run"):
        f, g = getattr(o.lib, name), getattr(base, name)
        f.argtypes, f.restype = g.argtypes, g.restype
    assert o.lib.oracle_pairwise_momentum() == pairwise and o.lib.oracle_real_size() == np.dtype(o.real).itemsize
    return o


# ---- the cases of tests/test_forcing_guard_gpu.py: name -> (nx, ny, steps the longest test on it runs, guard_case keywords) ----
# Seeds are the first ones on which every condition of conditions() holds (tests/test_forcing_guard_cpu.py asserts them).
CASES = {
    "260x33": (260, 33, 23, dict(seed=33)),
    "132x40": (132, 40, 11, dict(seed=1)),
    "1024x8": (1024, 8, 11, dict(seed=4)),
    "256x37": (256, 37, 23, dict(seed=3)),
    "1024x50": (1024, 50, 23, dict(seed=46)),
    # no blocked cell in rows ny-4 .. ny-1: with obst_paths = 1 the deep kernels' waves on the forcing row run collide2<false>
    "256x37 open top": (256, 37, 23, dict(seed=61, open_top=True)),
    "33x17": (33, 17, 21, dict(seed=1)),
    "130x31": (130, 31, 21, dict(seed=1)),
    "128x128": (128, 128, 21, dict(seed=2)),
    "128x6": (128, 6, 23, dict(seed=1)),
    "132x64": (132, 64, 23, dict(seed=1)),
    "260x512": (260, 512, 23, dict(seed=32)),
    "1024x1024": (1024, 1024, 23, dict(seed=10)),
    # no blocked cell at all (collide2<false> everywhere): nothing but the dips refuses, so they are wider here to last 23 steps
    "2048x260 free": (2048, 260, 23, dict(seed=104, blocked=0.0, hy=24, hx=64)),
    "2048x260 walls": (2048, 260, 8, dict(seed=2, blocked=1e-4, walls=True)),
    "260x50": (260, 50, 23, dict(seed=32)),
    "256x64": (256, 64, 23, dict(seed=15)),
    # ensemble members, each with constants of its own
    "48x40 a": (48, 40, 13, dict(seed=1)),
    "48x40 b": (48, 40, 13, dict(seed=1, density=0.21, accel=0.25, omega=1.3)),
    "48x40 c": (48, 40, 13, dict(seed=5, density=0.5, accel=0.15, omega=1.2)),
    "48x40 d": (48, 40, 13, dict(seed=11, density=0.1, accel=0.2, omega=1.0)),
    # double precision
    "70x50": (70, 50, 19, dict(seed=1)),
    "200x72": (200, 72, 19, dict(seed=3)),
}
# run_until of the gated ensemble test: check points at steps 8 and 12; on the fp32 oracle the members' av_vels change by 0.146,
# 0.135, 0.139 and 0.106 over the four steps up to step 8 (tests/test_forcing_guard_cpu.py asserts the distance from the tolerance)
GATE_MAX_STEPS, GATE_WINDOW, GATE_TOL = 12, 4, 0.12
MEMBERS = ("48x40 a", "48x40 b", "48x40 c", "48x40 d")
DOUBLE_CASES = ("70x50", "200x72")


def case(name, real=np.float32):
    nx, ny, nsteps, kw = CASES[name]
    return guard_case(nx, ny, nsteps=nsteps, real=real, **kw)


def plane_norm(got, ref):
    """max |got - ref| of each plane over the plane's mean |ref|, the largest over the planes (one plane for av_vels)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.ndim == 1:
        got, ref = got[None], ref[None]
    n = ref.shape[0]
    return float(np.max(np.max(np.abs(got - ref).reshape(n, -1), axis=1) / np.mean(np.abs(ref).reshape(n, -1), axis=1)))


# the fp32 oracle's two forms may differ from the fp64 oracle by this much of a plane's mean at the end of a case: ten times
# what they differ by after one step (2e-6).  Beyond it the state amplifies rounding and a gate built on the spread is no gate.
SPREAD_MAX = 2.5e-5


def side_windows(nx):
    """the columns left and right of the periodic wrap at x = 0 that the wrap conditions look at"""
    w = min(64, nx // 4)
    x = np.arange(nx)
    return x >= nx - w, x < w


def conditions(nx, audits, density, nsteps):
    """the conditions of the issue on one case; audits = {oracle name: per-step list of guard_audit}, the first entry the
    fp32 oracle of the Makefile; returns the list of conditions that do NOT hold"""
    names = list(audits)
    first = audits[names[0]]
    bad = []
    left, right = side_windows(nx)
    last_wave = np.arange(nx) >= (nx // 256) * 256
    reached = {k: [] for k in CLAUSES}
    mixed_pair, mixed_left, mixed_right, mixed_last = [], [], [], []
    for t in range(nsteps):
        st = first[t]
        acc, ref = st["accepted"], st["refused"]
        # (beyond the issue's "finite": a state that has grown past ten times the case's density is on its way out)
        if not st["finite"] or not st["peak"] <= 10.0 * density:
            bad.append("step %d: state not finite or above 10 x density" % t)
        if ref.sum() < 8 or acc.sum() < 8:
            bad.append("step %d: %d refused, %d accepted" % (t, ref.sum(), acc.sum()))
        for n in names:
            if audits[n][t]["margin"] < 1e-4:
                bad.append("step %d: margin %.2e in %s" % (t, audits[n][t]["margin"], n))
            if not np.array_equal(audits[n][t]["accepted"], acc):
                bad.append("step %d: %s decides otherwise" % (t, n))
        for k in CLAUSES:
            if st["sole"][k]:
                reached[k].append(t)
        pairs = nx // 2
        a2, r2 = acc[:2 * pairs].reshape(pairs, 2), ref[:2 * pairs].reshape(pairs, 2)
        if np.any((a2[:, 0] & r2[:, 1]) | (a2[:, 1] & r2[:, 0])):
            mixed_pair.append(t)
        for where, rec in ((left, mixed_left), (right, mixed_right), (last_wave, mixed_last)):
            if np.any(acc & where) and np.any(ref & where):
                rec.append(t)
    for k in CLAUSES:
        if 0 not in reached[k]:
            bad.append("f%d never refuses alone at step 0" % k)
        if nsteps > 1 and not any(0 < t < 8 for t in reached[k]):
            bad.append("f%d never refuses alone at steps 1..7" % k)
    for what, rec in (("a lane pair", mixed_pair), ("the columns left of the wrap", mixed_left),
                      ("the columns right of the wrap", mixed_right)):
        if 0 not in rec or (nsteps > 1 and not any(0 < t < 8 for t in rec)):
            bad.append("refused and accepted cells do not both occur in %s at step 0 and at one of steps 1..7" % what)
    if nx % 256 and not mixed_last:   # (260 columns: four cells in the middle of the dip across the wrap, mixed at step 0 only)
        bad.append("refused and accepted cells never both occur in the partly filled last wave")
    return bad

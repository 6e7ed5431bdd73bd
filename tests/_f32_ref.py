"""Truth, unit and statistics for holding an fp32 timestep to fp64, in units of rounding.

No GPU and no restatement of the product here: the truth is the fp64 oracle (oracle/d2q9_oracle.c) run on the fp32 state
widened to double with the fp32 run constants widened to double, so what is left between a kernel and the truth is the rounding
of the kernel's arithmetic and of its fp32 constants.  tests/test_f32_accuracy_cpu.py proves the gates on the CPU,
tests/test_f32_accuracy_gpu.py applies them to the HIP kernels.

Unit.  For a value x of speed k on a fluid cell, e = (x - truth) / (2^-24 w_k rho), rho = the truth's density of the cell
(a collision conserves it, so it is the density of the gathered cell and of the cell after the step alike).  w_k rho is the size
of the value at rest and 2^-24 the relative half-spacing of fp32, so e = 1 is about one correct rounding of the value.

Statistics of e over the fluid values of a case (stats): max |e| and rms; the mean per speed class (rest / axis / diagonal) with
its standard error rms / sqrt(n) -- the three fp32 weights all round up, each by 0.125 units, and a step takes omega of that into
every value: most of the positive mean a correct kernel shows; per cell the mass error sum_k w_k e_k and the momentum errors sum_k c_k w_k e_k (units of
2^-24 rho), mean and standard error.

Sensitivities (sensitivities): the least-squares fit e = a P1 + b P2 + c over the fluid values with
  P1 = (truth_out - g) / (w_k rho)                         d out / d ln omega in units of the value at rest
  P2 = omega (4.5 j_k^2 - 1.5 j^2) / rho^2                 d out / d ln(1/rho) of the quadratic terms, same units
so a is the relative error of the relaxation rate the kernel applied and b that of its 1.5/rho coefficient (reciprocal, the 1.5
and the 3.0 on top of it), both in units of 2^-24, with standard errors from the residual.

Gates (check_gates), each of a kernel against the fp32 oracle measured on the same case, both against the truth:
  rms <= 1.25 x the oracle's, max <= 2 x the oracle's; class, mass and momentum means within 5 pooled standard errors;
  |a - a_oracle| <= 5 sigma; |b - b_oracle| <= 2 + 5 sigma (a reciprocal good to 1 ulp is up to 2 units of systematic error).
"""
import numpy as np

U = 2.0 ** -24
W = np.array([4.0 / 9.0] + [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])
OPP = [0, 3, 4, 1, 2, 7, 8, 5, 6]
CLASSES = {"rest": [0], "axis": [1, 2, 3, 4], "diag": [5, 6, 7, 8]}

SHAPES = [(33, 19), (64, 48), (256, 8)]
OMEGAS = [0.6, 1.0, 1.7, 1.99]
DENSITIES = [0.1, 1.0, 100.0]
STATES = ["near_rest", "driven"]
BLOCKED = 0.08

RMS_RATIO, MAX_RATIO, NSIGMA, B_SLACK = 1.25, 2.0, 5.0, 2.0


# ---- states ---------------------------------------------------------------------------------------------------------

def near_rest(rng, nx, ny, density=0.1):
    """test_gpu_parity.random_case at any density: 8 % blocked cells, the rest state times 1 +- 10 % per value"""
    ob = (rng.random((ny, nx)) < BLOCKED).astype(np.int32)
    w = W.reshape(9, 1, 1) * density
    cells = (w * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5))).astype(np.float32)
    return ob, cells


def driven(rng, nx, ny, density=0.1):
    """far from rest and far from equilibrium: the equilibrium of a random rho (+- 10 %) and u uniform in +- 0.25 per component
    (Mach up to 0.6), times 1 +- 20 % per value; every value stays positive (the smallest equilibrium factor is 0.34375, on an axis speed against u)"""
    ob = (rng.random((ny, nx)) < BLOCKED).astype(np.int32)
    rho = density * (1.0 + 0.1 * (2.0 * rng.random((ny, nx)) - 1.0))
    ux = 0.25 * (2.0 * rng.random((ny, nx)) - 1.0)
    uy = 0.25 * (2.0 * rng.random((ny, nx)) - 1.0)
    usq = ux * ux + uy * uy
    cells = np.empty((9, ny, nx))
    for k in range(9):
        cu = CX[k] * ux + CY[k] * uy
        cells[k] = W[k] * rho * (1.0 + 3.0 * cu + 4.5 * cu * cu - 1.5 * usq)
    cells *= 1.0 + 0.2 * (2.0 * rng.random((9, ny, nx)) - 1.0)
    return ob, cells.astype(np.float32)


def build_state(kind, nx, ny, density):
    """the state of a case, seeded per shape (the same geometry and the same random draws at every density and omega)"""
    rng = np.random.default_rng(1000 * nx + ny + (0 if kind == "near_rest" else 500000))
    return {"near_rest": near_rest, "driven": driven}[kind](rng, nx, ny, density)


def max_mach(cells, ob):
    c = cells.astype(np.float64)
    rho = c.sum(0)
    jx, jy = np.tensordot(CX, c, 1), np.tensordot(CY, c, 1)
    return float(np.max((np.sqrt(jx * jx + jy * jy) / rho * np.sqrt(3.0))[ob == 0]))


# ---- truth ----------------------------------------------------------------------------------------------------------

def gather(cells):
    """the pull-stream gather with periodic wrap (kernels.cl:91-112): g_k(x, y) = f_k(x - cx_k, y - cy_k)"""
    return np.stack([np.roll(cells[k], (int(CY[k]), int(CX[k])), axis=(0, 1)) for k in range(9)])


def params_f64(oracle_f64, p32, ob, nsteps=1):
    """the fp32 run constants widened to double; free_cells_inv = 1 / free cells in double"""
    po = oracle_f64.make_params(p32.nx, p32.ny, max(nsteps, 1), p32.reynolds_dim, float(np.float32(p32.density)),
                                float(np.float32(p32.accel)), float(np.float32(p32.omega)))
    return oracle_f64.set_obstacles(po, ob)


def truth(oracle_f64, p32, ob, cells32, nsteps):
    """the fp64 oracle on cells32.astype(float64), step by step.  Returns a dict: `cells` the state after nsteps, `av` the
    av_vels record (1 / free cells in double), `u` per step the |u_i| of the fluid cells (what av_bound takes), `rho` the
    density of every cell of the last gathered state, and for one step also `g`, `jx`, `jy`: the gathered pre-collision state
    (accelerate_flow applied) and its momenta."""
    po = params_f64(oracle_f64, p32, ob, nsteps)
    cur = np.ascontiguousarray(cells32, dtype=np.float64).copy()
    nxt = np.empty_like(cur)
    fluid = ob == 0
    out = {"av": np.zeros(nsteps), "u": []}
    for t in range(nsteps):
        oracle_f64.accelerate_flow(po, cur, ob)
        g = gather(cur)
        rho = g.sum(0)
        jx, jy = np.tensordot(CX, g, 1), np.tensordot(CY, g, 1)
        out["u"].append(np.sqrt(jx * jx + jy * jy)[fluid] / rho[fluid])
        out["av"][t] = oracle_f64.timestep(po, cur, nxt, ob)
        cur, nxt = nxt, cur
    out.update(cells=cur, rho=rho, omega=float(po.omega), inv64=float(po.free_cells_inv))
    if nsteps == 1:
        out.update(g=g, jx=jx, jy=jy)
    return out


def blocked_equal(x, tr, ob):
    """bounce-back is a permutation: after one step a blocked cell holds the truth cast to fp32, exactly"""
    blk = ob != 0
    return np.array_equal(np.asarray(x)[:, blk], tr["cells"][:, blk].astype(np.float32))


# ---- unit and statistics ------------------------------------------------------------------------------------------------

def units(x, truth_cells, rho, ob):
    """e[9, fluid cells] = (x - truth) / (2^-24 w_k rho)"""
    fluid = ob == 0
    d = np.asarray(x, dtype=np.float64)[:, fluid] - truth_cells[:, fluid]
    return d / (U * W[:, None] * rho[fluid][None, :])


def _mean_se(v):
    v = np.ravel(v)
    return float(v.mean()), float(np.sqrt(np.mean(v * v)) / np.sqrt(v.size))


def stats(e):
    """dict: max, rms; rest / axis / diag: (mean, standard error) of the class; mass, momx, momy: (mean, standard error) of the
    per-cell sums in units of 2^-24 rho"""
    s = {"max": float(np.max(np.abs(e))), "rms": float(np.sqrt(np.mean(e * e)))}
    for name, ks in CLASSES.items():
        s[name] = _mean_se(e[ks])
    s["mass"] = _mean_se((W[:, None] * e).sum(0))
    s["momx"] = _mean_se(((W * CX)[:, None] * e).sum(0))
    s["momy"] = _mean_se(((W * CY)[:, None] * e).sum(0))
    return s


def sensitivities(e, tr, ob):
    """(a, sigma_a, b, sigma_b) of the fit e = a P1 + b P2 + c (module docstring), units of 2^-24 relative error"""
    fluid = ob == 0
    rho, jx, jy = tr["rho"][fluid], tr["jx"][fluid], tr["jy"][fluid]
    p1 = (tr["cells"][:, fluid] - tr["g"][:, fluid]) / (W[:, None] * rho[None, :])
    jk = CX[:, None] * jx[None, :] + CY[:, None] * jy[None, :]
    p2 = tr["omega"] * (4.5 * jk * jk - 1.5 * (jx * jx + jy * jy)[None, :]) / (rho * rho)[None, :]
    X = np.stack([p1.ravel(), p2.ravel(), np.ones(p1.size)], axis=1)
    y = e.ravel()
    coef, *_ = np.linalg.lstsq(X, y, rcond=None)
    res = y - X @ coef
    cov = np.linalg.inv(X.T @ X) * (res @ res) / (y.size - 3)
    return float(coef[0]), float(np.sqrt(cov[0, 0])), float(coef[1]), float(np.sqrt(cov[1, 1]))


def measure(x, tr, ob, fit=True):
    """stats of x against a truth(), plus a, sa, b, sb for a one-step truth"""
    e = units(x, tr["cells"], tr["rho"], ob)
    m = stats(e)
    if fit and "g" in tr:
        m["a"], m["sa"], m["b"], m["sb"] = sensitivities(e, tr, ob)
    return m


def check_gates(got, orc):
    """{gate: (value, limit, passed)} of a kernel's measure() against the fp32 oracle's on the same case"""
    g = {"rms": (got["rms"], RMS_RATIO * orc["rms"]), "max": (got["max"], MAX_RATIO * orc["max"])}
    for name in ("rest", "axis", "diag", "mass", "momx", "momy"):
        g[name] = (abs(got[name][0] - orc[name][0]), NSIGMA * float(np.hypot(got[name][1], orc[name][1])))
    if "a" in got:
        g["a"] = (abs(got["a"] - orc["a"]), NSIGMA * float(np.hypot(got["sa"], orc["sa"])))
        g["b"] = (abs(got["b"] - orc["b"]), B_SLACK + NSIGMA * float(np.hypot(got["sb"], orc["sb"])))
    return {k: (v, lim, bool(v <= lim)) for k, (v, lim) in g.items()}


def failed(gates):
    return sorted(k for k, (_, _, ok) in gates.items() if not ok)


def line(what, m):
    """one line of figures"""
    s = "%-44s max %6.2f rms %5.2f  rest %+5.2f axis %+5.2f diag %+5.2f  mass %+5.2f momx %+5.2f momy %+5.2f" % (
        what, m["max"], m["rms"], m["rest"][0], m["axis"][0], m["diag"][0], m["mass"][0], m["momx"][0], m["momy"][0])
    if "a" in m:
        s += "  a %+6.2f+-%.2f b %+6.2f+-%.2f" % (m["a"], m["sa"], m["b"], m["sb"])
    return s


# ---- av_vels ----------------------------------------------------------------------------------------------------------

C1, C2 = 33.0, 4.0


def av_bound(u_truth, inv):
    """Bound on |av_vels - truth's| of one step from the same state: inv * sum_i 2^-24 (C1 |u_i| + C2) over the fluid cells,
    u_truth = the truth's |u_i|, inv = 1 / free cells.  First-order worst case, every rounding at its limit and none
    cancelling, 1 = a relative error of 2^-24 (one correct rounding; a hardware result good to 1 ulp is 2).

    Per cell, collide_cell returns sqrt(usq) * densinv:
      density      8 additions of positive terms, each partial sum <= rho                          8
      reciprocal   1 ulp                                                                          2
      usq          fma(jx, jx, fl(jy jy)): 1 on jy^2 and 1 on the sum, halved by the root          1
      square root  1 ulp                                                                          2
      product      sqrt * densinv                                                                 1
      momenta      the last of the three roundings of jx and of jy is relative to the component: the pair moves |j| by 1   1
                   the others are relative to the differences they round, not to j: on exact inputs
                   |d jx| <= 2^-24 (|g1 - g3| + |da| + |db| + |da + db|) <= 2^-24 (g1 + g3 + 2 (g5 + g6 + g7 + g8)),
                   likewise jy with g2 + g4, and |d |j|| <= |d jx| + |d jy| <= 2^-24 (axis + 4 diagonals) <= 2^-24 4 rho   C2 = 4
    which is 15 |u_i| + 4.  (A count of typical rather than largest sizes -- one unit each for root, reciprocal, usq and
    product, the momenta at a third of rho -- gives about 4 |u_i| + 2; it leaves out the density sum and the second unit of a
    1-ulp result, and a sum of errors that is meant to hold without any cancelling has to carry those.)
    Per record entry, on top: free_cells_inv is an fp32 value (1) and the entry is rounded to fp32 (1); the partial sums are
    fp32 until a workgroup's total is widened to double, and a term passes through at most 16 fp32 additions on the way (3
    over a lane's four cells, the wave butterfly's 6, the workgroup's waves, a few trips of a grid-stride or row loop): 16.
    C1 = 15 + 2 + 16 = 33.  Against av_vels of about 0.1 this is 2e-6 relative where RTOL_AV is 1e-4."""
    u_truth = np.asarray(u_truth, dtype=np.float64)
    return float(inv) * U * float(C1 * np.sum(np.abs(u_truth)) + C2 * u_truth.size)

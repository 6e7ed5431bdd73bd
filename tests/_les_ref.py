"""The Smagorinsky subgrid viscosity of include/lbm.h ("Subgrid viscosity") restated in numpy float64, on top of
tests/_wall_ref.py, tests/_open_ref.py and tests/_trt_ref.py: the reference the GPU tests compare against.

A step with the model on is the step of _wall_ref with a relaxation rate per cell.  The rate comes from the gathered values
after the boundary fix (_trt_ref.gather, _open_ref.fix) by the header's statements, one ufunc per written operator; np.sqrt is
the correctly rounded square root.  The arrays om (and, with TRT, omega_m from tp = tau - 0.5 by the three statements of "Two
relaxation times") then go through _wall_ref.step in the place of its scalars: numpy broadcasts them, so gather, fix,
equilibrium, relaxation lines, bounce-back and moving walls are the imported ones, untouched.  With c None (or 0.0) a step is
_wall_ref.step itself and returns its arrays."""
import numpy as np

import _open_ref
import _trt_ref
import _wall_ref
from _force_ref import body_restatement

THIRD = np.float64(1.0) / np.float64(3.0)
HALF, ONE, TWO = np.float64(0.5), np.float64(1.0), np.float64(2.0)


def constants(omega, c):
    """(tau0, les_k): the header's two host statements"""
    omega, c = np.float64(omega), np.float64(c)
    tau0 = ONE / omega
    les_k = (np.float64(18.0) * np.sqrt(np.float64(2.0))) * (c * c)
    return float(tau0), float(les_k)


def moments(g):
    """(dens, densinv, u_x, u_y) of the gathered values: _trt_ref.step's statements (u_x, u_y are momenta)"""
    dens = g[0].copy()
    for k in range(1, 9):
        dens = dens + g[k]
    densinv = ONE / dens
    diag_a, diag_b = g[5] - g[7], g[8] - g[6]
    u_x = (g[1] - g[3]) + (diag_a + diag_b)
    u_y = (g[2] - g[4]) + (diag_a - diag_b)
    return dens, densinv, u_x, u_y


def stress(g):
    """(pxx, pyy, pxy, q, densinv) of the gathered values g, a list of nine float64 arrays: the header's device statements up
    to q"""
    dens, densinv, u_x, u_y = moments(g)
    d57 = g[5] + g[7]
    d68 = g[6] + g[8]
    dgs = d57 + d68
    p = dens * THIRD
    pxx = ((g[1] + g[3]) + dgs) - (p + (u_x * u_x) * densinv)
    pyy = ((g[2] + g[4]) + dgs) - (p + (u_y * u_y) * densinv)
    pxy = (d57 - d68) - (u_x * u_y) * densinv
    q = np.sqrt((pxx * pxx + pyy * pyy) + TWO * (pxy * pxy))
    return pxx, pyy, pxy, q, densinv


def rates(g, omega, c, magic=None):
    """(tau, om, omega_m or None) per cell of the gathered (and fixed) values g"""
    tau0, les_k = (np.float64(v) for v in constants(omega, c))
    with np.errstate(all="ignore"):                   # blocked cells go through the arithmetic and are replaced by the caller
        _, _, _, q, densinv = stress(g)
        tau = HALF * (tau0 + np.sqrt(tau0 * tau0 + les_k * (q * densinv)))
        om = ONE / tau
        omega_m = None
        if magic:
            tp = tau - HALF
            tm = np.float64(magic) / tp + HALF
            omega_m = ONE / tm
    return tau, om, omega_m


def gathered(f, ob, u_in=None, rho_out=None):
    """what a cell collides: the gather, and the boundary fix where open boundaries are on"""
    g = _trt_ref.gather(f)
    return g if u_in is None else _open_ref.fix(g, ob, u_in, rho_out)


def step(f, ob, omega, magic=None, u_in=None, rho_out=None, wall=None, c=None):
    """_wall_ref.step with the model: (cells, |u| with 0 on blocked cells).  magic: None or 0 = BGK, else TRT with that magic
    parameter.  c: None or 0.0 = off, the arrays of _wall_ref.step."""
    if not c:
        om_m = _trt_ref.omega_minus(omega, magic) if magic else None
        return _wall_ref.step(f, ob, omega, om_m, u_in, rho_out, wall)
    assert f.dtype == np.float64 and f.shape[0] == 9
    _, om, omega_m = rates(gathered(f, ob, u_in, rho_out), omega, c, magic)
    with np.errstate(all="ignore"):                   # the rates of blocked cells may be NaN; bounce-back replaces their cells
        return _wall_ref.step(f, ob, om, omega_m, u_in, rho_out, wall)


def effective_omega(f, ob, omega, c, u_in=None, rho_out=None):
    """om of every cell in the step that streams f (blocked cells: whatever the arithmetic gives)"""
    return rates(gathered(f, ob, u_in, rho_out), omega, c)[1]


# ---- the two flows of the tests -------------------------------------------------------------------------------------------

COUETTE_C = 2.0     # |S| = U / H is tiny in the Couette case: a constant this large makes the eddy viscosity 12.9 % of the total
GATE = 1e-4         # the Couette case's wall force and profile against the formula, on the CPU and on the GPU

CAVITY = dict(nx=32, ny=32, U=0.1, rho=0.1, omega=1.99, c=0.17, steps=3000, bgk_limit=2000)


def couette_force(nx, ny, U, rho, omega, c):
    """rho (nu + c^2 U / H) U nx / H: a steady shear has |S| = U / H, so nu_t = c^2 U / H everywhere; nu = (1 / omega - 1 / 2) / 3"""
    h = float(ny - 2)
    return rho * ((1.0 / omega - 0.5) / 3.0 + c * c * U / h) * U * nx / h


def couette_figures(before, f):
    """(relative error of F_x on the top wall, on the bottom wall, the same against the molecular viscosity alone, profile error
    over U) from the state the last step streamed and the settled state"""
    c = _wall_ref.COUETTE
    ob, _, _ = _wall_ref.couette_maps()
    want = couette_force(c["nx"], c["ny"], c["U"], c["rho"], c["omega"], COUETTE_C)
    plain = _wall_ref.couette_force(c["nx"], c["ny"], c["U"], c["rho"], c["omega"])
    rel = []
    for row, sign in ((c["ny"] - 1, -1.0), (0, +1.0)):
        body = np.zeros_like(ob)
        body[row] = 1
        fx, _, links, _ = body_restatement(before, ob, body)
        assert links == 3 * c["nx"]
        rel.append((abs(fx - sign * want) / want, abs(fx - sign * plain) / plain))
    err = float(np.max(np.abs(_wall_ref.column_velocity(f, c["nx"] // 2) - _wall_ref.couette_profile(c["ny"], c["U"])))) / c["U"]
    return rel[0][0], rel[1][0], min(rel[0][1], rel[1][1]), err


def cavity_maps(nx=CAVITY["nx"], ny=CAVITY["ny"], U=CAVITY["U"]):
    """(obstacles, u_x, u_y): the four edge rows and columns blocked, row ny - 1 moving with (U, 0) on columns 1 .. nx - 2"""
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    ob[:, 0] = ob[:, nx - 1] = 1
    u_x = np.zeros((ny, nx), dtype=np.float64)
    u_x[ny - 1, 1:nx - 1] = U
    return ob, u_x, np.zeros((ny, nx), dtype=np.float64)


def velocity_magnitude(f, ob):
    """(max |u| over the fluid cells, min density over them) of a stored state"""
    fluid = ob == 0
    with np.errstate(all="ignore"):
        rho = np.sum(f, axis=0)
        jx = f[1] + f[5] + f[8] - f[3] - f[6] - f[7]
        jy = f[2] + f[5] + f[6] - f[4] - f[7] - f[8]
        u = np.sqrt(jx * jx + jy * jy) / rho
    return float(np.max(u[fluid])), float(np.min(rho[fluid]))

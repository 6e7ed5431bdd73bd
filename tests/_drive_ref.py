"""The body force of include/lbm.h ("Body force") restated in numpy float64, on top of tests/_les_ref.py, tests/_wall_ref.py,
tests/_open_ref.py and tests/_trt_ref.py: the reference the GPU tests compare bits against.

With drive None (or (0, 0)) a step is _les_ref.step itself and returns its arrays.  With the force on, the gather and the
boundary fix (_les_ref.gathered), the host constants (_trt_ref.omega_minus, _les_ref.constants), the subgrid rates
(_les_ref.rates, which is handed the shifted momenta through its own `moments`), the bounce-back by mask and the moving walls
(_wall_ref.apply) are the imported ones.  What the force changes cannot be imported: the momenta gain half the force before the
equilibrium reads them, so the equilibrium and the relaxation lines are written out here once more, on the shifted momenta and
with the header's source behind them, one ufunc per written operator in the header's order (numpy never contracts two ufunc
calls into an FMA).  tests/test_drive_restatement_cpu.py holds these lines, with F = 0 in place, to _les_ref.step bit for bit."""
import contextlib
import json
import os

import numpy as np

import _les_ref
import _open_ref
import _trt_ref
import _wall_ref
from _force_ref import restatement
from _trt_ref import OPP, PAIRS

ZERO, HALF, ONE, THREE, NINE = (np.float64(v) for v in (0.0, 0.5, 1.0, 3.0, 9.0))
W0, W1, W2 = np.float64(4.0) / np.float64(9.0), np.float64(1.0) / np.float64(9.0), np.float64(1.0) / np.float64(36.0)
S1, S2 = np.float64(1.0) / np.float64(3.0), np.float64(1.0) / np.float64(12.0)
W = [W0] + [W1] * 4 + [W2] * 4
S = [None] + [S1] * 4 + [S2] * 4


def is_on(drive):
    return drive is not None and not (float(drive[0]) == 0.0 and float(drive[1]) == 0.0)


_plain_moments = _les_ref.moments


def moments(g, drive):
    """(dens, densinv, u_x, u_y): _les_ref.moments with half the force added to the two momenta"""
    dens, densinv, u_x, u_y = _plain_moments(g)
    return dens, densinv, u_x + HALF * np.float64(drive[0]), u_y + HALF * np.float64(drive[1])


@contextlib.contextmanager
def _shifted_moments(drive):
    """_les_ref's statements read the shifted momenta: its `moments` is this module's for the duration"""
    _les_ref.moments = lambda g: moments(g, drive)
    try:
        yield
    finally:
        _les_ref.moments = _plain_moments


def vectors(a, b):
    """c_k . (a, b) in the pattern of uvec: index 0 is not used"""
    return [None, a, b, -a, -b, a + b, -a + b, -a - b, a - b]


def collide(g, omega, omega_m, drive):
    """The fluid statements on the gathered (and fixed) values g: (out list of nine, |u|).  omega, omega_m: scalars, or the
    per-cell arrays of the subgrid model; omega_m None: BGK."""
    f_x, f_y = np.float64(drive[0]), np.float64(drive[1])
    ic_sq = THREE
    dens, densinv, u_x, u_y = moments(g, drive)
    u_sq = u_x * u_x + u_y * u_y
    uvec = vectors(u_x, u_y)
    half_densinv_icsq = HALF * densinv * ic_sq
    eq = [W0 * (dens - half_densinv_icsq * u_sq)]
    for k in range(1, 9):
        t = uvec[k] * ic_sq
        tsq = t * uvec[k]
        eq.append(W[k] * (dens + t + half_densinv_icsq * (tsq - u_sq)))
    # the source
    v_x, v_y = u_x * densinv, u_y * densinv
    uF = v_x * f_x + v_y * f_y
    t3 = THREE * uF
    cF = vectors(f_x, f_y)
    se, so = [W0 * (ZERO - t3)], [None]
    for k in range(1, 9):
        cv = uvec[k] * densinv
        se.append(W[k] * (NINE * (cv * cF[k]) - t3))
        so.append(S[k] * cF[k])
    pe = ONE - HALF * omega
    out = [None] * 9
    out[0] = (g[0] + omega * (eq[0] - g[0])) + pe * se[0]
    if omega_m is None:
        for k in range(1, 9):
            out[k] = (g[k] + omega * (eq[k] - g[k])) + pe * (se[k] + so[k])
    else:
        po = ONE - HALF * omega_m
        for k, q in PAIRS:
            a, b = eq[k] - g[k], eq[q] - g[q]
            sp, sm = HALF * (a + b), HALF * (a - b)
            rp, rm = omega * sp, omega_m * sm
            fe, fo = pe * se[k], po * so[k]
            out[k] = (g[k] + (rp + rm)) + (fe + fo)
            out[q] = (g[q] + (rp - rm)) + (fe - fo)
    return out, np.sqrt(u_sq) * densinv


def step(f, ob, omega, magic=None, u_in=None, rho_out=None, wall=None, c=None, drive=None):
    """_les_ref.step with the body force drive = (F_x, F_y): (cells, |u| with 0 on blocked cells).  drive None or (0, 0): the
    arrays of _les_ref.step."""
    if not is_on(drive):
        return _les_ref.step(f, ob, omega, magic, u_in, rho_out, wall, c)
    assert f.dtype == np.float64 and f.shape[0] == 9
    g = _les_ref.gathered(f, ob, u_in, rho_out)
    blocked = ob != 0
    with np.errstate(all="ignore"):                   # blocked cells go through the arithmetic and are replaced below
        if c:
            with _shifted_moments(drive):
                _, om, om_m = _les_ref.rates(g, omega, c, magic)
        else:
            om = np.float64(omega)
            om_m = np.float64(_trt_ref.omega_minus(omega, magic)) if magic else None
        out, u = collide(g, om, om_m, drive)
    cells = np.stack([np.where(blocked, g[OPP[k]], out[k]) for k in range(9)])
    return _wall_ref.apply(cells, ob, wall), np.where(blocked, 0.0, u)


def fields(f, ob, density, drive=None):
    """The output stage (dp_output_cell) on the stored state f: (u_x, u_y, u, pressure); blocked cells give 0, 0, 0,
    density / 3.  With the force on the two momentum sums of the stored state lose half of it before the division: the physical
    velocity."""
    blocked = ob != 0
    with np.errstate(all="ignore"):
        rho = np.zeros_like(f[0])
        for k in range(9):
            rho = rho + f[k]
        jx = f[1] + f[5] + f[8] - f[3] - f[6] - f[7]
        jy = f[2] + f[5] + f[6] - f[4] - f[7] - f[8]
        if is_on(drive):
            jx = jx - HALF * np.float64(drive[0])
            jy = jy - HALF * np.float64(drive[1])
        ux, uy = jx / rho, jy / rho
        uu = np.sqrt(ux * ux + uy * uy)
        pr = rho * (np.float64(1.0) / np.float64(3.0))
    rest = np.float64(density) * (np.float64(1.0) / np.float64(3.0))
    return (np.where(blocked, 0.0, ux), np.where(blocked, 0.0, uy), np.where(blocked, 0.0, uu), np.where(blocked, rest, pr))


# ---- the three flows with exact answers, and the sweep ---------------------------------------------------------------------

DENSITY = 0.1
L316, L14 = 3.0 / 16.0, 0.25

POISEUILLE = dict(nx=8, ny=11, force=(1e-6, 0.0), steps=20000, omegas=(0.6, 1.0, 1.7, 1.9))
HYDROSTATIC = dict(nx=9, ny=12, force=(0.0, -1e-4), steps=30000, cases=((1.0, L316), (1.7, None)))
BALANCE = dict(nx=24, ny=15, force=(2e-6, 0.0), steps=30000, cases=((1.0, L316), (1.4, None)), fluid=296)
SWEEP = dict(forces=tuple(i * 1e-7 for i in range(1, 9)), omega=1.0, magic=L316, window=64, rel_tol=1e-7, max_steps=30000)
START = 200    # steps after which the GPU tests compare cells with the restatement's


def channel_mask(nx, ny):
    """walls on rows 0 and ny - 1, periodic in x"""
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    return ob


def box_mask(nx, ny):
    """all four borders blocked"""
    ob = channel_mask(nx, ny)
    ob[:, 0] = ob[:, nx - 1] = 1
    return ob


def balance_mask():
    """the channel of BALANCE with a 4 x 4 block at rows 5-8, columns 8-11"""
    ob = channel_mask(BALANCE["nx"], BALANCE["ny"])
    ob[5:9, 8:12] = 1
    return ob


def run(ob, omega, magic, drive, steps, f=None):
    """`steps` restated steps from rest (or from f) with accel = 0: the state"""
    ny, nx = ob.shape
    f = _open_ref.rest_state(DENSITY, ny, nx).copy() if f is None else f
    for _ in range(steps):
        f = step(f, ob, omega, magic, drive=drive)[0]
    return f


def parabola(ny, omega, f_x, rho):
    """u(y) of the force-driven flow between walls half-way: F_x (y - 1/2)(H - (y - 1/2)) / (2 rho nu) on rows 1 .. ny - 2"""
    h = float(ny - 2)
    nu = (1.0 / omega - 0.5) / 3.0
    y = np.arange(1, ny - 1, dtype=np.float64) - 0.5
    return f_x * y * (h - y) / (2.0 * rho * nu)


def poiseuille_figures(ux, uy, pressure, omega, f_x=POISEUILLE["force"][0]):
    """(deviation, density spread, max |u_y|) from the output stage's fields of the channel: max |u - parabola| / max parabola over
    the fluid cells, (max - min) / mean of the density there, max |u_y| there"""
    ny = ux.shape[0]
    rho = 3.0 * pressure[1:ny - 1]
    p = parabola(ny, omega, f_x, float(rho.mean()))
    dev = float(np.max(np.abs(ux[1:ny - 1] - p[:, None])) / np.max(p))
    return dev, float((rho.max() - rho.min()) / rho.mean()), float(np.max(np.abs(uy[1:ny - 1])))


def hydrostatic_figures(uu, pressure, f_y=HYDROSTATIC["force"][1]):
    """(max |u| over the fluid cells, max relative error of the row-to-row density steps against 3 F_y)"""
    ny, nx = uu.shape
    rho = 3.0 * pressure[1:ny - 1, 1:nx - 1]
    steps = rho[1:] - rho[:-1]
    return float(np.max(uu[1:ny - 1, 1:nx - 1])), float(np.max(np.abs(steps / (3.0 * f_y) - 1.0)))


def balance_figures(fx, fy, f_x=BALANCE["force"][0], fluid=BALANCE["fluid"]):
    """(|sum F_x / (F_x N_fluid) - 1|, |sum F_y| / (F_x N_fluid)) of the momentum-exchange force over all blocked cells"""
    total = f_x * fluid
    return abs(fx / total - 1.0), abs(fy) / abs(total)


def state_figures(kind, f, ob, omega, drive):
    """the figures of a flow from a stored state, through fields() and, for the balance, the force of the next step"""
    ux, uy, uu, pr = fields(f, ob, DENSITY, drive)
    if kind == "poiseuille":
        return poiseuille_figures(ux, uy, pr, omega, drive[0])
    if kind == "hydrostatic":
        return hydrostatic_figures(uu, pr, drive[1])
    fx, fy = restatement(f, ob)[:2]
    return balance_figures(fx, fy, drive[0])


# ---- tests/golden/drive.json and the gates on its figures and on the library's -----------------------------------------------
# The gates are conditions the known answers set, not figures of the code under test; tests/test_drive_restatement_cpu.py says
# why, and applies them to the fixture's figures, tests/test_drive_gpu.py to the library's.

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GATED_OMEGAS = (0.6, 1.0, 1.7)
CAP = 1e-9


def fixture():
    with open(os.path.join(GOLDEN, "drive.json")) as f:
        return json.load(f)


def poiseuille_table(fix):
    """{(magic or None, omega): (deviation, spread, max |u_y|)} of the fixture"""
    return {(e["magic"], e["omega"]): (e["deviation"], e["spread"], e["uy"]) for e in fix["poiseuille"]["entries"]}


def case_table(fix, flow, keys):
    return {(e["magic"], e["omega"]): tuple(e[k] for k in keys) for e in fix[flow]["entries"]}


def poiseuille_gates(fig, stored):
    """fig, stored: {(magic or None, omega): (deviation, spread, max |u_y|)}, the figures under test and the fixture's; fig may
    hold any subset of the fixture's runs, and each gate is applied to the runs it has"""
    lines = []
    for key, (dev, spread, uy) in sorted(fig.items(), key=str):
        magic, w = key
        name = "BGK" if magic is None else "Lambda %.4f" % magic
        lines.append("%s omega %.1f: deviation %.3e (fixture %.3e), density spread %.2e (gate %.2e), |u_y| %.2e (gate %.2e)" % (
            name, w, dev, stored[key][0], spread, 100.0 * stored[key][1], uy, 100.0 * stored[key][2]))
        assert 0.0 <= spread <= 100.0 * stored[key][1], lines[-1]
        assert 0.0 <= uy <= 100.0 * stored[key][2], lines[-1]
        if magic == L316 and w in GATED_OMEGAS:                                  # omega 1.9 has not settled: printed, not gated
            bound = min(100.0 * stored[key][0], CAP)
            assert dev <= bound, (lines[-1], bound)
    if (L14, 1.0) in fig and (L14, 1.7) in fig:
        a, b = fig[(L14, 1.0)][0], fig[(L14, 1.7)][0]
        lines.append("Lambda 1/4: deviation %.9e at omega 1.0, %.9e at 1.7 (gates: equal to 1e-6 relative, >= 1e-3)" % (a, b))
        assert abs(a - b) <= 1e-6 * abs(b) and min(a, b) >= 1e-3, lines[-1]
    if (None, 0.6) in fig:
        other = fig[(L316, 0.6)][0] if (L316, 0.6) in fig else stored[(L316, 0.6)][0]
        lines.append("BGK omega 0.6: deviation %.3e against %.3e at Lambda 3/16 (gate >= 10 x)" % (fig[(None, 0.6)][0], other))
        assert fig[(None, 0.6)][0] >= 10.0 * other, lines[-1]
    return lines


def hydrostatic_gates(umax, step_error, stored_umax):
    bound = min(100.0 * stored_umax, 1e-12)
    line = "hydrostatic: max |u| %.2e (gate %.2e), density steps against 3 F_y %.2e (gate 1e-9)" % (umax, bound, step_error)
    assert 0.0 <= umax <= bound and step_error <= 1e-9, line
    return line


def balance_gates(rel, lift, stored_rel):
    """rel = |sum F_x / (F_x N_fluid) - 1|, lift = |sum F_y| / (F_x N_fluid)"""
    bound = min(100.0 * stored_rel, CAP)
    line = "balance: |sum F_x / (F_x N) - 1| %.2e, |sum F_y| / (F_x N) %.2e (gate %.2e on both)" % (rel, lift, bound)
    assert rel <= bound and lift <= bound, line
    return line


def mirror_gate(fx, fx_mirrored, stored_rel):
    """the member with the mirrored force: the opposite sum F_x, within the margin of the balance gate"""
    total = BALANCE["force"][0] * BALANCE["fluid"]
    bound = min(100.0 * stored_rel, CAP)
    line = "mirrored force: |sum F_x + sum F_x'| / (F_x N) %.2e (gate %.2e)" % (abs(fx + fx_mirrored) / total, bound)
    assert fx > 0.0 > fx_mirrored and abs(fx + fx_mirrored) <= bound * total, line
    return line


def sweep_gate(av, forces, stored_spread):
    """Stokes regime: the settled av_vels over F_x is one constant across the members, within 10 x the spread the restatement shows"""
    ratio = np.asarray(av, dtype=np.float64) / np.asarray(forces, dtype=np.float64)
    spread = float((ratio.max() - ratio.min()) / ratio.mean())
    line = "sweep: av_vels / F_x %.6e .. %.6e, spread %.2e (gate %.2e)" % (ratio.min(), ratio.max(), spread, 10.0 * stored_spread)
    assert np.all(ratio > 0.0) and spread <= 10.0 * stored_spread, line
    return line

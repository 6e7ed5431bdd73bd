"""The scalar's record of include/lbm.h ("Scalar record") restated in numpy float64, on top of tests/_scalar_ref.py and
tests/_buoy_ref.py, which are imported and not edited: the reference the GPU tests compare bits against, the sweeps the steady
runs stop on, and the cavity's convective Nusselt number.

cells() is the header's three statements on the GATHERED values of a scalar step.  _scalar_ref.step does not hand out what it
gathers, so gathered() restates that half of it, statement for statement, and collided() the other half: check_gather() holds the
pair to _scalar_ref.step bit for bit, the gate of this restatement.  entry() adds in the device's order: _buoy_ref.segment_sums
(the lane's pair sum, the tree of a 16-cell segment) and _buoy_ref.reduce (dp_reduce with one block).

`defect` names a seeded mistake (tests/test_scalar_record_restatement_cpu.py holds each one to the fixture): "written" takes c
from the state the step writes and not from the gathered values, "no_half" takes the velocity without the half-force, "blocked"
counts the blocked cells' stored values, "flat" adds the cells in one flat sum."""
import json
import os
from types import SimpleNamespace

import numpy as np

import _buoy_ref as bref
import _drive_ref
import _scalar_ref as sref
import _steady_rule
from _scalar_ref import CX, CY, OPP, SIXTH, THIRD, THREE

DEFECTS = ("written", "no_half", "blocked", "flat")
NAMES = ("content", "flux_x", "flux_y")
CRITERIA = {"content": "scalar", "flux_x": "scalar_flux_x", "flux_y": "scalar_flux_y"}


def gathered(g, ob, c_wall=None, c_in=None):
    """h[0..4] of every cell behind the wall, inlet and outlet statements: the first half of _scalar_ref.step"""
    ny, nx = ob.shape
    blocked = ob != 0
    wall = np.full((ny, nx), np.nan) if c_wall is None else np.asarray(c_wall, dtype=np.float64)
    with np.errstate(all="ignore"):
        h = [g[0]]
        for k in range(1, 5):
            shift = (CY[k], CX[k])
            q_blocked = np.roll(blocked, shift, axis=(0, 1))
            q_wall = np.roll(wall, shift, axis=(0, 1))
            back = g[OPP[k]]
            held = THIRD * q_wall - back
            h.append(np.where(q_blocked, np.where(np.isnan(q_wall), back, held), np.roll(g[k], shift, axis=(0, 1))))
        if c_in is not None:
            h[1] = h[1].copy()
            h[3] = h[3].copy()
            h[1][:, 0] = np.asarray(c_in, dtype=np.float64) - (((h[0][:, 0] + h[2][:, 0]) + h[3][:, 0]) + h[4][:, 0])
            h[3][:, nx - 1] = g[3][:, nx - 1]
    return h


def collided(g, h, ob, u_x, u_y, om_s):
    """the second half of _scalar_ref.step on gathered values h"""
    blocked = ob != 0
    om_s = np.float64(om_s)
    with np.errstate(all="ignore"):
        c = (((h[0] + h[1]) + h[2]) + h[3]) + h[4]
        a_x = THREE * (c * u_x)
        a_y = THREE * (c * u_y)
        e = [THIRD * c, SIXTH * (c + a_x), SIXTH * (c + a_y), SIXTH * (c - a_x), SIXTH * (c - a_y)]
        out = [h[k] + om_s * (e[k] - h[k]) for k in range(5)]
    return np.stack([np.where(blocked, g[k], out[k]) for k in range(5)])


def check_gather(g, ob, u_x, u_y, om_s, c_wall=None, c_in=None):
    """gathered() and collided() are _scalar_ref.step, bit for bit: returns that step's result"""
    g1 = sref.step(g, ob, u_x, u_y, om_s, c_wall, c_in)
    assert np.array_equal(collided(g, gathered(g, ob, c_wall, c_in), ob, u_x, u_y, om_s), g1, equal_nan=True)
    return g1


def cells(g, ob, u_x, u_y, c_wall=None, c_in=None, defect=None, written=None):
    """(c, c u_x, c u_y) of every cell, +0.0 on the blocked ones.  written: the state the step writes, for the defect of that name"""
    blocked = ob != 0
    h = gathered(g, ob, c_wall, c_in)
    with np.errstate(all="ignore"):
        c = (((h[0] + h[1]) + h[2]) + h[3]) + h[4]
        if defect == "written":
            c = (((written[0] + written[1]) + written[2]) + written[3]) + written[4]
        q_x = c * u_x
        q_y = c * u_y
    if defect == "blocked":
        stored = (((g[0] + g[1]) + g[2]) + g[3]) + g[4]
        return np.where(blocked, stored, c), np.where(blocked, 0.0, q_x), np.where(blocked, 0.0, q_y)
    return tuple(np.where(blocked, 0.0, v) for v in (c, q_x, q_y))


def entry(values, defect=None):
    """the record's three entries of one step from cells(), added in the device's order"""
    if defect == "flat":
        return tuple(np.float64(np.sum(v)) for v in values)
    return tuple(bref.reduce(bref.segment_sums(v)) for v in values)


def passive_entry(fa, g, ob, om_s, drive=None, c_wall=None, c_in=None, defect=None):
    """scalar step n of a passive scalar on the state fa that flow step n streams: (g after it, the step's three entries)"""
    u_x, u_y = sref.velocity(fa, ob, drive)
    g1 = check_gather(g, ob, u_x, u_y, om_s, c_wall, c_in)
    return g1, entry(cells(g, ob, u_x, u_y, c_wall, c_in, defect, g1), defect)


def passive_advance(f, g, fl, om_s, c_wall=None, c_in=None, defect=None):
    """_scalar_ref.advance with the record: (f, g, the step's three entries, |u| per cell of the flow step)"""
    fa = sref.streamed(f, fl)
    g1, rec = passive_entry(fa, g, fl.ob, om_s, fl.drive, c_wall, c_in if fl.opened is not None else None, defect)
    u_in, rho_out = fl.opened if fl.opened is not None else (None, None)
    f1, u = _drive_ref.step(fa, fl.ob, fl.omega, fl.magic, u_in, rho_out, drive=fl.drive)
    return f1, g1, rec, u


def buoyant_advance(f, g, s, defect=None):
    """_buoy_ref.advance with the record: (f, g, the step's three entries, |u| per cell of the flow step, the streamed state).
    The velocity is the output stage's on the streamed state, less half of the force of the scalar state the step reads."""
    f1, g1, u, fa = bref.advance(f, g, s)
    F = bref.force(g, s.b, s.c_ref, s.drive)
    u_x, u_y = bref.fields(fa, s.ob, 1.0, F, "no_half" if defect == "no_half" else None)[:2]
    c_in = s.c_in if s.opened is not None else None
    if defect != "no_half":
        assert np.array_equal(check_gather(g, s.ob, u_x, u_y, s.om_s, s.c_wall, c_in), g1, equal_nan=True)
    return f1, g1, entry(cells(g, s.ob, u_x, u_y, s.c_wall, c_in, defect, g1), defect), u, fa


# ---- the sweeps the steady runs stop on ---------------------------------------------------------------------------------------

BOX = dict(n=12, H=10, omega=1.5, Pr=0.71, c_ref=0.5, Ras=(1e3, 3e3, 1e4), window=16, rel_tol=1e-4, cap=512, which="flux_x")
CHANNEL = dict(nx=37, ny=29, omega=1.0, accel=0.005, Ds=(0.4, 0.25, 0.1), window=32, rel_tol=1e-2, cap=1600, which="content")
START = 48           # steps of the first member of each sweep that the CPU module recomputes


def box(Ra):
    """the closed box of BOX: _buoy_ref.cavity at another size and Rayleigh number"""
    B = BOX
    n, H = B["n"], B["H"]
    ob = _drive_ref.box_mask(n, n)
    nu = bref.viscosity(B["omega"])
    kappa = nu / B["Pr"]
    wall = np.full((n, n), np.nan)
    wall[1:n - 1, 0], wall[1:n - 1, n - 1] = 1.0, 0.0
    x = (np.arange(n, dtype=np.float64) - 0.5)[None, :]
    c0 = np.broadcast_to(1.0 - x / H, (n, n)).copy()
    s = bref.setting(ob, bref.RHO0, 0.0, B["omega"], (0.0, bref.layer_buoyancy(Ra, nu, kappa, H)), B["c_ref"], kappa, c_wall=wall)
    return SimpleNamespace(s=s, c0=c0, f0=sref.rest(ob, bref.RHO0))


def channel(D):
    """_steady_rule.channel(37, 29) under accelerate_flow, the wall of row 0 held at 1, every other blocked cell insulating, the
    scalar from zero: the content rises until the fluid is at the wall's value"""
    C = CHANNEL
    ob = _steady_rule.channel(C["nx"], C["ny"])
    wall = np.full(ob.shape, np.nan)
    wall[0] = 1.0
    fl = sref.flow(ob, bref.RHO0, C["accel"], C["omega"])
    return SimpleNamespace(fl=fl, ob=ob, D=D, wall=wall, c0=np.zeros(ob.shape), f0=sref.rest(ob, bref.RHO0))


def box_records(Ra, steps, defect=None):
    """float64[3, steps] of a box member from rest"""
    cs = box(Ra)
    f, g, rec = cs.f0, sref.init(cs.c0), []
    for _ in range(steps):
        f, g, r = buoyant_advance(f, g, cs.s, defect)[:3]
        rec.append(r)
    return np.array(rec).T


def channel_records(D, steps, defect=None):
    """float64[3, steps] of a channel member from rest"""
    cs = channel(D)
    f, g, rec, om = cs.f0, sref.init(cs.c0), [], sref.omega_s(D)
    for _ in range(steps):
        f, g, r = passive_advance(f, g, cs.fl, om, cs.wall, None, defect)[:3]
        rec.append(r)
    return np.array(rec).T


def stops(records, sweep):
    """_steady_rule.rule on the chosen value's records of a plain run to the cap: (steps, converged)"""
    chosen = np.ascontiguousarray(np.stack([r[NAMES.index(sweep["which"])] for r in records]))
    return _steady_rule.rule(chosen, 0, sweep["cap"], sweep["window"], sweep["rel_tol"])


def check_stops(entry_of_fixture, sweep, members_at_cap):
    """the issue's conditions on the chosen inputs, on the fixture's entry"""
    steps, conv = entry_of_fixture["stops"], entry_of_fixture["converged"]
    assert len({s for s, c in zip(steps, conv) if c}) >= 2, steps                    # two different counts among those that converge
    assert sum(1 for s, c in zip(steps, conv) if not c and s == sweep["cap"]) >= members_at_cap, (steps, conv)
    assert min(steps) > sweep["window"], steps                                       # no stop at the first check point


# ---- the known flow ------------------------------------------------------------------------------------------------------------

def nusselt_convective(flux_x, ob, H, kappa, dC=1.0):
    """1 + <c u_x> H / (kappa dC): the volume-averaged Nusselt number of a side-heated cavity from the last entry of flux_x"""
    return 1.0 + float(flux_x) / float(np.count_nonzero(ob == 0)) * H / (kappa * dC)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scalar_steady.json")


def fixture():
    with open(GOLDEN) as fh:
        return json.load(fh)

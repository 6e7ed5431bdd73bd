"""Buoyancy of include/lbm.h ("Buoyancy") restated in numpy float64, on top of tests/_scalar_ref.py, tests/_drive_ref.py and
tests/_les_ref.py: the reference the GPU tests compare bits against, the flows with known answers and their figures.

force() is the header's four statements on a cell's five stored scalar values.  A flow step under a force that differs from cell to
cell is _drive_ref.collide and _drive_ref.moments, which take arrays for `drive`, behind _les_ref.gathered; _drive_ref.is_on and
_drive_ref.step do not take arrays, so the step wrapper (flow_step) and the output stage (fields) are restated here, statement for
statement.  The scalar step is _scalar_ref.step as it is.  advance() is the library's stream: scalar step n on state n's force, then
flow step n on the force of the scalar state that step has just written.

record() restates the order in which the device adds: per-lane pair sums, the tree over the eight lanes of a 16-cell segment,
then dp_reduce's lane-strided accumulation, wave butterfly and four waves in order (one block: grids of up to 4096 segments), so
av_vels and the force record are compared by np.array_equal too.

`defect` names a seeded mistake (tests/test_buoy_restatement_cpu.py holds each one to the gates): "sign" flips b, "no_half" leaves
the output stage's half-force out, "old_array" lets the flow read the scalar's old array, "no_f0" drops F0 while buoyancy is on."""
import json
import os
from types import SimpleNamespace

import numpy as np

import _drive_ref
import _les_ref
import _scalar_ref as sref
import _trt_ref
import _wall_ref
from _drive_ref import HALF
from _trt_ref import CX, CY, OPP

DEFECTS = ("sign", "no_half", "old_array", "no_f0")


def force(g, b, c_ref, f0=None, defect=None):
    """(F_x, F_y) per cell from the stored scalar populations g[5, ny, nx]: the header's statements"""
    f0 = (0.0, 0.0) if (f0 is None or defect == "no_f0") else f0
    b_x, b_y = (np.float64(-v if defect == "sign" else v) for v in b)
    c = (((g[0] + g[1]) + g[2]) + g[3]) + g[4]
    d = c - np.float64(c_ref)
    return np.float64(f0[0]) + b_x * d, np.float64(f0[1]) + b_y * d


def flow_step(f, ob, omega, F, magic=None, u_in=None, rho_out=None, wall=None, c=None):
    """_drive_ref.step with the per-cell force F = (F_x[ny, nx], F_y[ny, nx]): (cells, |u| with 0 on blocked cells)"""
    assert f.dtype == np.float64 and f.shape[0] == 9
    g = _les_ref.gathered(f, ob, u_in, rho_out)
    blocked = ob != 0
    with np.errstate(all="ignore"):                   # blocked cells go through the arithmetic and are replaced below
        if c:
            with _drive_ref._shifted_moments(F):
                _, om, om_m = _les_ref.rates(g, omega, c, magic)
        else:
            om = np.float64(omega)
            om_m = np.float64(_trt_ref.omega_minus(omega, magic)) if magic else None
        out, u = _drive_ref.collide(g, om, om_m, F)
    cells = np.stack([np.where(blocked, g[OPP[k]], out[k]) for k in range(9)])
    return _wall_ref.apply(cells, ob, wall), np.where(blocked, 0.0, u)


def fields(f, ob, density, F, defect=None):
    """_drive_ref.fields with the per-cell force: the two momentum sums lose half of each cell's own force"""
    blocked = ob != 0
    with np.errstate(all="ignore"):
        rho = np.zeros_like(f[0])
        for k in range(9):
            rho = rho + f[k]
        jx = f[1] + f[5] + f[8] - f[3] - f[6] - f[7]
        jy = f[2] + f[5] + f[6] - f[4] - f[7] - f[8]
        if defect != "no_half":
            jx = jx - HALF * F[0]
            jy = jy - HALF * F[1]
        ux, uy = jx / rho, jy / rho
        uu = np.sqrt(ux * ux + uy * uy)
        pr = rho * (np.float64(1.0) / np.float64(3.0))
    rest = np.float64(density) * (np.float64(1.0) / np.float64(3.0))
    return (np.where(blocked, 0.0, ux), np.where(blocked, 0.0, uy), np.where(blocked, 0.0, uu), np.where(blocked, rest, pr))


def setting(ob, density, accel, omega, b, c_ref, D, magic=None, opened=None, wall=None, les=None, drive=None, c_wall=None, c_in=None):
    """everything advance() needs of one grid: opened = None or (u_in[ny], rho_out), wall = None or (u_x, u_y, rho_wall), les = None
    or the Smagorinsky constant, drive = None or F0"""
    return SimpleNamespace(ob=ob, density=density, accel=accel, omega=omega, b=b, c_ref=c_ref, D=D, om_s=sref.omega_s(D), magic=magic,
                           opened=opened, wall=wall, les=les, drive=drive, c_wall=c_wall, c_in=c_in)


def advance(f, g, s, defect=None):
    """scalar step n, then flow step n: (f, g, |u| per cell of the flow step, the state the flow step streamed)"""
    fa = f if s.opened is not None else sref.accelerate(f, s.ob, s.density, s.accel)
    u_x, u_y = fields(fa, s.ob, 1.0, force(g, s.b, s.c_ref, s.drive, defect), defect)[:2]
    g1 = sref.step(g, s.ob, u_x, u_y, s.om_s, s.c_wall, s.c_in if s.opened is not None else None)
    u_in, rho_out = s.opened if s.opened is not None else (None, None)
    F = force(g if defect == "old_array" else g1, s.b, s.c_ref, s.drive, defect)
    f1, u = flow_step(fa, s.ob, s.omega, F, s.magic, u_in, rho_out, s.wall, s.les)
    return f1, g1, u, fa


def final_state(f, g, s, defect=None):
    """the output stage on the two current states"""
    return fields(f, s.ob, s.density, force(g, s.b, s.c_ref, s.drive, defect), defect)


# ---- the order in which the device adds ---------------------------------------------------------------------------------------

def segment_sums(v):
    """v[ny, nx], one value per cell (0.0 where a cell counts nothing): the sums of the 16-cell row segments, flat [ny * nseg], in
    the tree of dp_segment_tree8 over the lanes' pair sums; a lane without a second cell adds 0.0, a lane past the row's end is 0.0"""
    ny, nx = v.shape
    nseg = -(-(-(-nx // 2)) // 8)
    a = np.zeros((ny, nseg * 8))
    b = np.zeros((ny, nseg * 8))
    a[:, :(nx + 1) // 2] = v[:, 0::2]
    b[:, :nx // 2] = v[:, 1::2]
    p = (a + b).reshape(ny, nseg, 8)
    q = p[:, :, 0::2] + p[:, :, 1::2]
    r = q[:, :, 0::2] + q[:, :, 1::2]
    return (r[:, :, 0] + r[:, :, 1]).reshape(-1)


def reduce(seg):
    """dp_reduce with one block of 256 lanes on the flat segment sums: lane-strided accumulation, the wave butterfly, the four
    waves in order"""
    assert seg.size <= 4096
    acc = np.zeros(256)
    for i0 in range(0, seg.size, 256):
        chunk = seg[i0:i0 + 256]
        acc[:chunk.size] = acc[:chunk.size] + chunk
    w = acc.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ o]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def cell_forces(fa, ob, counted):
    """dp_force_cell on every counted blocked cell of the streamed state fa: (F_x[ny, nx], F_y[ny, nx]), one addition per link
    term for k = 1..8 in ascending order, +0.0 elsewhere"""
    blocked = ob != 0
    fx, fy = np.zeros(ob.shape), np.zeros(ob.shape)
    for k in range(1, 9):
        shift = (CY[k], CX[k])
        use = counted & np.roll(~blocked, shift, axis=(0, 1))
        s = np.roll(fa[k], shift, axis=(0, 1)) + fa[OPP[k]]
        if CX[k]:
            fx = np.where(use, fx + s if CX[k] > 0 else fx - s, fx)
        if CY[k]:
            fy = np.where(use, fy + s if CY[k] > 0 else fy - s, fy)
    return fx, fy


def counted_cells(ob, body, opened):
    """the blocked cells whose links the record counts: those of the body (None: all), outside columns 0 and nx - 1 with open
    boundaries on"""
    counted = (ob != 0) if body is None else ((ob != 0) & (np.asarray(body) != 0))
    if opened:
        counted = counted.copy()
        counted[:, 0] = counted[:, -1] = False
    return counted


def record(u, fa, ob, free_cells_inv, counted=None):
    """(av_vels entry, F_x, F_y) of one step as the device adds them; counted None: no force record"""
    av = reduce(segment_sums(u)) * np.float64(free_cells_inv)
    if counted is None:
        return av, None, None
    fx, fy = cell_forces(fa, ob, counted)
    return av, reduce(segment_sums(fx)), reduce(segment_sums(fy))


# ---- the flows with known answers ------------------------------------------------------------------------------------------
# Each has a setup shared by tests/golden/make_buoy.py, the CPU module and the GPU module, and a function that turns fields into
# the figures the gates are about.

RHO0 = 0.1
START = 200                      # steps of every flow that the CPU module recomputes
LAYER = dict(nx=32, ny=18, H=16, omega=1.6, steps=20000, Ra=1500.0)
ONSET = dict(Ras=(1500.0, 1900.0), steps=8000, t0=7000, eps=1e-3, theory=1707.76)
CAVITY = dict(n=32, H=30, omega=1.5, Pr=0.71, Ra=1e3, steps=20000, theory=1.118)
DRIVEN = dict(Ra=1900.0, drive=(2e-6, 0.0))


def viscosity(omega):
    return (1.0 / omega - 0.5) / 3.0


def layer_buoyancy(Ra, nu, kappa, H, dC=1.0):
    """|b| = rho0 a of a layer with that Rayleigh number: Ra = (|b| dC / rho0) H^3 / (nu kappa)"""
    return Ra * nu * kappa * RHO0 / (dC * H ** 3)


def layer(Ra, eps=0.0, drive=None):
    """the layer of LAYER between a wall held at 1 (row 0) and one held at 0 (row ny - 1), periodic in x, D = nu, c_ref 0.5, the
    scalar on the straight conduction profile plus eps sin(pi y / H) cos(2 pi x / nx), the flow at rest"""
    L = LAYER
    nx, ny, H = L["nx"], L["ny"], L["H"]
    ob = _drive_ref.channel_mask(nx, ny)
    nu = viscosity(L["omega"])
    wall = np.full((ny, nx), np.nan)
    wall[0], wall[ny - 1] = 1.0, 0.0
    y = (np.arange(ny, dtype=np.float64) - 0.5)[:, None]
    x = np.arange(nx, dtype=np.float64)[None, :]
    c0 = (1.0 - y / H) + eps * np.sin(np.pi * y / H) * np.cos(2.0 * np.pi * x / nx)
    s = setting(ob, RHO0, 0.0, L["omega"], (0.0, layer_buoyancy(Ra, nu, nu, H)), 0.5, nu, drive=drive, c_wall=wall)
    return SimpleNamespace(s=s, c0=c0, f0=sref.rest(ob, RHO0))


def cavity():
    """the closed box of CAVITY: column 0 held at 1, column n - 1 at 0, rows 0 and n - 1 insulating, c_ref 0.5, the scalar on the
    straight conduction profile, the flow at rest"""
    C = CAVITY
    n, H = C["n"], C["H"]
    ob = _drive_ref.box_mask(n, n)
    nu = viscosity(C["omega"])
    kappa = nu / C["Pr"]
    wall = np.full((n, n), np.nan)
    wall[1:n - 1, 0], wall[1:n - 1, n - 1] = 1.0, 0.0
    x = (np.arange(n, dtype=np.float64) - 0.5)[None, :]
    c0 = np.broadcast_to(1.0 - x / H, (n, n)).copy()
    b = layer_buoyancy(C["Ra"], nu, kappa, H)
    assert np.sqrt(b / RHO0 * H) < 0.1                # the buoyant velocity scale stays small against the lattice's
    s = setting(ob, RHO0, 0.0, C["omega"], (0.0, b), 0.5, kappa, c_wall=wall)
    return SimpleNamespace(s=s, c0=c0, f0=sref.rest(ob, RHO0))


def max_uy(u_y, ob):
    return float(np.max(np.abs(u_y[ob == 0])))


def nusselt(c):
    """the mean Nusselt number on the hot wall of the cavity: -dC/dx at the wall half-way between columns 0 and 1, second order
    from the wall value and the first two fluid columns, times H / dC"""
    n, H = CAVITY["n"], CAVITY["H"]
    slope = (8.0 * 1.0 - 9.0 * c[1:n - 1, 1] + c[1:n - 1, 2]) / 3.0
    return float(np.mean(slope)) * H


def onset_figures(a0, a1):
    """a0, a1: max |u_y| of the two members at steps t0 and `steps`: (rate at Ra 1500, rate at Ra 1900, the Ra of zero growth by
    straight interpolation)"""
    dt = float(ONSET["steps"] - ONSET["t0"])
    r = [float(np.log(a1[k] / a0[k])) / dt for k in range(2)]
    lo, hi = ONSET["Ras"]
    return r[0], r[1], lo + (hi - lo) * (0.0 - r[0]) / (r[1] - r[0])


def run(cs, steps, samples=(), defect=None):
    """`steps` restated steps of a setup: (f, g, {step: (scalar field, final_state fields)} at the samples)"""
    f, g, seen = cs.f0, sref.init(cs.c0), {}
    for n in range(1, steps + 1):
        f, g = advance(f, g, cs.s, defect)[:2]
        if n in samples:
            seen[n] = (sref.field(g, cs.s.ob), final_state(f, g, cs.s, defect))
    return f, g, seen


def probes(f, g, s, defect=None):
    """six numbers that pin the two states down after a short stretch, none of them a sum that symmetry makes zero: the scalar
    field's sum, sum of squares and one cell beside the west edge of the middle row; the output stage's u_y there, its sum of
    squares and its largest magnitude"""
    c = sref.field(g, s.ob)
    u_y = final_state(f, g, s, defect)[1]
    at = (c.shape[0] // 2, 1)
    return [float(np.sum(c)), float(np.sum(c * c)), float(c[at]), float(u_y[at]), float(np.sum(u_y * u_y)), float(np.max(np.abs(u_y)))]


SHORT = {"rest": lambda: layer(LAYER["Ra"]), "onset_1500": lambda: layer(1500.0, ONSET["eps"]),
         "onset_1900": lambda: layer(1900.0, ONSET["eps"]), "cavity": cavity,
         "driven": lambda: layer(DRIVEN["Ra"], ONSET["eps"], DRIVEN["drive"])}

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "buoy.json")


def fixture():
    with open(GOLDEN) as fh:
        return json.load(fh)


def close(got, want, rel=1e-9):
    """the fixture's figure to 1e-9 relative: the same digits"""
    return abs(got - want) <= rel * abs(want)

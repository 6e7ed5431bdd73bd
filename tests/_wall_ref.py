"""Moving walls of include/lbm.h ("Moving walls") restated in numpy float64, on top of tests/_open_ref.py: the reference the
GPU tests compare bits against.

A step with walls moving is _open_ref.step (which is _trt_ref.step while open boundaries are off) followed by the header's
statements on the blocked cells that move.  After that step a blocked cell holds the plain bounce-back, cells[k] = g[OPP[k]],
so `out[1] = g[3] + a` is cells[1] + a there: one ufunc per written operator, np.where on the moving cells.  With no cell
moving (no setting, or every velocity +-0.0 on the blocked cells) the arrays of _open_ref.step are returned untouched.

The force needs no restatement of its own: _open_ref.force, _force_ref.restatement and _force_ref.body_restatement read the
stored state, which already carries what the wall added."""
import numpy as np

import _open_ref
import _trt_ref

C23 = np.float64(2.0) / np.float64(3.0)
C16 = np.float64(1.0) / np.float64(6.0)


def moving(ob, u_x, u_y):
    """the blocked cells whose two components do not both compare equal to 0.0"""
    return (np.asarray(ob) != 0) & ~((np.asarray(u_x) == 0.0) & (np.asarray(u_y) == 0.0))


def terms(u_x, u_y, rho_wall):
    """(a, b, p, q) of the header's statements"""
    rho = np.float64(rho_wall)
    u_x, u_y = np.asarray(u_x, dtype=np.float64), np.asarray(u_y, dtype=np.float64)
    rx = rho * u_x
    ry = rho * u_y
    a = C23 * rx
    b = C23 * ry
    p = C16 * (rx + ry)
    q = C16 * (ry - rx)
    return a, b, p, q


def apply(cells, ob, wall):
    """cells float64[9, ny, nx] after a step with every wall at rest -> with wall = (u_x, u_y, rho_wall); the same array
    where no cell moves"""
    if wall is None:
        return cells
    u_x, u_y, rho_wall = wall
    mv = moving(ob, u_x, u_y)
    if not mv.any():
        return cells
    a, b, p, q = terms(u_x, u_y, rho_wall)
    out = np.array(cells, dtype=np.float64, copy=True)
    out[1] = np.where(mv, cells[1] + a, cells[1])
    out[3] = np.where(mv, cells[3] - a, cells[3])
    out[2] = np.where(mv, cells[2] + b, cells[2])
    out[4] = np.where(mv, cells[4] - b, cells[4])
    out[5] = np.where(mv, cells[5] + p, cells[5])
    out[7] = np.where(mv, cells[7] - p, cells[7])
    out[6] = np.where(mv, cells[6] + q, cells[6])
    out[8] = np.where(mv, cells[8] - q, cells[8])
    return out


def step(f, ob, omega, omega_m=None, u_in=None, rho_out=None, wall=None):
    """_open_ref.step with wall = None or (u_x float64[ny, nx], u_y float64[ny, nx], rho_wall): (cells, |u| with 0 on blocked
    cells)"""
    cells, u = _open_ref.step(f, ob, omega, omega_m, u_in, rho_out)
    return apply(cells, ob, wall), u


# ---- the Couette case of the tests: 16 x 16, walls on rows 0 and ny - 1, the top wall moving ----------------------------------

COUETTE = dict(nx=16, ny=16, U=0.05, rho=0.1, omega=1.2, steps=6000, magic=3.0 / 16.0)


def couette_maps(nx=COUETTE["nx"], ny=COUETTE["ny"], U=COUETTE["U"]):
    """(obstacles, u_x, u_y): rows 0 and ny - 1 blocked, row ny - 1 moving with (U, 0)"""
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    u_x = np.zeros((ny, nx), dtype=np.float64)
    u_x[ny - 1] = U
    return ob, u_x, np.zeros((ny, nx), dtype=np.float64)


def couette_profile(ny, U):
    """U (y - 1/2) / (ny - 2) on the fluid rows 1 .. ny - 2: both wall planes lie half-way between a blocked row and its
    fluid neighbour"""
    y = np.arange(1, ny - 1, dtype=np.float64)
    return U * (y - 0.5) / float(ny - 2)


def column_velocity(f, x):
    """u_x on the fluid rows of column x of the state f of a walled channel"""
    ny = f.shape[1]
    c = f[:, 1:ny - 1, x]
    return (c[1] + c[5] + c[8] - c[3] - c[6] - c[7]) / np.sum(c, axis=0)


def couette_force(nx, ny, U, rho, omega):
    """rho nu U nx / H, the shear force on either wall of the settled flow; nu = (1 / omega - 1 / 2) / 3"""
    return rho * ((1.0 / omega - 0.5) / 3.0) * U * nx / float(ny - 2)


_couette = {}


def couette_run(trt):
    """the settled state of the Couette case and the state one step before it (what the last step streamed), once per
    operator"""
    if trt not in _couette:
        c = COUETTE
        ob, u_x, u_y = couette_maps()
        om = _trt_ref.omega_minus(c["omega"], c["magic"]) if trt else None
        f = _open_ref.rest_state(c["rho"], c["ny"], c["nx"])
        before = f
        for _ in range(c["steps"]):
            before = f
            f, u = step(f, ob, c["omega"], om, wall=(u_x, u_y, c["rho"]))
        _couette[trt] = (before, f, u)
    return _couette[trt]

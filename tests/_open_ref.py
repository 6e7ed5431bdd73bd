"""Open boundaries of include/lbm.h ("Open boundaries") restated in numpy float64, on top of tests/_trt_ref.py: the reference
the GPU tests compare bits against.

A step with open boundaries is gather, boundary fix, collision.  The gather and the collision are _trt_ref's, untouched: the
fixed gathered values go back through the inverse of its gather (a permutation of the cells, exact), so that _trt_ref.step
gathers exactly them and collides.  The fix is the header's two statement blocks, one ufunc per written operator, np.where
on the fluid test.  With the setting off (u_in None) a step is _trt_ref.step itself."""
import numpy as np

import _trt_ref
from _trt_ref import CX, CY, OPP, gather

TWO, HALF, ONE = np.float64(2.0), np.float64(0.5), np.float64(1.0)
C23 = np.float64(2.0) / np.float64(3.0)
C16 = np.float64(1.0) / np.float64(6.0)


def ungather(g):
    """the f whose gather is g: f_k(x) = g[k](x + c_k)"""
    return np.stack([np.roll(g[k], (-CY[k], -CX[k]), axis=(0, 1)) for k in range(9)])


def fix(g, ob, u_in, rho_out):
    """the boundary fix on the gathered values g (a list of nine float64[ny, nx]): new arrays, g is not modified"""
    g = [np.array(a, dtype=np.float64, copy=True) for a in g]
    ny, nx = ob.shape
    assert nx >= 3
    u = np.asarray(u_in, dtype=np.float64)
    assert u.shape == (ny,)
    rho_out = np.float64(rho_out)
    with np.errstate(all="ignore"):                   # blocked cells go through the arithmetic and keep their values
        # inlet, x == 0
        fluid = ob[:, 0] == 0
        c = [a[:, 0].copy() for a in g]
        s0 = (c[0] + c[2]) + c[4]
        s1 = (c[3] + c[6]) + c[7]
        rho = (s0 + TWO * s1) / (ONE - u)
        ru = rho * u
        d = HALF * (c[2] - c[4])
        g[1][:, 0] = np.where(fluid, c[3] + C23 * ru, c[1])
        g[5][:, 0] = np.where(fluid, (c[7] - d) + C16 * ru, c[5])
        g[8][:, 0] = np.where(fluid, (c[6] + d) + C16 * ru, c[8])
        # outlet, x == nx - 1
        fluid = ob[:, nx - 1] == 0
        c = [a[:, nx - 1].copy() for a in g]
        s0 = (c[0] + c[2]) + c[4]
        s1 = (c[1] + c[5]) + c[8]
        ru = (s0 + TWO * s1) - rho_out
        d = HALF * (c[2] - c[4])
        g[3][:, nx - 1] = np.where(fluid, c[1] - C23 * ru, c[3])
        g[7][:, nx - 1] = np.where(fluid, (c[5] + d) - C16 * ru, c[7])
        g[6][:, nx - 1] = np.where(fluid, (c[8] - d) - C16 * ru, c[6])
    return g


def step(f, ob, omega, omega_m=None, u_in=None, rho_out=None):
    """One timestep of the state f float64[9, ny, nx]: (cells, |u| with 0 on blocked cells).  u_in None: the periodic step of
    _trt_ref on f (the caller has accelerated it).  Else open boundaries: no accelerate_flow, f is the stored state."""
    if u_in is None:
        return _trt_ref.step(f, ob, omega, omega_m)
    assert f.dtype == np.float64 and f.shape[0] == 9
    return _trt_ref.step(ungather(fix(gather(f), ob, u_in, rho_out)), ob, omega, omega_m)


def counted_cells(ob, body=None):
    """the blocked cells whose links count while open boundaries are on: those of the body (None: every blocked cell) outside
    columns 0 and nx - 1"""
    counted = ob != 0
    if body is not None:
        counted = counted & (np.asarray(body) != 0)
    counted = counted.copy()
    counted[:, 0] = False
    counted[:, -1] = False
    return counted


def force(f, ob, body=None):
    """the momentum-exchange force of the step that streams the stored state f, with the column rule: (F_x, F_y, links, sum of
    |link terms|), as tests/test_force_gpu.restatement returns them"""
    assert f.dtype == np.float64
    blocked = ob != 0
    outer = counted_cells(ob, body)
    fx = fy = 0.0
    links, mag = 0, 0.0
    for k in range(1, 9):
        shift = (CY[k], CX[k])
        counted = outer & np.roll(~blocked, shift, axis=(0, 1))
        term = (np.roll(f[k], shift, axis=(0, 1)) + f[OPP[k]])[counted]
        fx += CX[k] * float(np.sum(term))
        fy += CY[k] * float(np.sum(term))
        links += int(term.size)
        mag += float(np.sum(np.abs(term)))
    return fx, fy, links, mag


def poiseuille(ny, u_max):
    """p(y) = 4 U (y - 1/2)(H - (y - 1/2)) / H^2 on rows 1 .. ny - 2, H = ny - 2; 0 on the wall rows 0 and ny - 1"""
    h = float(ny - 2)
    y = np.arange(ny, dtype=np.float64)
    p = 4.0 * u_max * (y - 0.5) * (h - (y - 0.5)) / (h * h)
    p[0] = p[ny - 1] = 0.0
    return p


def rest_state(density, ny, nx):
    """the library's rest state (d2q9-bgk.c:529-550 in double)"""
    w = np.zeros(9, dtype=np.float64)
    w[0] = np.float64(density) * 4.0 / 9.0
    w[1:5] = np.float64(density) / 9.0
    w[5:9] = np.float64(density) / 36.0
    return np.ascontiguousarray(np.broadcast_to(w.reshape(9, 1, 1), (9, ny, nx)))


def jx_of(f):
    return f[1] + f[5] + f[8] - f[3] - f[6] - f[7]


def channel_figures(f, u_max):
    """(spread of the column flux, mid-column shape error) of the channel check on the state f of a walled channel"""
    ny, nx = f.shape[1:]
    jx = jx_of(f)
    flux = np.sum(jx[1:ny - 1, :], axis=0)
    spread = float((flux.max() - flux.min()) / flux.mean())
    m = jx[1:ny - 1, nx // 2]
    p = poiseuille(ny, u_max)[1:ny - 1]
    shape = float(np.max(np.abs(m / m.sum() - p / p.sum())) * (ny - 2))
    return spread, shape

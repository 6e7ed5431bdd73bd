"""The two-relaxation-time collision of include/lbm.h ("Two relaxation times") restated in numpy float64: the reference the
GPU tests compare bits against.

Every line is one IEEE double operation per element, in the order of the header's statements (numpy never contracts two
ufunc calls into an FMA): the gather by np.roll, density and momenta, the equilibrium, the relaxation lines of either
operator, bounce-back by mask.  tests/test_trt_restatement_cpu.py holds the BGK mode of this file to the fp64 oracle's
pairwise no-FMA build bit for bit, which is what makes a bit comparison of the TRT mode mean something."""
import numpy as np

# speed k: c_k = (CX[k], CY[k]); OPP[k] the opposite speed (include/lbm.h)
CX = [0, 1, 0, -1, 0, 1, -1, -1, 1]
CY = [0, 0, 1, 0, -1, 1, 1, -1, -1]
OPP = [0, 3, 4, 1, 2, 7, 8, 5, 6]
PAIRS = [(1, 3), (2, 4), (5, 7), (6, 8)]


def omega_minus(omega, magic):
    """the header's three statements, in double"""
    omega, magic = np.float64(omega), np.float64(magic)
    tp = np.float64(1.0) / omega - np.float64(0.5)
    tm = magic / tp + np.float64(0.5)
    omega_m = np.float64(1.0) / tm
    return float(omega_m)


def gather(f):
    """g[k](x) = f_k(x - c_k), periodic in x and y (kernels.cl:91-112); np.roll(a, s)[i] = a[i - s]"""
    return [np.roll(f[k], (CY[k], CX[k]), axis=(0, 1)) for k in range(9)]


def step(f, ob, omega, omega_m=None):
    """One timestep of the accelerated state f float64[9, ny, nx] under the mask ob: (cells float64[9, ny, nx], |u| float64[ny,
    nx] with 0 on blocked cells).  omega_m None: BGK; else TRT with that second rate."""
    assert f.dtype == np.float64 and f.shape[0] == 9
    omega = np.float64(omega)
    g = gather(f)
    blocked = ob != 0
    ic_sq = np.float64(3.0)
    w0, w1, w2 = np.float64(4.0) / np.float64(9.0), np.float64(1.0) / np.float64(9.0), np.float64(1.0) / np.float64(36.0)
    with np.errstate(all="ignore"):                   # blocked cells go through the arithmetic and are replaced below
        dens = g[0].copy()
        for k in range(1, 9):
            dens = dens + g[k]
        densinv = np.float64(1.0) / dens
        diag_a, diag_b = g[5] - g[7], g[8] - g[6]
        u_x = (g[1] - g[3]) + (diag_a + diag_b)
        u_y = (g[2] - g[4]) + (diag_a - diag_b)
        u_sq = u_x * u_x + u_y * u_y
        uvec = [None, u_x, u_y, -u_x, -u_y, u_x + u_y, -u_x + u_y, -u_x - u_y, u_x - u_y]
        half_densinv_icsq = np.float64(0.5) * densinv * ic_sq
        eq = [w0 * (dens - half_densinv_icsq * u_sq)]
        for k in range(1, 9):
            t = uvec[k] * ic_sq
            tsq = t * uvec[k]
            eq.append((w1 if k < 5 else w2) * (dens + t + half_densinv_icsq * (tsq - u_sq)))
        out = [None] * 9
        if omega_m is None:
            for k in range(9):
                out[k] = g[k] + omega * (eq[k] - g[k])
        else:
            omega_m = np.float64(omega_m)
            out[0] = g[0] + omega * (eq[0] - g[0])
            for k, q in PAIRS:
                a, b = eq[k] - g[k], eq[q] - g[q]
                sp, sm = np.float64(0.5) * (a + b), np.float64(0.5) * (a - b)
                rp, rm = omega * sp, omega_m * sm
                out[k] = g[k] + (rp + rm)
                out[q] = g[q] + (rp - rm)
        u = np.sqrt(u_sq) * densinv
    # bounce-back: the un-relaxed value leaves through the opposite speed (kernels.cl:69, 187-197)
    cells = np.stack([np.where(blocked, g[OPP[k]], out[k]) for k in range(9)])
    return cells, np.where(blocked, 0.0, u)

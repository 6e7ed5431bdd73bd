"""Flows with a known answer, for tests/test_flows_gpu.py, tests/test_flows_restatement_cpu.py and tests/golden/make_flows.py:
geometry and figures only.  A step is _open_ref.step, a force is _open_ref.force; nothing of the method is restated here.

The channel: 32x11, walls on rows 0 and 10, poiseuille(11, 0.01) at the inlet, density = rho_out = 0.1, from rest.  Halfway
bounce-back puts the wall planes half a cell outside the first fluid rows, where poiseuille() has its zeros; where the computed
profile has its own depends on the collision.  `shape` of _open_ref.channel_figures measures the difference.

The cylinder: Schaefer and Turek's benchmark 2D-1 at Re = 20 (Benchmark computations of laminar flow around a cylinder, Notes
on Numerical Fluid Mechanics 52, 1996).  In cylinder diameters D: a channel 22 long and 4.1 between the wall planes, the
centre 2 behind the inlet and 2 above the lower wall plane, a parabolic inlet with U_mean = 2/3 U_max, Re = U_mean D / nu.
Published bounds: C_d 5.57 - 5.59, C_l 0.0104 - 0.0110, C = 2 F / (rho U_mean^2 D)."""
import numpy as np

import _open_ref
import _trt_ref

DENSITY = 0.1
MAGIC = 3.0 / 16.0

# the channel of the TRT wall-position check
CH_NX, CH_NY, CH_U, CH_STEPS = 32, 11, 0.01, 12000
CH_OMEGAS = (0.6, 1.0, 1.7, 1.9)

# Schaefer-Turek 2D-1
CD_PUBLISHED, CL_PUBLISHED = 5.58, 0.0107
U_MEAN, REYNOLDS = 0.04, 20.0


def channel_mask():
    ob = np.zeros((CH_NY, CH_NX), dtype=np.int32)
    ob[0] = ob[CH_NY - 1] = 1
    return ob


def cylinder_channel(D):
    """the 2D-1 case at D cells per diameter (a multiple of 10, so that 4.1 D is whole): a dict of the obstacle map `ob`, the
    body map `body` (the disc alone), `u_in`, `omega`, `omega_m` (Lambda = 3/16) and the constants.  The wall planes lie half
    a cell inside the wall rows 0 and ny - 1, at y = 1/2 and y = ny - 3/2, and the inlet plane on column 0."""
    assert D % 10 == 0 and D > 0
    nx, ny = 22 * D, (41 * D) // 10 + 2
    cx, cy, r = 2.0 * D, 0.5 + 2.0 * D, 0.5 * D
    yy, xx = np.mgrid[0:ny, 0:nx]
    body = (((xx - cx) ** 2 + (yy - cy) ** 2) <= r * r).astype(np.int32)
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    ob |= body
    nu = U_MEAN * D / REYNOLDS
    omega = 1.0 / (3.0 * nu + 0.5)
    return {"D": D, "nx": nx, "ny": ny, "cx": cx, "cy": cy, "r": r, "ob": ob, "body": body, "u_mean": U_MEAN, "nu": nu,
            "u_in": _open_ref.poiseuille(ny, 1.5 * U_MEAN), "omega": omega, "omega_m": _trt_ref.omega_minus(omega, MAGIC),
            "magic": MAGIC, "density": DENSITY, "rho_out": DENSITY}


def coefficients(fx, fy, D):
    """(C_d, C_l) = 2 (F_x, F_y) / (rho U_mean^2 D); fx and fy numbers or arrays"""
    s = 2.0 / (DENSITY * U_MEAN * U_MEAN * D)
    return np.asarray(fx, dtype=np.float64) * s, np.asarray(fy, dtype=np.float64) * s


def mirrored(case):
    """the same case flipped in y: the disc nearer the upper wall, the same drag and the opposite lift"""
    out = dict(case)
    out["ob"] = np.ascontiguousarray(case["ob"][::-1])
    out["body"] = np.ascontiguousarray(case["body"][::-1])
    out["u_in"] = np.ascontiguousarray(case["u_in"][::-1])
    out["cy"] = (case["ny"] - 1) - case["cy"]
    return out


def rest(case):
    return _open_ref.rest_state(case["density"], case["ny"], case["nx"]).copy()


def step(f, case, trt=True):
    return _open_ref.step(f, case["ob"], case["omega"], case["omega_m"] if trt else None, case["u_in"], case["rho_out"])[0]


def force(f, case):
    return _open_ref.force(f, case["ob"], case["body"])

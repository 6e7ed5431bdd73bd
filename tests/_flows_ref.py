"""Flows with a known answer, for tests/test_flows_gpu.py, tests/test_flows_restatement_cpu.py and tests/golden/make_flows.py:
geometry, figures, the fixture tests/golden/flows.json and the gates on its figures.  A step is _open_ref.step, a force is
_open_ref.force; nothing of the method is restated here.

The channel: 32x11, walls on rows 0 and 10, poiseuille(11, 0.01) at the inlet, density = rho_out = 0.1, from rest.  Halfway
bounce-back puts the wall planes half a cell outside the first fluid rows, where poiseuille() has its zeros; where the computed
profile has its own depends on the collision.  `shape` of _open_ref.channel_figures measures the difference.

The cylinder: Schaefer and Turek's benchmark 2D-1 at Re = 20 (Benchmark computations of laminar flow around a cylinder, Notes
on Numerical Fluid Mechanics 52, 1996).  In cylinder diameters D: a channel 22 long and 4.1 between the wall planes, the
centre 2 behind the inlet and 2 above the lower wall plane, a parabolic inlet with U_mean = 2/3 U_max, Re = U_mean D / nu.
Published bounds: C_d 5.57 - 5.59, C_l 0.0104 - 0.0110, C = 2 F / (rho U_mean^2 D)."""
import json
import os

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


# ---- tests/golden/flows.json and the gates on its figures and on the library's -----------------------------------------------
# The gates are conditions that the answer known from outside sets, not figures of the code under test;
# tests/test_flows_restatement_cpu.py says why, and applies them to the fixture's figures, tests/test_flows_gpu.py to the library's.

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
L316, L14 = 3.0 / 16.0, 0.25
BGK_OMEGAS = (0.6, 1.0, 1.7)


def fixture():
    with open(os.path.join(GOLDEN, "flows.json")) as f:
        return json.load(f)


def channel_table(fix):
    """{(magic or None, omega): (spread, shape)} of the fixture; the diverged BGK entry holds NaNs"""
    nan = float("nan")
    return {(e["magic"], e["omega"]): (nan if e["spread"] is None else e["spread"], nan if e["shape"] is None else e["shape"])
            for e in fix["channel"]["entries"]}


def channel_gates(fig):
    """fig {(magic or None, omega): (spread, shape)} with Lambda = 3/16 and 1/4 at the four omegas and BGK at 0.6, 1.0, 1.7"""
    lines = []
    for magic in (L316, L14):
        shapes = [fig[(magic, w)][1] for w in CH_OMEGAS]
        assert all(s > 0.0 for s in shapes)
        lines.append("Lambda %.4f: shape %s, max / min %.4f (gate 1.1)" % (magic, " ".join("%.4e" % s for s in shapes),
                                                                          max(shapes) / min(shapes)))
        assert max(shapes) / min(shapes) <= 1.1, (magic, shapes)                 # the wall does not move with omega
    bgk = [fig[(None, w)][1] for w in BGK_OMEGAS]
    lines.append("BGK: shape %s, max / min %.2f (gate >= 10)" % (" ".join("%.4e" % s for s in bgk), max(bgk) / min(bgk)))
    assert min(bgk) > 0.0 and max(bgk) / min(bgk) >= 10.0, bgk                   # the figure is not blind: with BGK it moves
    for w in CH_OMEGAS:
        s316, s14 = fig[(L316, w)][1], fig[(L14, w)][1]
        lines.append("omega %.1f: shape at 3/16 %.4e (gate 1e-4), at 1/4 %.4e, ratio %.1f (gate >= 100), 1/4 against BGK at 1: %.2e "
                     "(gate 1e-3)" % (w, s316, s14, s14 / s316, abs(s14 - fig[(None, 1.0)][1]) / fig[(None, 1.0)][1]))
        assert s316 <= 1e-4, (w, s316)                                           # half-way: the parabola itself
        assert s14 >= 100.0 * s316, (w, s14, s316)
        assert abs(s14 - fig[(None, 1.0)][1]) <= 1e-3 * fig[(None, 1.0)][1], (w, s14, fig[(None, 1.0)][1])
    for (magic, w), (spread, _) in sorted(fig.items(), key=str):
        if w <= 1.7:
            lines.append("%s omega %.1f: spread %.2e (gate 1e-9)" % ("BGK" if magic is None else "Lambda %.4f" % magic, w, spread))
            assert abs(spread) <= 1e-9, (magic, w, spread)                       # one flux through every column: settled
    return lines


def tail_of(fx, fy, D, tail=6000):
    """the figures of a record's last `tail` entries, as the fixture's "tail" holds them"""
    cd, cl = coefficients(fx[-tail:], fy[-tail:], D)
    assert cd.shape == (tail,)
    return {"cd_mean": float(cd.mean()), "cd_min": float(cd.min()), "cd_max": float(cd.max()), "cl_mean": float(cl.mean())}


def cylinder_gates(t):
    """t: the figures of the last 6 000 steps at D = 10"""
    cd, cl, swing = t["cd_mean"], t["cl_mean"], (t["cd_max"] - t["cd_min"]) / t["cd_mean"]
    line = ("D 10: C_d %.4f (%+.2f %% of 5.58, gate 7 %%), max - min %.3f %% (gate 0.2 %%), C_l %.5f (%+.1f %% of 0.0107, gate 25 %%)"
            % (cd, 100.0 * (cd / CD_PUBLISHED - 1.0), 100.0 * swing, cl, 100.0 * (cl / CL_PUBLISHED - 1.0)))
    assert abs(cd - CD_PUBLISHED) <= 0.07 * CD_PUBLISHED, line
    assert 0.0 <= swing <= 2e-3, line
    assert cl > 0.0 and abs(cl - CL_PUBLISHED) <= 0.25 * CL_PUBLISHED, line   # the disc is nearer the lower wall
    return line


def mirror_gates(t0, t1, stored):
    """the mirrored member: the same C_d, the opposite C_l, each within 100 x what the restatement's two runs differ by and
    1e-6 of C_d at the most (a flipped sign or a wrong member's record is 1e-2)"""
    d_cd, d_cl = abs(t0["cd_mean"] - t1["cd_mean"]), abs(t0["cl_mean"] + t1["cl_mean"])
    cap = 1e-6 * t0["cd_mean"]
    g_cd, g_cl = min(100.0 * stored["d_cd"], cap), min(100.0 * stored["d_cl"], cap)
    line = "mirrored member: |C_d - C_d'| %.2e (gate %.2e), |C_l + C_l'| %.2e (gate %.2e)" % (d_cd, g_cd, d_cl, g_cl)
    assert d_cd <= g_cd and d_cl <= g_cl, line
    return line


def finer_gates(t20, t10):
    """D = 20 against D = 10: nearer the published drag, and within 5 % of it"""
    e20, e10 = abs(t20["cd_mean"] - CD_PUBLISHED), abs(t10["cd_mean"] - CD_PUBLISHED)
    line = "D 20: C_d %.4f (%+.2f %% of 5.58, gate 5 %% and below D 10's %+.2f %%), C_l %.5f" % (
        t20["cd_mean"], 100.0 * (t20["cd_mean"] / CD_PUBLISHED - 1.0), 100.0 * (t10["cd_mean"] / CD_PUBLISHED - 1.0),
        t20["cl_mean"])
    assert e20 < e10 and e20 <= 0.05 * CD_PUBLISHED, line
    return line

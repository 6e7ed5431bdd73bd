"""tests/_les_ref.py, the numpy restatement of include/lbm.h's "Subgrid viscosity", held to what does not need a GPU.

  1. With c None (and 0.0) the restatement returns the arrays of _wall_ref.step, bit for bit: BGK and TRT, with and without open
     boundaries and moving walls, on 33x19 and 17x16.
  2. les_k is the header's two host statements, evaluated in Python floats.
  3. Couette flow: the 16 x 16 channel of _wall_ref.COUETTE (U = 0.05, rho = rho_wall = 0.1, omega = 1.2, accel 0), from rest, 6000
     steps, c = 2.0.  A steady shear has |S| = U / H, so the force on each wall must be rho (nu + c^2 U / H) U nx / H with H =
     ny - 2, and the fluid-row profile must stay linear.  The restatement misses the force by 3.6e-6 (BGK) and 5.5e-6 (TRT,
     Lambda = 3/16) relative and the profile by 2.7e-6 U and 4.1e-6 U; the gate is 1e-4 on both, about 18 x that and 1/1300 of
     the 12.9 % by which the molecular viscosity alone misses - and the plain formula is asserted to fail the gate.
  4. The lid-driven cavity separates BGK from the model: 32 x 32, the four edge rows and columns blocked, row ny - 1 moving with
     U = 0.1 on columns 1 .. nx - 2, rho = rho_wall = 0.1, omega = 1.99, accel 0, from rest.  BGK is non-finite before step 2000
     (step 716 was observed); c = 0.17 is finite with positive densities after 3000 steps and max |u| < U (0.0811 was observed).
  5. On random states the moment form of pxx, pyy, pxy equals sum_k c_a c_b (g_k - eq_k) within 64 * 2^-53 * sum |g_k|: a
     generous bound on purpose, it guards against a slip of sign or index."""
import numpy as np
import pytest

import _les_ref
import _open_ref
import _trt_ref
import _wall_ref
from _les_ref import GATE, couette_figures
from _wall_ref import COUETTE

U53 = 2.0 ** -53
_couette, _cavity = {}, {}


# ---- 1. off is _wall_ref.step ------------------------------------------------------------------------------------------------

def random_case(nx, ny, seed):
    rng = np.random.default_rng(seed)
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    ob[ny // 2 - 2:ny // 2 + 2, nx // 4:nx // 4 + 5] = 1
    ob[3, 0] = ob[2, nx - 1] = 1
    w = np.array([4.0 / 9.0] + [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4).reshape(9, 1, 1)
    f = w * 0.1 * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5))
    u_x = np.where(ob != 0, 0.1 * (rng.random((ny, nx)) - 0.5), 0.0)
    u_y = np.where(ob != 0, 0.1 * (rng.random((ny, nx)) - 0.5), 0.0)
    u_x[0] = u_y[0] = 0.0
    return ob, f, (u_x, u_y, 0.0985)


@pytest.mark.parametrize("nx,ny", [(33, 19), (17, 16)])
@pytest.mark.parametrize("walled", [False, True])
@pytest.mark.parametrize("opened", [False, True])
@pytest.mark.parametrize("magic", [None, 3.0 / 16.0])
def test_off_returns_the_arrays_of_wall_ref(magic, opened, walled, nx, ny):
    ob, f, wall = random_case(nx, ny, 100 * nx + ny)
    setting = (_open_ref.poiseuille(ny, 0.03), 0.1) if opened else (None, None)
    om = _trt_ref.omega_minus(1.3, magic) if magic else None
    want, want_u = _wall_ref.step(f, ob, 1.3, om, *setting, wall=wall if walled else None)
    for c in (None, 0.0):
        got, got_u = _les_ref.step(f, ob, 1.3, magic, *setting, wall=wall if walled else None, c=c)
        assert got.tobytes() == want.tobytes() and got_u.tobytes() == want_u.tobytes()
    # and on is another flow, on fluid cells alone
    on, _ = _les_ref.step(f, ob, 1.3, magic, *setting, wall=wall if walled else None, c=0.17)
    fluid = ob == 0
    assert np.all(np.isfinite(on)) and not np.array_equal(on[:, fluid], want[:, fluid])
    assert on[:, ~fluid].tobytes() == want[:, ~fluid].tobytes()


# ---- 2. the host statements --------------------------------------------------------------------------------------------------

def test_les_k_is_the_headers_host_statements():
    import math
    for omega, c in ((1.2, 2.0), (1.99, 0.17), (1.0, 0.1), (1.7, 0.3)):
        tau0, les_k = _les_ref.constants(omega, c)
        assert tau0 == 1.0 / omega
        assert les_k == (18.0 * math.sqrt(2.0)) * (c * c)
    assert math.sqrt(2.0) == 1.4142135623730951                       # the correctly rounded double
    assert abs(_les_ref.constants(1.0, 0.17)[1] - 25.455844122715710 * 0.0289) < 1e-14   # 18 sqrt(2) = 25.4558441227157...


# ---- 3. Couette flow ---------------------------------------------------------------------------------------------------------

def couette_run(trt):
    """(the state one step before the last, the settled state) of the Couette case with c = COUETTE_C, once per operator"""
    if trt not in _couette:
        c = COUETTE
        ob, u_x, u_y = _wall_ref.couette_maps()
        f = _open_ref.rest_state(c["rho"], c["ny"], c["nx"])
        before = f
        for _ in range(c["steps"]):
            before = f
            f, _ = _les_ref.step(f, ob, c["omega"], c["magic"] if trt else None, wall=(u_x, u_y, c["rho"]), c=_les_ref.COUETTE_C)
        _couette[trt] = (before, f)
    return _couette[trt]


@pytest.mark.parametrize("trt", [False, True])
def test_couette_gives_the_analytic_wall_force(trt):
    before, f = couette_run(trt)
    top, bottom, plain, err = couette_figures(before, f)
    print("Couette %s with c = %g: F_x within %.2e (top) %.2e (bottom) of rho (nu + c^2 U / H) U nx / H, %.2e of the molecular "
          "formula; profile within %.2e U" % ("TRT" if trt else "BGK", _les_ref.COUETTE_C, top, bottom, plain, err))
    assert top <= GATE and bottom <= GATE
    assert err <= GATE
    assert plain > GATE and plain > 0.1                                # the molecular viscosity alone misses by 12.9 %
    c = COUETTE
    assert all(np.array_equal(_wall_ref.column_velocity(f, x), _wall_ref.column_velocity(f, 0)) for x in range(c["nx"]))


# ---- 4. the cavity -----------------------------------------------------------------------------------------------------------

def cavity_run(c_smag, steps):
    """(first step after which the state is not finite, or None; the last state; the smallest om seen on a fluid cell)"""
    key = (c_smag, steps)
    if key not in _cavity:
        v = _les_ref.CAVITY
        ob, u_x, u_y = _les_ref.cavity_maps()
        fluid = ob == 0
        f = _open_ref.rest_state(v["rho"], v["ny"], v["nx"])
        blew, om_min = None, np.inf
        with np.errstate(all="ignore"):
            for t in range(1, steps + 1):
                if c_smag:
                    om_min = min(om_min, float(np.min(_les_ref.effective_omega(f, ob, v["omega"], c_smag)[fluid])))
                f, _ = _les_ref.step(f, ob, v["omega"], None, wall=(u_x, u_y, v["rho"]), c=c_smag)
                if not np.all(np.isfinite(f)):
                    blew = t
                    break
        _cavity[key] = (blew, f, om_min)
    return _cavity[key]


def test_the_cavity_separates_bgk_from_the_model():
    v = _les_ref.CAVITY
    ob, _, _ = _les_ref.cavity_maps()
    blew, _, _ = cavity_run(None, v["bgk_limit"])
    print("cavity %dx%d omega %g lid %g: BGK is not finite after step %s" % (v["nx"], v["ny"], v["omega"], v["U"], blew))
    assert blew is not None and blew < v["bgk_limit"]
    blew, f, om_min = cavity_run(v["c"], v["steps"])
    assert blew is None and np.all(np.isfinite(f))
    umax, rho_min = _les_ref.velocity_magnitude(f, ob)
    print("  c = %g: finite after %d steps, max |u| %.4f, min density %.4f, smallest om %.4f" % (v["c"], v["steps"], umax, rho_min, om_min))
    assert rho_min > 0.0 and np.all(f[:, ob == 0] > 0.0)
    assert 0.0 < umax < v["U"]
    assert om_min < v["omega"]


# ---- 5. the moment form of the stress ----------------------------------------------------------------------------------------

def test_the_moment_form_is_the_second_moment_of_the_non_equilibrium_part():
    rng = np.random.default_rng(17)
    w = np.array([4.0 / 9.0] + [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4)
    g = [w[k] * 0.1 * (1.0 + 0.4 * (rng.random((40, 50)) - 0.5)) for k in range(9)]
    pxx, pyy, pxy, q, _ = _les_ref.stress(g)
    # the equilibrium of _trt_ref.step, restated: only to have eq[k] - g[k] to sum
    dens, densinv, jx, jy = _les_ref.moments(g)
    ux, uy = jx * densinv, jy * densinv
    usq = ux * ux + uy * uy
    cx, cy = np.array(_trt_ref.CX, dtype=np.float64), np.array(_trt_ref.CY, dtype=np.float64)
    eq = [w[k] * dens * (1.0 + 3.0 * (cx[k] * ux + cy[k] * uy) + 4.5 * (cx[k] * ux + cy[k] * uy) ** 2 - 1.5 * usq) for k in range(9)]
    want = {}
    for name, a, b in (("xx", cx, cx), ("yy", cy, cy), ("xy", cx, cy)):
        want[name] = sum(a[k] * b[k] * (g[k] - eq[k]) for k in range(9))
    bound = 64.0 * U53 * sum(np.abs(g[k]) for k in range(9))
    worst = 0.0
    for got, name in ((pxx, "xx"), (pyy, "yy"), (pxy, "xy")):
        err = np.abs(got - want[name])
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), name
    print("moment form against sum c_a c_b (g_k - eq_k): within %.3f of the bound" % worst)
    assert np.all(q > 0.0) and float(np.max(np.abs(pxy))) > 1e3 * float(np.max(bound))       # the bound is far below the signal
    assert np.array_equal(q, np.sqrt((pxx * pxx + pyy * pyy) + 2.0 * (pxy * pxy)))

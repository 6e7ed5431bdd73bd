"""tests/_wall_ref.py, the numpy restatement of include/lbm.h's "Moving walls", held to what does not need a GPU.

  1. Couette flow: 16 x 16, rows 0 and 15 blocked, the top wall moving with u_x = U = 0.05, rho_wall 0.1, omega 1.2, accel 0,
     from rest, 6000 steps, with BGK and with TRT (Lambda = 3/16).  The column profile equals U (y - 1/2) / (ny - 2) within
     1e-10 U (both walls sit half-way; a throw-away restatement gave 3.2e-13 U with TRT and 3.5e-13 U with BGK), and the
     unchanged momentum-exchange sum gives F_x = -rho nu U nx / H with the top wall as body and +rho nu U nx / H with the bottom
     wall, to 1e-9 relative (about 1e-13 was observed).  accel is 0, so accelerate_flow adds 0.0 to positive values and is
     left out.
  2. A map whose velocities are all +-0.0 is _open_ref.step bit for bit, with -0.0 stored in a blocked cell.
  3. One hand-computed moving cell: the six intermediate values, the nine values the cell writes and the |u| it returns,
     sixteen in all, against the header's statements evaluated in Python floats."""
import numpy as np
import pytest

import _open_ref
import _trt_ref
import _wall_ref
from _force_ref import body_restatement
from _wall_ref import COUETTE, couette_run


@pytest.mark.parametrize("trt", [False, True])
def test_couette_profile_is_linear(trt):
    c = COUETTE
    _, f, u = couette_run(trt)
    got = _wall_ref.column_velocity(f, c["nx"] // 2)
    err = float(np.max(np.abs(got - _wall_ref.couette_profile(c["ny"], c["U"])))) / c["U"]
    print("Couette %s: max |u_x - U (y - 1/2) / H| = %.2e U" % ("TRT" if trt else "BGK", err))
    assert err <= 1e-10
    # the flow is the same in every column, and a blocked cell returns |u| = 0 whether it moves or not
    assert all(np.array_equal(_wall_ref.column_velocity(f, x), got) for x in range(c["nx"]))
    assert np.all(u[0] == 0.0) and np.all(u[c["ny"] - 1] == 0.0) and np.all(u[1:c["ny"] - 1] > 0.0)
    # a wall velocity along the wall conserves mass
    mass = float(np.sum(f[:, 1:c["ny"] - 1]))
    assert abs(mass - c["rho"] * c["nx"] * (c["ny"] - 2)) <= 1e-9 * mass


@pytest.mark.parametrize("trt", [False, True])
def test_couette_wall_forces_are_the_shear(trt):
    c = COUETTE
    before, _, _ = couette_run(trt)
    ob, _, _ = _wall_ref.couette_maps()
    want = _wall_ref.couette_force(c["nx"], c["ny"], c["U"], c["rho"], c["omega"])
    assert abs(want - 6.3492063492e-4) < 1e-13
    for row, sign in ((c["ny"] - 1, -1.0), (0, +1.0)):
        body = np.zeros_like(ob)
        body[row] = 1
        fx, fy, links, _ = body_restatement(before, ob, body)
        rel = abs(fx - sign * want) / want
        print("Couette %s: F_x on wall row %d = %+.13e, %+.13e expected (%.1e relative)" %
              ("TRT" if trt else "BGK", row, fx, sign * want, rel))
        assert links == 3 * c["nx"]
        assert rel <= 1e-9


def random_case(seed, ny=9, nx=11):
    rng = np.random.default_rng(seed)
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    ob[3:5, 4:7] = 1
    f = np.array([4.0 / 9.0] + [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4).reshape(9, 1, 1) * 0.1 * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5))
    return ob, f


@pytest.mark.parametrize("opened", [False, True])
def test_a_map_of_zeros_is_the_step_without_walls_bit_for_bit(opened):
    ob, f = random_case(5)
    f[3, 0, 2] = -0.0                        # stored in a blocked cell: plain bounce-back hands the sign on to speed 1
    f[6, 4, 5] = -0.0
    ny, nx = ob.shape
    setting = (_open_ref.poiseuille(ny, 0.03), 0.1) if opened else (None, None)
    want, want_u = _open_ref.step(f, ob, 1.3, _trt_ref.omega_minus(1.3, 0.25), *setting)
    zeros = np.zeros((ny, nx))
    signed = np.where(np.arange(nx)[None, :] % 2 == 0, 0.0, -0.0) * np.ones((ny, 1))
    assert np.any(np.signbit(signed)) and np.all(signed == 0.0)
    for wall in (None, (zeros, zeros, 0.1), (signed, -signed, 0.1), (signed, zeros, 0.1)):
        got, got_u = _wall_ref.step(f, ob, 1.3, _trt_ref.omega_minus(1.3, 0.25), *setting, wall=wall)
        assert got.tobytes() == want.tobytes()           # every bit, signed zeros included
        assert got_u.tobytes() == want_u.tobytes()
    # the -0.0 went through the blocked cell as it was: a cell that added +0.0 would have lost the sign
    assert np.signbit(want[1, 0, 1]) and want[1, 0, 1] == 0.0     # g[3] of cell (0, 1) is f_3 of cell (0, 2)
    # a velocity on a fluid cell is not read
    on_fluid = zeros.copy()
    on_fluid[2, 2] = 0.04
    assert ob[2, 2] == 0
    got, _ = _wall_ref.step(f, ob, 1.3, None, wall=(on_fluid, zeros, 0.1))
    assert got.tobytes() == _open_ref.step(f, ob, 1.3, None)[0].tobytes()


def test_one_moving_cell_by_hand():
    ob, f = random_case(11)
    y, x = 4, 5
    assert ob[y, x] != 0
    ux, uy, rho = 0.03, -0.0125, 0.0985
    u_x, u_y = np.zeros(ob.shape), np.zeros(ob.shape)
    u_x[y, x], u_y[y, x] = ux, uy
    g = [float(a[y, x]) for a in _trt_ref.gather(f)]
    # the header's statements, one Python float operation per operator
    rx = rho * ux
    ry = rho * uy
    a = (2.0 / 3.0) * rx
    b = (2.0 / 3.0) * ry
    p = (1.0 / 6.0) * (rx + ry)
    q = (1.0 / 6.0) * (ry - rx)
    want = [g[0], g[3] + a, g[4] + b, g[1] - a, g[2] - b, g[7] + p, g[8] + q, g[5] - p, g[6] - q]
    ta, tb, tp, tq = (float(v[y, x]) for v in _wall_ref.terms(u_x, u_y, rho))
    assert (ta, tb, tp, tq) == (a, b, p, q)
    assert (rx, ry) == (float(np.float64(rho) * np.float64(ux)), float(np.float64(rho) * np.float64(uy)))
    cells, u = _wall_ref.step(f, ob, 1.1, None, wall=(u_x, u_y, rho))
    for k in range(9):
        assert float(cells[k, y, x]) == want[k], k
    assert u[y, x] == 0.0
    # the values are bounce-back plus 6 w_k rho_wall c_k . u_wall, and what the cell adds sums to no mass
    for k, w in zip(range(1, 9), [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4):
        add = 6.0 * w * rho * (_trt_ref.CX[k] * ux + _trt_ref.CY[k] * uy)
        assert abs((want[k] - g[_trt_ref.OPP[k]]) - add) <= 4 * 2.0 ** -53 * abs(g[_trt_ref.OPP[k]])
    # every other cell is the step without walls
    plain, _ = _open_ref.step(f, ob, 1.1, None)
    other = np.ones(ob.shape, dtype=bool)
    other[y, x] = False
    assert cells[:, other].tobytes() == plain[:, other].tobytes() and not np.array_equal(cells[:, y, x], plain[:, y, x])

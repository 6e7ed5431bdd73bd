"""The numpy restatement of the open boundaries (tests/_open_ref.py) held to what is known without a GPU: the control that
makes the bit comparison of tests/test_open_gpu.py mean something.

  1. with the setting off its step is _trt_ref.step, bit for bit;
  2. after one open step from a random positive state on 16x16 and 33x19 with walls, every fluid cell of column 0 carries
     u_in[y] as jx / rho and every fluid cell of column nx - 1 carries rho_out as its density, within 4 ulp.  The unit: jx is
     a sum of six populations and rho of nine, each addition rounds at the magnitude of the populations, that is of rho, not
     at that of u rho.  So the density is held to 4 ulp of rho_out, and the velocity to 4 ulp of the ratio's scale, 1.0:
     |jx / rho - u| <= 4 * 2^-52, which says jx is within 4 ulp(rho) of rho u.  In ulp of u itself the figure has no bound
     independent of u (measured: 38 at U = 0.05, 150 at U = 0.01); both figures are printed.
  3. the channel check of the issue: 32x11, walls on rows 0 and 10, density = rho_out = 0.1 from rest, the parabola of
     _open_ref.poiseuille with U = 0.01 at the inlet, 8000 steps at omega 1.0 and 1.7.  The spread (max - min) / mean over the
     columns of the flux sum_y jx is below 1e-7 (measured: 2.4e-13 and 8.9e-11 with TRT, 2.7e-13 and 4.0e-10 with BGK); with
     TRT at Lambda = 3/16 the mid-column shape error max|m / sum m - p / sum p| (ny - 2) is below 1e-4 (measured 2.1e-5 at both
     rates), with BGK in the same runs above 1e-3 (measured 4.2e-3 and 1.2e-2): the check tells the half-way wall from a
     displaced one."""
import numpy as np
import pytest

import _open_ref
import _trt_ref
from _dp_states import random_state

MAGIC = 3.0 / 16.0
ULP1 = 2.0 ** -52


def walled(nx, ny):
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    return ob


@pytest.mark.parametrize("nx,ny", [(16, 16), (33, 19)])
def test_off_is_the_periodic_step_bit_for_bit(nx, ny):
    f = random_state(np.random.default_rng(nx), 0.1, ny, nx)
    ob = walled(nx, ny)
    ob[ny // 2, nx // 3] = 1
    for om in (None, _trt_ref.omega_minus(1.7, MAGIC)):
        got, want = _open_ref.step(f, ob, 1.7, om), _trt_ref.step(f, ob, 1.7, om)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # and the identity fix composes to the same step: gather, ungather is exact
        again = _trt_ref.step(_open_ref.ungather(_open_ref.gather(f)), ob, 1.7, om)
        assert np.array_equal(again[0], want[0])


@pytest.mark.parametrize("trt", [False, True])
@pytest.mark.parametrize("nx,ny", [(16, 16), (33, 19)])
def test_one_step_sets_the_inlet_velocity_and_the_outlet_density(nx, ny, trt):
    f = random_state(np.random.default_rng(nx), 0.1, ny, nx)
    ob = walled(nx, ny)
    u_in, rho_out = _open_ref.poiseuille(ny, 0.05), 0.1
    om = _trt_ref.omega_minus(1.7, MAGIC) if trt else None
    cells, _ = _open_ref.step(f, ob, 1.7, om, u_in, rho_out)
    periodic, _ = _trt_ref.step(f, ob, 1.7, om)
    assert not np.array_equal(cells, periodic)
    assert np.array_equal(cells[:, :, 1:nx - 1], periodic[:, :, 1:nx - 1])          # the fix is local to the two columns
    rho = cells.sum(axis=0)
    u = _open_ref.jx_of(cells) / rho
    fluid = ob[:, 0] == 0
    du = np.abs(u[:, 0] - u_in)[fluid]
    drho = np.abs(rho[:, nx - 1] - rho_out)[ob[:, nx - 1] == 0]
    print("%dx%d %s: inlet |jx/rho - u| up to %.2f ulp(1.0) (%.1f ulp of u), outlet |rho - rho_out| up to %.2f ulp" %
          (nx, ny, "TRT" if trt else "BGK", du.max() / ULP1, (du / np.spacing(u_in[fluid])).max(), drho.max() / np.spacing(rho_out)))
    assert np.all(du <= 4.0 * ULP1)
    assert np.all(drho <= 4.0 * np.spacing(rho_out))
    # the periodic step of the same state carries neither
    rho_p = periodic.sum(axis=0)
    assert np.max(np.abs((_open_ref.jx_of(periodic) / rho_p)[:, 0] - u_in)[fluid]) > 1e-3
    assert np.max(np.abs(rho_p[:, nx - 1] - rho_out)[fluid]) > 1e-4


_channel = {}


def channel_run(omega, trt):
    key = (omega, trt)
    if key not in _channel:
        nx, ny, u_max = 32, 11, 0.01
        ob = walled(nx, ny)
        u_in = _open_ref.poiseuille(ny, u_max)
        om = _trt_ref.omega_minus(omega, MAGIC) if trt else None
        f = _open_ref.rest_state(0.1, ny, nx)
        for _ in range(8000):
            f, _u = _open_ref.step(f, ob, omega, om, u_in, 0.1)
        _channel[key] = _open_ref.channel_figures(f, u_max)
    return _channel[key]


@pytest.mark.parametrize("omega", [1.0, 1.7])
def test_channel_check(omega):
    spread_trt, shape_trt = channel_run(omega, True)
    spread_bgk, shape_bgk = channel_run(omega, False)
    print("32x11 omega %.1f after 8000 steps: flux spread TRT %.2e BGK %.2e; shape error TRT %.2e BGK %.2e" %
          (omega, spread_trt, spread_bgk, shape_trt, shape_bgk))
    assert 0.0 <= spread_trt < 1e-7 and 0.0 <= spread_bgk < 1e-7
    assert shape_trt < 1e-4
    assert shape_bgk > 1e-3

"""The numpy restatement of the two-relaxation-time collision (tests/_trt_ref.py) held to what is known without a GPU: the
control that makes the bit comparison of tests/test_trt_gpu.py mean something.

  1. in BGK mode it equals the fp64 oracle's pairwise no-FMA build (the statements dp_collide_cell restates) bit for bit;
  2. in TRT mode a step conserves mass to _dp_states.MASS_REL;
  3. in TRT mode the fluid momentum it takes out of a step is the momentum-exchange force of _force_ref.restatement, within
     gate 2 of tests/test_force_gpu.py (2 9N 2^-53 sum|f|);
  4. Lambda = 1/4 at omega = 1 gives omega_m = 1 exactly, and that degenerate TRT step stays within 2^-53 (2|out| + 6|out - g|)
     of the BGK step: five more roundings of the increment (a + b, a - b, their halves are exact, rp + rm; |a + b| / 2 and
     |a - b| / 2 counted with |out - g| each, hence 6 with the BGK increment's own) and the two final additions."""
import math

import numpy as np
import pytest

import _trt_ref
from _dp_states import MASS_REL, build_oracle_nofma, oracle_params
from _force_ref import accelerated, case, fluid_momentum, restatement

U = 2.0 ** -53
SHAPES = [(3, 3), (16, 16), (33, 19), (48, 35)]
MAGIC = 3.0 / 16.0
STEPS = 40


@pytest.fixture(scope="module")
def oracle_nofma(tmp_path_factory):
    return build_oracle_nofma(tmp_path_factory)


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_bgk_mode_equals_the_pairwise_oracle_bit_for_bit(lbm, oracle_nofma, nx, ny):
    p, ob, cells = case(lbm, nx, ny, STEPS)
    q = oracle_params(oracle_nofma, p)
    for t in range(STEPS):
        f = accelerated(oracle_nofma, p, ob, cells)
        ref = np.empty_like(f)
        oracle_nofma.timestep(q, f, ref, ob)
        got, u = _trt_ref.step(f, ob, p.omega)
        assert np.array_equal(got, ref), (nx, ny, t)
        assert np.all(u[ob != 0] == 0.0) and np.all(u[ob == 0] >= 0.0)
        cells = ref
    assert np.all(np.isfinite(cells))


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_trt_mode_conserves_mass_and_balances_momentum(lbm, oracle_nofma, nx, ny):
    p, ob, cells = case(lbm, nx, ny, 12)
    om = _trt_ref.omega_minus(p.omega, MAGIC)
    worst_mass = worst_mom = 0.0
    for t in range(12):
        f = accelerated(oracle_nofma, p, ob, cells)
        cells, _ = _trt_ref.step(f, ob, p.omega, om)
        rel = abs(math.fsum(cells.ravel().tolist()) / math.fsum(f.ravel().tolist()) - 1.0)
        worst_mass = max(worst_mass, rel)
        assert rel <= MASS_REL, (t, rel)
        fx, fy, links, _ = restatement(f, ob)
        tol = 2.0 * 9 * nx * ny * U * float(np.sum(np.abs(f)))
        bx, by = fluid_momentum(f, ob)
        ax, ay = fluid_momentum(cells, ob)
        worst_mom = max(worst_mom, abs((ax - bx) + fx) / tol, abs((ay - by) + fy) / tol)
        assert links > 0 and abs((ax - bx) + fx) <= tol and abs((ay - by) + fy) <= tol, (t, ax - bx, fx, ay - by, fy, tol)
    print("%dx%d TRT: mass per step within %.2e, momentum balance within %.2e of its gate" % (nx, ny, worst_mass, worst_mom))
    # and it is another operator: the BGK step of the last accelerated state differs
    bgk, _ = _trt_ref.step(f, ob, p.omega)
    assert float(np.max(np.abs(cells - bgk) / np.abs(bgk))) > 1e-3


def test_omega_minus():
    assert _trt_ref.omega_minus(1.0, 0.25) == 1.0
    # Lambda = (1/omega - 1/2)(1/omega_m - 1/2) to rounding, and omega_m inside (0, 2)
    for omega in (1.0, 1.2125, 1.7, 1.85):
        for magic in (3.0 / 16.0, 0.25, 1.0 / 12.0, 1.0 / 6.0):
            om = _trt_ref.omega_minus(omega, magic)
            assert 0.0 < om < 2.0
            assert abs((1.0 / omega - 0.5) * (1.0 / om - 0.5) / magic - 1.0) <= 8 * U


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_degenerate_trt_step_stays_within_its_roundings_of_the_bgk_step(lbm, oracle_nofma, nx, ny):
    p, ob, cells = case(lbm, nx, ny, 12)
    p.omega = 1.0
    worst = 0.0
    for t in range(12):
        f = accelerated(oracle_nofma, p, ob, cells)
        bgk, _ = _trt_ref.step(f, ob, 1.0)
        trt, u = _trt_ref.step(f, ob, 1.0, _trt_ref.omega_minus(1.0, 0.25))
        g = np.stack(_trt_ref.gather(f))
        bound = U * (2.0 * np.abs(bgk) + 6.0 * np.abs(bgk - g))
        diff = np.abs(trt - bgk)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0.0, diff / bound, 0.0))))
        assert np.all(diff <= bound), (t, float(np.max(diff - bound)))
        assert np.array_equal(trt[:, ob != 0], bgk[:, ob != 0])            # bounce-back is the same statement
        cells = bgk
    print("%dx%d: degenerate TRT within %.3e of the bound" % (nx, ny, worst))

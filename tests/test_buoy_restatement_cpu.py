"""The numpy restatement of buoyancy (tests/_buoy_ref.py) on the CPU: what it is tied to, the fixture it wrote, and the seeded
defects.

  1. ties: under a force that is the same on every cell, flow_step and fields are _drive_ref.step and _drive_ref.fields bit for
     bit, under every option (the restated wrappers add nothing); with C == c_ref the force is F0 exactly; a step with b = (0, 0)
     and no body force is the passive scalar's advance;
  2. the order of the device's sums (segment_sums, reduce) adds every cell once, on odd widths too;
  3. the fixture: every flow's probes after START steps are recomputed and equal tests/golden/buoy.json to 1e-9 relative, and the
     fixture's full-length figures meet the gates the GPU module applies: the stratified layer at rest at rounding level, max |u_y|
     falling at Ra 1500 and rising at Ra 1900, Ra_c by interpolation within twice the restatement's own deviation of 1707.76 (it is
     2.4 % above it at H = 16), the cavity's Nusselt number within twice its own deviation of de Vahl Davis's 1.118 (0.11 % below);
  4. seeded defects: the sign of b flipped, the output stage's half-force left out, the flow reading the scalar's old array, F0
     dropped - each run for START steps misses the fixture's probes of at least one flow by far more than the 1e-9 the gate allows."""
import numpy as np
import pytest

import _buoy_ref as bref
import _drive_ref
import _dp_matrix as dm
import _scalar_ref as sref
from _dp_states import random_state


@pytest.fixture(scope="module")
def fix():
    return bref.fixture()


def small(nx=11, ny=9, seed=3):
    ob, _ = dm.matrix_mask(nx, ny)
    return ob, random_state(np.random.default_rng(seed), 0.1, ny, nx)


@pytest.mark.parametrize("magic,opened,wall,les", [(None, False, False, None), (3.0 / 16.0, False, False, None), (None, True, False, None),
                                                   (None, False, True, None), (None, False, False, 0.17), (0.25, True, True, 0.3)])
def test_a_uniform_force_is_the_body_force(magic, opened, wall, les):
    nx, ny = 11, 9
    ob, f = small(nx, ny)
    drive = (4e-5, -1e-5)
    F = (np.full((ny, nx), drive[0]), np.full((ny, nx), drive[1]))
    u_in, rho_out = (dm.inlet_profile(nx, ny, 0), 0.1) if opened else (None, None)
    w = dm.member_wall(type("m", (), {"ob": ob}), 0, nx, ny) if wall else None
    got = bref.flow_step(f, ob, 1.2, F, magic, u_in, rho_out, w, les)
    want = _drive_ref.step(f, ob, 1.2, magic, u_in, rho_out, w, les, drive)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert all(np.array_equal(a, b) for a, b in zip(bref.fields(f, ob, 0.1, F), _drive_ref.fields(f, ob, 0.1, drive)))
    assert not np.array_equal(got[0], _drive_ref.step(f, ob, 1.2, magic, u_in, rho_out, w, les)[0])


def test_the_force_statements():
    rng = np.random.default_rng(5)
    g = sref.init(np.full((4, 6), 0.75))
    fx, fy = bref.force(g, (3e-5, -2e-5), float(sref.field(g, np.zeros((4, 6)))[0, 0]), (1e-6, 0.0))
    assert np.all(fx == 1e-6) and np.all(fy == 0.0)                             # C == c_ref: F0 exactly
    g = sref.init(0.5 + rng.random((4, 6)))
    c = sref.field(g, np.zeros((4, 6)))
    fx, fy = bref.force(g, (3e-5, -2e-5), 1.0)
    assert np.array_equal(fx, 0.0 + 3e-5 * (c - 1.0)) and np.array_equal(fy, 0.0 + -2e-5 * (c - 1.0))
    sx, sy = bref.force(g, (3e-5, -2e-5), 1.0, defect="sign")
    assert np.array_equal(sx, -fx) and np.array_equal(sy, -fy)


def test_without_buoyancy_a_step_is_the_passive_scalars():
    nx, ny = 11, 9
    ob, f = small(nx, ny)
    g = sref.init(0.5 + np.random.default_rng(9).random((ny, nx)))
    s = bref.setting(ob, 0.1, 0.005, 1.2, (0.0, 0.0), 0.3, 0.05)
    f1, g1 = bref.advance(f, g, s)[:2]
    # the passive path has no force at all; with F = +0.0 on every cell the source adds +0.0 and the shift adds +0.0
    p1, q1 = sref.advance(f, g, sref.flow(ob, 0.1, 0.005, 1.2), sref.omega_s(0.05))
    assert np.array_equal(g1, q1) and np.array_equal(f1, p1)


@pytest.mark.parametrize("nx,ny", [(33, 19), (17, 16), (6, 5)])
def test_the_order_of_the_sums_adds_every_cell_once(nx, ny):
    v = np.random.default_rng(nx).random((ny, nx))
    seg = bref.segment_sums(v)
    assert seg.shape == (ny * -(-nx // 16),)
    assert abs(bref.reduce(seg) - np.sum(v)) <= 1e-13 * np.sum(v)
    one = np.zeros((ny, nx))
    one[ny - 1, nx - 1] = 1.0
    assert bref.reduce(bref.segment_sums(one)) == 1.0


def test_the_fixtures_probes(fix):
    assert fix["start"] == bref.START
    for name, make in bref.SHORT.items():
        cs = make()
        f, g, _ = bref.run(cs, bref.START)
        got = bref.probes(f, g, cs.s)
        print(name, got)
        assert all(bref.close(a, b) for a, b in zip(got, fix["probes"][name])), (name, got, fix["probes"][name])
        assert all(p != 0.0 for p in got[:3]) and got[5] > 0.0


def test_the_fixtures_figures_meet_the_gates(fix):
    rest, onset, cavity = fix["rest"], fix["onset"], fix["cavity"]
    # settled: the last five thousand steps stay at rounding level, nine orders below the first thousand's
    late = [rest["history"][str(n)] for n in range(16000, 20001, 1000)]
    assert rest["steps"] == bref.LAYER["steps"] and max(late) <= 1e-14 and rest["history"]["1000"] >= 1e-6
    (a0, a1), (b0, b1) = onset["amplitudes"]
    assert a1 < a0 and b1 > b0
    assert onset["rates"][0] < 0.0 < onset["rates"][1]
    assert onset["deviation"] == abs(onset["Ra_c"] / 1707.76 - 1.0) and onset["deviation"] < 0.03
    assert abs(cavity["nusselt"] / 1.118 - 1.0) == cavity["deviation"] and cavity["deviation"] < 0.05
    hist = cavity["history"]
    assert abs(hist[str(cavity["steps"])] - hist[str(cavity["steps"] - 2500)]) <= 1e-10   # a settled Nusselt number
    assert cavity["max_u"] < 0.1 / np.sqrt(3.0)


CAUGHT_BY = {"sign": "onset_1900", "no_half": "rest", "old_array": "onset_1900", "no_f0": "driven"}


@pytest.mark.parametrize("defect", bref.DEFECTS)
def test_a_seeded_defect_misses_the_fixture(fix, defect):
    name = CAUGHT_BY[defect]
    cs = bref.SHORT[name]()
    f, g, _ = bref.run(cs, bref.START, defect=defect)
    got, want = bref.probes(f, g, cs.s, defect), fix["probes"][name]
    miss = [abs(a - b) / abs(b) for a, b in zip(got, want)]
    print(defect, name, miss)
    assert not all(bref.close(a, b) for a, b in zip(got, want))
    assert max(miss) >= 1e-6                                                  # not by a hair: a thousand times the gate

"""Moving walls (include/lbm.h, "Moving walls"; lbm_dwall_*) on the GPU: every WALL instance of the four double-precision
kernel families against tests/_wall_ref.py, bit for bit.

WALL is a fourth template flag beside FORCE, TRT and OPEN of d2q9_dp_step, d2q9_dp_multi (LBMDouble at "multistep" 0 and 8),
d2q9_dp_ensemble (EnsembleDouble.run) and d2q9_dp_ensemble_gated (EnsembleDouble.run_until): 32 more separately compiled
kernels.  The cases (make_case with `wall`), the drivers, the gates and the bodies of the tests that every option repeats are
tests/_dp_matrix.py's; its open_context and open_ensemble call set_wall on a handle before anything else happens to it.

  1. the matrix: the 8 FORCE x TRT x OPEN combinations x the 4 families x 33x19 and 17x16, three members, runs of 1, 1, 1 and 7
     steps.  Per member a velocity with |component| <= 0.05 on every blocked cell, but one wall row and part of the body, which
     stay at exactly 0.0: both branches of the obstacle run beside each other.  rho_wall differs per member.  Compared: cells
     after each run, av_vels, the force record and force() before each run; ensemble members also against the contexts;
  2. a region wider than the grid: 6x5, rows 0 and 4 moving with a velocity per column and member, in d2q9_dp_multi and both
     ensemble kernels, six single steps.  A copy of a wall cell that takes another cell's velocity fails here;
  3. off is off: set_wall and then off, and a map of +-0.0, equal a handle that never heard of walls in cells, av_vels, the force
     record and force(), on both shapes in all families;
  4. identities: "multistep" 0 against 8 and context against member (in 1), one run of 10 against 3 + 7, a member stopped by
     run_until against a plain run to its count (37x29, four members, a moving lid);
  5. end to end: Couette flow, 16x16, 6000 steps through LBMDouble with "multistep" 8 and "force", to the profile bound and the
     two wall forces of tests/test_wall_restatement_cpu.py, the downloaded state equal to _wall_ref.couette_run alongside on the
     CPU."""
import numpy as np
import pytest

import _dp_matrix as dm
import _wall_ref

pytestmark = pytest.mark.gpu

SHAPES = dm.SHAPES
RUNS = dm.RUNS
FLAGS = dm.flags(3)
once = dm.Once()


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


# ---- 1. the instance matrix --------------------------------------------------------------------------------------------

def matrix_case(lbm, nx, ny, force, trt, opened, mode="on"):
    return dm.make_case(lbm, nx, ny, 3, sum(RUNS), force, trt, opened, wall=mode)


def test_the_velocities_hold_what_they_promise(lbm):
    for nx, ny in SHAPES:
        case = matrix_case(lbm, nx, ny, 1, 0, 0)
        for m in case.members:
            u_x, u_y, rho = m.wall
            blocked = m.ob != 0
            mv = _wall_ref.moving(m.ob, u_x, u_y)
            assert np.all(u_x[~blocked] == 0.0) and np.all(u_y[~blocked] == 0.0)
            assert max(np.abs(u_x).max(), np.abs(u_y).max()) <= 0.05
            assert not mv[0].any() and mv[ny - 1].all()                           # one wall row rests, the other moves
            body = m.body != 0
            assert np.count_nonzero(body & mv) >= 8 and np.count_nonzero(body & ~mv) >= 4
            assert np.count_nonzero(blocked & ~body & mv) >= nx                   # moving cells outside the body too
        assert len({m.wall[2] for m in case.members}) == 3 and len({m.wall[0].tobytes() for m in case.members}) == 3


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", dm.FAMILIES)
@pytest.mark.parametrize("force,trt,opened", FLAGS)
def test_every_wall_instance_equals_the_reference(lbm, oracle_f64, force, trt, opened, family, nx, ny):
    what = "%s<%d,%d,%d,1> %dx%d" % (family, force, trt, opened, nx, ny)
    case = matrix_case(lbm, nx, ny, force, trt, opened)
    dm.check_every_instance(once, matrix_case, lbm, oracle_f64, case, (force, trt, opened), family, nx, ny, what,
                            force_off_against_on=True)


# ---- 2. a region wider than the grid -------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["dp_multi", "ensemble", "gated"])
def test_region_wider_than_the_grid(lbm, oracle_f64, family):
    case = dm.narrow_case(lbm)
    for m in case.members:
        u_x, u_y, _ = m.wall
        assert len(set(u_x[0])) == case.nx and len(set(u_x[-1])) == case.nx and len(set(u_y[0])) == case.nx
        assert max(np.abs(u_x).max(), np.abs(u_y).max()) <= 0.1
    dm.check_region_wider_than_the_grid(once, lbm, oracle_f64, family, case)


# ---- 3. off is off -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", dm.FAMILIES)
@pytest.mark.parametrize("force,trt,opened", [(1, 0, 0), (1, 1, 1)])
def test_off_is_off(lbm, force, trt, opened, family, nx, ny):
    what = "%s<%d,%d,%d> %dx%d" % (family, force, trt, opened, nx, ny)
    # ... and that flow is not the one with the walls moving
    dm.check_off_is_off(once, matrix_case, lbm, (force, trt, opened), family, nx, ny, what, ("off", "zeros"), "matrix",
                        matrix_case(lbm, nx, ny, force, trt, opened), finite=False)


# ---- 4. identities -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", dm.FAMILIES)
def test_one_run_of_ten_against_three_and_seven(lbm, family):
    nx, ny = SHAPES[0]
    dm.check_one_run_of_ten_against_three_and_seven(once, lbm, family, lambda: matrix_case(lbm, nx, ny, 1, 1, 0))


def test_a_member_stopped_by_run_until_is_a_plain_run_to_its_count(lbm):
    nx, ny = 37, 29
    u_x, u_y = np.zeros((ny, nx)), np.zeros((ny, nx))
    u_x[ny - 1] = 0.04                                                            # the lid
    rhos = np.array([0.1, 0.0985, 0.102, 0.1])
    # the lid drives it: without the setting member 0 is another flow
    dm.check_a_member_stopped_by_run_until(lbm, None, lambda ens: ens.set_wall(u_x, u_y, rhos),
                                           lambda sim, k: sim.set_wall(u_x, u_y, rhos[k]), "moving lid %dx%d",
                                           (0, lambda sim: None))


# ---- 5. end to end: Couette flow -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("trt", [False, True])
def test_couette_flow_end_to_end(lbm, trt):
    c = _wall_ref.COUETTE
    nx, ny, steps = c["nx"], c["ny"], c["steps"]
    ob, u_x, u_y = _wall_ref.couette_maps()
    p = lbm.make_dparams(nx, ny, steps, density=c["rho"], accel=0.0, omega=c["omega"], obstacles=ob)
    top, bottom = np.zeros_like(ob), np.zeros_like(ob)
    top[ny - 1], bottom[0] = 1, 1

    def context(force):
        sim = lbm.LBMDouble(p, ob)
        sim.set_option("multistep", 8)
        sim.set_option("force", force)
        if trt:
            sim.set_trt(c["magic"])
        sim.set_wall(u_x, u_y, c["rho"])
        sim.upload(None)
        return sim

    with context(1) as sim:
        sim.set_body(top)
        sim.run(steps)
        cells = sim.download(av_vels=False)[0]
        f_top = sim.force()
        record = sim.force_record()
    with context(0) as sim:                                                       # a body map may change between runs here
        sim.run(steps)
        assert np.array_equal(sim.download(av_vels=False)[0], cells)
        sim.set_body(top)
        assert sim.force() == f_top
        sim.set_body(bottom)
        f_bottom = sim.force()
    _, want, _ = _wall_ref.couette_run(trt)
    assert np.array_equal(cells, want)                                            # _wall_ref alongside, bit for bit
    err = float(np.max(np.abs(_wall_ref.column_velocity(cells, nx // 2) - _wall_ref.couette_profile(ny, c["U"])))) / c["U"]
    shear = _wall_ref.couette_force(nx, ny, c["U"], c["rho"], c["omega"])
    rel_top, rel_bottom = abs(f_top[0] + shear) / shear, abs(f_bottom[0] - shear) / shear
    print("Couette %s on the GPU: profile within %.2e U, F_x top %+.13e (%.1e relative) bottom %+.13e (%.1e relative)" %
          ("TRT" if trt else "BGK", err, f_top[0], rel_top, f_bottom[0], rel_bottom))
    assert err <= 1e-10
    assert rel_top <= 1e-9 and rel_bottom <= 1e-9
    assert abs(record[0][-1] + shear) <= 1e-9 * shear                             # the record's last entry is the settled force too

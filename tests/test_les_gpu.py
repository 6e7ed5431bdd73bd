"""The Smagorinsky subgrid viscosity (include/lbm.h, "Subgrid viscosity"; lbm_dles_*) on the GPU: every LES instance of the four
double-precision kernel families against tests/_les_ref.py.

LES is a fifth template flag beside FORCE, TRT, OPEN and WALL of d2q9_dp_step, d2q9_dp_multi (LBMDouble at "multistep" 0 and 8),
d2q9_dp_ensemble (EnsembleDouble.run) and d2q9_dp_ensemble_gated (EnsembleDouble.run_until): 64 more separately compiled
kernels.  The cases (make_case with `wall` and `les`), the drivers, the gates and the bodies of the tests that every option
repeats are tests/_dp_matrix.py's; its open_context and open_ensemble call set_wall and then set_les on a handle before anything
else happens to it.  The Couette gate and figures are tests/_les_ref.py's.

  1. the matrix: the 16 FORCE x TRT x OPEN x WALL combinations x the 4 families x 33x19 and 17x16, three members with c = 0.1,
     0.17 and 0.3, runs of 1, 1, 1 and 7 steps.  Compared with _les_ref: cells after each run, av_vels under the bound of the
     existing matrix, the force record, force() before each run; ensemble members against the contexts, bit for bit;
  2. a region wider than the grid: 6x5 in d2q9_dp_multi and both ensemble kernels, six single steps;
  3. off is off: set_les(c) and then set_les(0.0) equals a handle that never heard of it in cells, av_vels, the force record and
     force(), on both shapes in all families; on is on: with c = 0.17 the cells differ from BGK's (this fails without the feature,
     as does every test here that calls set_les);
  4. identities, by np.array_equal: "multistep" 0, 3 and 8; one run of 10 against 3 + 7; context against member; a member stopped
     by run_until on "av_vels" and on "drag" against a plain run to its count (37x29, four members, a moving lid);
  5. errors and what keeps the setting;
  6. end to end: the Couette case of tests/test_les_restatement_cpu.py through LBMDouble ("multistep" 8, "force", one body map
     per wall row) and through two-member EnsembleDoubles, held to the same 1e-4; the cavity through LBMDouble with c = 0.17 for
     3000 steps: finite, positive densities, max |u| < U.  No GPU test runs the BGK cavity to its blow-up; that half is the CPU
     module's.  An ensemble is all BGK or all TRT (lbm_dtrt_ens_set), so the Couette ensembles are one per operator, their two
     members differing in c.

The comparisons with numpy in 1, 2 and 5 rest on the device's double-precision square root being correctly rounded; the
comparisons between device forms in 3 and 4 do not.  Bits are asked for, and bits hold: on an MI355X the cells of all 128 matrix
cases, of the 6x5 cases and of the error tests equal the restatement by np.array_equal after every run, so the largest distance
seen is 0 ulps of om, and no looser bound is in this module.  The Couette runs of 6 give the CPU module's figures to the digit
(3.6e-06 and 5.5e-06 on the force, 2.68e-06 U and 4.06e-06 U on the profile), the cavity its max |u| of 0.0811."""
import numpy as np
import pytest

import _dp_matrix as dm
import _les_ref
import _wall_ref
from _dp_matrix import CS
from _les_ref import GATE

pytestmark = pytest.mark.gpu

SHAPES = dm.SHAPES
RUNS = dm.RUNS
FLAGS = dm.flags(4)
once = dm.Once()


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


# ---- 1. the instance matrix --------------------------------------------------------------------------------------------

def matrix_case(lbm, nx, ny, force, trt, opened, wall, mode="on"):
    return dm.make_case(lbm, nx, ny, 3, sum(RUNS), force, trt, opened, wall="on" if wall else None, les=mode)


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", dm.FAMILIES)
@pytest.mark.parametrize("force,trt,opened,wall", FLAGS)
def test_every_les_instance_equals_the_reference(lbm, oracle_f64, force, trt, opened, wall, family, nx, ny):
    what = "%s<%d,%d,%d,%d,1> %dx%d" % (family, force, trt, opened, wall, nx, ny)
    case = matrix_case(lbm, nx, ny, force, trt, opened, wall)
    assert [m.les for m in case.members] == [0.1, 0.17, 0.3]
    dm.check_every_instance(once, matrix_case, lbm, oracle_f64, case, (force, trt, opened, wall), family, nx, ny, what)


# ---- 2. a region wider than the grid -------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["dp_multi", "ensemble", "gated"])
def test_region_wider_than_the_grid(lbm, oracle_f64, family):
    case = dm.narrow_case(lbm, les="on")
    assert [m.les for m in case.members] == CS[:3]
    dm.check_region_wider_than_the_grid(once, lbm, oracle_f64, family, case)


# ---- 3. off is off, on is on ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", dm.FAMILIES)
@pytest.mark.parametrize("force,trt,opened,wall", [(1, 0, 0, 0), (1, 1, 1, 1)])
def test_off_is_off_and_on_is_on(lbm, force, trt, opened, wall, family, nx, ny):
    what = "%s<%d,%d,%d,%d> %dx%d" % (family, force, trt, opened, wall, nx, ny)
    # with c = 0.17 in every member the cells differ from those of the flow without the model
    case = matrix_case(lbm, nx, ny, force, trt, opened, wall)
    for m in case.members:
        m.les_on = m.les = 0.17
    dm.check_off_is_off(once, matrix_case, lbm, (force, trt, opened, wall), family, nx, ny, what, ("off",), "on", case, finite=True)


# ---- 4. identities -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trt,wall", [(0, 0), (1, 1)])
def test_multistep_0_3_and_8_agree(lbm, trt, wall):
    nx, ny = SHAPES[0]
    dm.check_multistep_0_3_and_8_agree(once, lbm, ("forms", trt, wall), lambda: matrix_case(lbm, nx, ny, 1, trt, 0, wall))


@pytest.mark.parametrize("family", dm.FAMILIES)
def test_one_run_of_ten_against_three_and_seven(lbm, family):
    nx, ny = SHAPES[0]
    dm.check_one_run_of_ten_against_three_and_seven(once, lbm, family, lambda: matrix_case(lbm, nx, ny, 1, 1, 0, 1))


@pytest.mark.parametrize("on", ["av_vels", "drag"])
def test_a_member_stopped_by_run_until_is_a_plain_run_to_its_count(lbm, on):
    nx, ny = 37, 29
    u_x, u_y = np.zeros((ny, nx)), np.zeros((ny, nx))
    u_x[ny - 1] = 0.04                                                            # the lid
    rhos = np.array([0.1, 0.0985, 0.102, 0.1])

    def set_ensemble(ens):
        ens.set_wall(u_x, u_y, rhos)
        ens.set_les(CS)

    def set_member(sim, k):
        sim.set_wall(u_x, u_y, rhos[k])
        sim.set_les(CS[k])

    # the model changes it: with the lid alone member 3 is another flow
    dm.check_a_member_stopped_by_run_until(lbm, on, set_ensemble, set_member, "moving lid %dx%d with the model",
                                           (3, lambda sim: sim.set_wall(u_x, u_y, rhos[3])))


# ---- 5. errors and what keeps the setting --------------------------------------------------------------------------------

LBM_ERR_ARG, LBM_ERR_STATE = 1, 3


def test_errors_and_what_keeps_the_setting(lbm, oracle_f64):
    lib = lbm.load_library()
    nx, ny = 17, 16
    case = matrix_case(lbm, nx, ny, 0, 0, 0, 0, None)
    m = case.members[0]
    want = dm.reference_step(oracle_f64, m.p, m.ob, None, m.cells0, None, None, None, 0.17)[0]
    plain = dm.reference_step(oracle_f64, m.p, m.ob, None, m.cells0, None, None, None, None)[0]
    assert not np.array_equal(want, plain)
    with lbm.LBMDouble(m.p, m.ob) as sim:
        assert sim.les() == (0.0, 0.0)                                            # off by default
        sim.upload(m.cells0)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], plain)
        assert lib.lbm_dles_set(sim.ctx, 0.17) == LBM_ERR_STATE                   # after a step
        assert b"first step" in lib.lbm_last_error()
        assert sim.les() == (0.0, 0.0)
        sim.upload(m.cells0)                                                      # accepted again
        sim.set_les(0.17)
        assert sim.les() == (0.17, _les_ref.constants(m.p.omega, 0.17)[1])        # c and les_k as the host statements give them
        for bad in (-0.1, float("nan"), float("inf")):
            assert lib.lbm_dles_set(sim.ctx, bad) == LBM_ERR_ARG
            assert sim.les()[0] == 0.17
        assert lib.lbm_dles_get(sim.ctx, None, None) == LBM_ERR_ARG
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], want)
        assert lib.lbm_dles_set(sim.ctx, 0.0) == LBM_ERR_STATE
        sim.upload(m.cells0)                                                      # uploads keep the setting
        sim.upload_obstacles(m.ob)
        assert sim.les()[0] == 0.17
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], want)
        # the model and TRT in either order
        magic = 3.0 / 16.0
        both = dm.reference_step(oracle_f64, m.p, m.ob, None, m.cells0, magic, None, None, 0.17)[0]
        sim.upload(m.cells0)
        sim.set_trt(magic)                                                        # the model first, TRT second
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], both)
    with lbm.LBMDouble(m.p, m.ob) as sim:
        sim.set_trt(magic)                                                        # TRT first, the model second
        sim.set_les(0.17)
        sim.upload(m.cells0)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], both)
    # an ensemble: a refused call changes nothing, on the host or on the device
    ms = case.members
    cs = np.array([0.1, 0.17, 0.3])
    start = np.stack([q.cells0 for q in ms])
    wants = np.stack([dm.reference_step(oracle_f64, q.p, q.ob, None, q.cells0, None, None, None, float(c))[0] for q, c in zip(ms, cs)])
    with lbm.EnsembleDouble([q.p for q in ms], np.stack([q.ob for q in ms])) as ens:
        assert not np.any(ens.les()[0])
        ens.set_les(cs)
        got_c, got_k = ens.les()
        assert np.array_equal(got_c, cs)
        assert got_k.tolist() == [_les_ref.constants(q.p.omega, float(c))[1] for q, c in zip(ms, cs)]
        for member, bad in ((1, 0.0), (2, float("nan")), (0, -1.0), (2, float("inf"))):
            r = cs.copy()
            r[member] = bad
            assert lib.lbm_dles_ens_set(ens.ens, r.ctypes.data) == LBM_ERR_ARG
            assert ("member %d" % member) in lib.lbm_last_error().decode()
            assert np.array_equal(ens.les()[0], cs)
        assert lib.lbm_dles_ens_get(ens.ens, None, None) == LBM_ERR_ARG
        ens.upload(start)
        ens.run(1)
        assert np.array_equal(ens.download(av_vels=False)[0], wants)
        assert lib.lbm_dles_ens_set(ens.ens, None) == LBM_ERR_STATE
        assert lib.lbm_dles_ens_set(ens.ens, cs.ctypes.data) == LBM_ERR_STATE
        ens.upload(start)                                                         # keeps the setting
        assert np.array_equal(ens.les()[0], cs)
        ens.run(1)
        assert np.array_equal(ens.download(av_vels=False)[0], wants)
        ens.upload(start)
        ens.set_les(None)                                                         # off
        assert not np.any(ens.les()[0])
        ens.run(1)
        assert np.array_equal(ens.download(av_vels=False)[0][0], plain)
        ens.upload(start)
        ens.set_les(0.17)                                                         # one value for all
        assert np.array_equal(ens.les()[0], [0.17] * 3)


# ---- 6. end to end -------------------------------------------------------------------------------------------------------

def couette_setup(lbm):
    c = _wall_ref.COUETTE
    ob, u_x, u_y = _wall_ref.couette_maps()
    p = lbm.make_dparams(c["nx"], c["ny"], c["steps"], density=c["rho"], accel=0.0, omega=c["omega"], obstacles=ob)
    top, bottom = np.zeros_like(ob), np.zeros_like(ob)
    top[c["ny"] - 1], bottom[0] = 1, 1
    return c, ob, u_x, u_y, p, top, bottom


def couette_gates(c, cells, f_top, f_bottom, smag, what):
    want = _les_ref.couette_force(c["nx"], c["ny"], c["U"], c["rho"], c["omega"], smag)
    plain = _wall_ref.couette_force(c["nx"], c["ny"], c["U"], c["rho"], c["omega"])
    err = float(np.max(np.abs(_wall_ref.column_velocity(cells, c["nx"] // 2) - _wall_ref.couette_profile(c["ny"], c["U"])))) / c["U"]
    rel_top, rel_bottom = abs(f_top + want) / want, abs(f_bottom - want) / want
    print("Couette %s on the GPU, c = %g: profile within %.2e U, F_x top %+.13e (%.1e relative) bottom %+.13e (%.1e relative)" %
          (what, smag, err, f_top, rel_top, f_bottom, rel_bottom))
    assert err <= GATE
    assert rel_top <= GATE and rel_bottom <= GATE
    assert abs(f_top + plain) / plain > GATE                                      # the molecular formula fails the gate


@pytest.mark.parametrize("trt", [False, True])
def test_couette_flow_end_to_end(lbm, trt):
    c, ob, u_x, u_y, p, top, bottom = couette_setup(lbm)
    smag = _les_ref.COUETTE_C

    def context(force):
        sim = lbm.LBMDouble(p, ob)
        sim.set_option("multistep", 8)
        sim.set_option("force", force)
        if trt:
            sim.set_trt(c["magic"])
        sim.set_wall(u_x, u_y, c["rho"])
        sim.set_les(smag)
        sim.upload(None)
        return sim

    with context(1) as sim:
        sim.set_body(top)
        sim.run(c["steps"])
        cells = sim.download(av_vels=False)[0]
        f_top = sim.force()
        record = sim.force_record()
    with context(0) as sim:                                                       # a body map may change between runs here
        sim.run(c["steps"])
        assert np.array_equal(sim.download(av_vels=False)[0], cells)
        sim.set_body(top)
        assert sim.force() == f_top
        sim.set_body(bottom)
        f_bottom = sim.force()
    couette_gates(c, cells, f_top[0], f_bottom[0], smag, "TRT" if trt else "BGK")
    want = _les_ref.couette_force(c["nx"], c["ny"], c["U"], c["rho"], c["omega"], smag)
    assert abs(record[0][-1] + want) <= GATE * want                               # the record's last entry is the settled force too


@pytest.mark.parametrize("trt", [False, True])
def test_couette_flow_in_a_two_member_ensemble(lbm, trt):
    c, ob, u_x, u_y, p, top, bottom = couette_setup(lbm)
    smags = [_les_ref.COUETTE_C, 1.0]
    forces = {}
    for name, body in (("top", top), ("bottom", bottom)):
        with lbm.EnsembleDouble([p, p], ob) as ens:
            ens.set_option("force", 1)
            if trt:
                ens.set_trt(c["magic"])
            ens.set_wall(u_x, u_y, c["rho"])
            ens.set_les(smags)
            ens.set_body(body)
            ens.upload(None)
            ens.run(c["steps"])
            cells = ens.download(av_vels=False)[0]
            forces[name] = ens.force()[0]
    for k, smag in enumerate(smags):
        couette_gates(c, cells[k], float(forces["top"][k]), float(forces["bottom"][k]), smag, "member %d %s" % (k, "TRT" if trt else "BGK"))
    assert not np.array_equal(cells[0], cells[1])


def test_the_cavity_stays_finite_with_the_model(lbm):
    v = _les_ref.CAVITY
    ob, u_x, u_y = _les_ref.cavity_maps()
    p = lbm.make_dparams(v["nx"], v["ny"], v["steps"], density=v["rho"], accel=0.0, omega=v["omega"], obstacles=ob)
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_wall(u_x, u_y, v["rho"])
        sim.set_les(v["c"])
        sim.upload(None)
        sim.run(v["steps"])
        cells, av = sim.download()
    assert np.all(np.isfinite(cells)) and np.all(np.isfinite(av))
    umax, rho_min = _les_ref.velocity_magnitude(cells, ob)
    print("cavity on the GPU, c = %g: finite after %d steps, max |u| %.4f, min density %.4f" % (v["c"], v["steps"], umax, rho_min))
    assert rho_min > 0.0 and np.all(cells[:, ob == 0] > 0.0)
    assert 0.0 < umax < v["U"]

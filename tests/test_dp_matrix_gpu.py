"""Every FORCE x TRT x OPEN instance of the four double-precision kernel families against numpy.

FORCE (option "force"), TRT (set_trt) and OPEN (set_open) are template flags of d2q9_dp_step, d2q9_dp_multi (LBMDouble at
"multistep" 0 and 8), d2q9_dp_ensemble (EnsembleDouble.run) and d2q9_dp_ensemble_gated (EnsembleDouble.run_until): 32
separately compiled kernels, chosen by launch_step / launch_multi (lbm_dp.cpp) and launch_dens (lbm_dens.cpp).  The reference
is tests/_dp_matrix.reference_step, which only routes a state to tests/_open_ref.py, tests/_trt_ref.py (through the steps of the
options that are off here) and tests/_force_ref.py's restatement and body_restatement; tests/test_dp_matrix_cpu.py holds the
inputs to what these comparisons need of them.  The cases, the drivers, the gates and the cache (dm.Once) are tests/_dp_matrix.py's.

Gates, all taken from the suite as it stands:
  cells after every run            np.array_equal with the reference applied that many times
  av_vels per step                 within N 2^-53 sum|u| of the reference's sum|u| * free_cells_inv (N = nx ny cells; the bound
                                   between two summation orders of N terms)
  force record per step            within 8 L 2^-53 sum|link terms| of the reference's force (L links; test_force_gpu's gate)
  force() before a run             equals the record entry the run's first step writes
  FORCE off against FORCE on, members against LBMDouble contexts, stop counts: no tolerance

  1. the matrix: the 8 flag combinations x the 4 families x 33x19 (nx odd, ragged tiles, column nx - 1 alone in the third tile
     column) and 17x16 (column nx - 1 alone in a second tile column, one tile row: the region's rows wrap in y and the staged
     profile holds grid rows more than once).  Three members with their own omega, Lambda, inlet profile, rho_out, state and
     matrix_mask(nx, ny, member); runs of 1, 1, 1 and 7 steps (d2q9_dp_multi: one launch of depth 7; the ensembles: 3 + 3 + 1);
  2. bodies at the open columns: OPEN and FORCE on in the 4 families on 33x19, 17x16 and 48x35, twelve single steps, once with
     every blocked cell counted (the walls touch both columns) and once with the members' bodies (the lips in columns 1 and
     nx - 2); member 1 has a body cell beside the blocked cell of column 0.  Ensemble members also against LBMDouble contexts;
  3. 5x4 without walls in the two ensemble kernels: the region of every tile is wider than the grid; the force is exactly +0.0;
  4. a steady run per criterion on 48x32 with four members on their own maps and bodies, OPEN, TRT and FORCE on.

Which test launches which instance (<FORCE,TRT,OPEN>; "matrix" is test_every_instance_equals_the_reference of this module,
named where it is the first test to launch the instance, and it launches every one of the 32):

  instance  d2q9_dp_step                d2q9_dp_multi               d2q9_dp_ensemble              d2q9_dp_ensemble_gated
  <0,0,0>   test_dp_gpu                 test_dp_gpu                 test_dp_ensemble_gpu          test_dp_steady_gpu
  <1,0,0>   test_force_gpu              test_force_gpu              test_force_gpu (members)      test_force_gpu, test_body_gpu (steady)
  <0,1,0>   test_trt_gpu (single steps) test_trt_gpu (single steps) test_trt_gpu (errors, 2 steps) matrix  [none before]
  <1,1,0>   test_trt_gpu (forms)        test_trt_gpu (forms)        test_trt_gpu (members)        test_trt_gpu (steady, both criteria)
  <0,0,1>   matrix  [none before]       test_open_gpu (channel)     test_open_gpu (errors, 2 steps) matrix  [none before]
  <0,1,1>   matrix  [none before]       test_open_gpu (channel)     matrix  [none before]         matrix  [none before]
  <1,0,1>   test_open_gpu (single)      test_open_gpu (single)      test_open_gpu (members 48x35) matrix  [none before]
  <1,1,1>   test_open_gpu (single)      test_open_gpu (single)      test_open_gpu (members 33x19) test_open_gpu (steady)

Seven instances had no launch before this module.  Two that were suspected of none had one: d2q9_dp_ensemble<0,1,0> runs two
steps in test_trt_gpu.test_errors_and_what_keeps_the_setting, and d2q9_dp_ensemble_gated<1,1,0> runs under both criteria in
test_trt_gpu.test_run_until_stops_every_member_where_the_rule_says."""
import numpy as np
import pytest

import _dp_matrix as dm
import _open_ref
from _dp_matrix import assert_equals_the_reference, assert_same_bits, plus_zero
from _steady_rule import CAP, OMEGAS, TOL, rule

pytestmark = pytest.mark.gpu

U = dm.U
SHAPES = dm.SHAPES
BODY_SHAPES = SHAPES + [(48, 35)]
RUNS = dm.RUNS
FLAGS = dm.flags(3)
once = dm.Once()
reference_of, run_of, _runs = once.reference_of, once.run_of, once.runs


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


# ---- 1. the instance matrix --------------------------------------------------------------------------------------------

def matrix_case(lbm, nx, ny, force, trt, opened):
    return dm.make_case(lbm, nx, ny, 3, sum(RUNS), force, trt, opened)


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", dm.FAMILIES)
@pytest.mark.parametrize("force,trt,opened", FLAGS)
def test_every_instance_equals_the_reference(lbm, oracle_f64, force, trt, opened, family, nx, ny):
    what = "%s<%d,%d,%d> %dx%d" % (family, force, trt, opened, nx, ny)
    case = matrix_case(lbm, nx, ny, force, trt, opened)
    refs = reference_of(oracle_f64, ("matrix", nx, ny, trt, opened), case, sum(RUNS))
    got = run_of(lbm, ("matrix", nx, ny, force, trt, opened), family, case, RUNS)
    assert_equals_the_reference(case, refs, got, RUNS, what)
    assert len({r.states[-1].tobytes() for r in got}) == case.n            # the members are different flows
    if not force:
        # the option computes the same flow, and force() needs no option
        on = run_of(lbm, ("matrix", nx, ny, 1, trt, opened), family, matrix_case(lbm, nx, ny, 1, trt, opened), RUNS)
        assert_same_bits(got, on, what)


# ---- 2. bodies at the open columns -------------------------------------------------------------------------------------

SINGLE = [1] * 12


def body_case(lbm, nx, ny, counted):
    """BGK and TRT alternate over the six cases: every shape and both ways of counting see both"""
    trt = (BODY_SHAPES.index((nx, ny)) + (counted == "body")) % 2 == 1
    return dm.make_case(lbm, nx, ny, 3, len(SINGLE), True, trt, True, counted=counted, beside=1)


@pytest.mark.parametrize("counted", ["all", "body"])
@pytest.mark.parametrize("nx,ny", BODY_SHAPES)
@pytest.mark.parametrize("family", dm.FAMILIES)
def test_bodies_at_the_open_columns(lbm, oracle_f64, family, nx, ny, counted):
    what = "%s %dx%d %s counted" % (family, nx, ny, counted)
    case = body_case(lbm, nx, ny, counted)
    key = ("body", nx, ny, counted)
    refs = reference_of(oracle_f64, key, case, len(SINGLE))
    got = run_of(lbm, key, family, case, SINGLE)
    assert_equals_the_reference(case, refs, got, SINGLE, what)
    # the gate sees the links into the two columns, on every state of the run: without them the force is far outside it
    for k, (m, ref) in enumerate(zip(case.members, refs)):
        for t in range(len(SINGLE)):
            west, east, dx, dy = dm.column_links(ref.states[t], m.ob, m.body)
            rx, ry, links, mag = ref.forces[t]
            assert west >= 8 and east >= 8 and max(abs(dx), abs(dy)) > 1000.0 * (8.0 * links * U * mag), (what, k, t)
    if family in ("ensemble", "gated"):
        # a member is the LBMDouble on its map and body, bit for bit, record and force() included
        assert_same_bits(got, run_of(lbm, key, "dp_step", case, SINGLE), what)
        assert_same_bits(got, run_of(lbm, key, "dp_multi", case, SINGLE), what)
    assert not np.array_equal(got[0].fx, got[1].fx) and not np.array_equal(got[1].fx, got[2].fx)


# ---- 3. the wrapped region in ensembles --------------------------------------------------------------------------------

@pytest.mark.parametrize("trt", [False, True])
@pytest.mark.parametrize("family", ["ensemble", "gated"])
def test_region_wider_than_the_grid(lbm, oracle_f64, family, trt):
    nx, ny, runs = 5, 4, [1] * 6
    case = dm.make_case(lbm, nx, ny, 3, len(runs), True, trt, True)
    assert all(not np.any(m.ob) and m.body is None for m in case.members)
    assert len({m.open[0].tobytes() for m in case.members}) == 3 and all(np.all(m.open[0] > 0.0) for m in case.members)
    key = ("wrapped", trt)
    refs = reference_of(oracle_f64, key, case, len(runs))
    got = run_of(lbm, key, family, case, runs)
    assert_equals_the_reference(case, refs, got, runs, "%s 5x4 %s" % (family, "TRT" if trt else "BGK"))
    for r in got:
        assert r.fx.shape == (len(runs),) and plus_zero(r.fx) and plus_zero(r.fy) and plus_zero(r.now)       # exactly +0.0
    assert len({r.states[-1].tobytes() for r in got}) == 3


# ---- 4. a steady run on per-member maps ----------------------------------------------------------------------------------

STEADY_AMPLITUDES = [0.02 * (1.0 + 0.5 * m) for m in range(4)]     # test_open_gpu.steady_profiles


def steady_case(lbm):
    nx, ny = 48, 32
    profiles = [_open_ref.poiseuille(ny, a) for a in STEADY_AMPLITUDES]
    return dm.make_case(lbm, nx, ny, 4, CAP, True, True, True, omegas=OMEGAS[4], profiles=profiles, rhos=[0.1] * 4, rest=True)


def steady_record(lbm):
    """av_vels and F_x of a plain run to the cap, computed once"""
    if "steady" not in _runs:
        with dm.open_ensemble(lbm, steady_case(lbm)) as ens:
            ens.run(CAP)
            _runs["steady"] = {"av": ens.download(cells=False)[1], "fx": ens.force_record()[0]}
    return _runs["steady"]


@pytest.mark.parametrize("on", ["av_vels", "drag"])
def test_run_until_on_per_member_maps_stops_every_member_where_the_rule_says(lbm, on):
    window = 7
    case = steady_case(lbm)
    assert len({m.ob.tobytes() for m in case.members}) == 4 and len({m.body.tobytes() for m in case.members}) == 4
    whole = steady_record(lbm)
    assert whole["av"].shape == (4, CAP) and np.all(np.isfinite(whole["av"])) and np.all(np.isfinite(whole["fx"]))
    # the stop decisions, on the host from the downloaded record
    want_steps, want_conv = rule(whole["av" if on == "av_vels" else "fx"], 0, CAP, window, TOL)
    print("per-member maps 48x32 window %d on %s: stops %s converged %s" % (window, on, want_steps.tolist(), want_conv.tolist()))
    assert np.any(want_conv) and len(set(want_steps.tolist())) >= 2
    with dm.open_ensemble(lbm, case) as ens:
        steps, conv = ens.run_until(CAP, window=window, rel_tol=TOL, on=on)
        assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
        cells, av = ens.download()
        fx, fy = ens.force_record()
        fields, re, now = ens.final_state(), ens.reynolds(), ens.force()
    for k, m in enumerate(case.members):
        c = int(steps[k])
        with dm.open_context(lbm, case, m, -1) as sim:
            sim.run(c)
            rc, rav = sim.download()
            rfx, rfy = sim.force_record()
            assert np.array_equal(cells[k], rc), k
            assert np.array_equal(av[k, :c], rav) and np.array_equal(av[k, :c], whole["av"][k, :c]), k
            assert np.array_equal(fx[k, :c], rfx) and np.array_equal(fy[k, :c], rfy), k
            assert np.array_equal(fx[k, :c], whole["fx"][k, :c]), k
            assert plus_zero(fx[k, c:]) and plus_zero(fy[k, c:]), k
            assert all(np.array_equal(a[k], b) for a, b in zip(fields, sim.final_state())), k
            assert re[k] == sim.reynolds() and (now[0][k], now[1][k]) == sim.force(), k

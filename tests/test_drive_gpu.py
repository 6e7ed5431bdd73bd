"""The body force (include/lbm.h, "Body force"; lbm_ddrive_*) on the GPU: every DRIVE instance of the four double-precision kernel
families against tests/_drive_ref.py, and the three force-driven flows with exact answers end to end.

DRIVE is a sixth template flag beside FORCE, TRT, OPEN, WALL and LES of d2q9_dp_step, d2q9_dp_multi (LBMDouble at "multistep" 0
and 8), d2q9_dp_ensemble (EnsembleDouble.run) and d2q9_dp_ensemble_gated (EnsembleDouble.run_until): 128 more separately
compiled kernels.  The cases (make_case with `wall`, `les` and `drive`), the drivers, the gates and the bodies of the tests that
every option repeats are tests/_dp_matrix.py's; its open_context and open_ensemble call set_wall, set_les and then set_drive on a
handle before anything else happens to it.  The fixture and the gates of the three flows are tests/_drive_ref.py's.

  1. the matrix: the 32 FORCE x TRT x OPEN x WALL x LES combinations x the 4 families x 33x19 and 17x16, three members each with
     its own force (both components non-zero, mixed signs, 1e-6 to 1e-4), runs of 1, 1, 1 and 7 steps.  Compared with _drive_ref:
     cells after each run by np.array_equal, av_vels under the bound of the existing matrix, the force record, force() before
     each run; ensemble members against the contexts, bit for bit;
  2. a region wider than the grid: 6x5 in d2q9_dp_multi and both ensemble kernels, six single steps;
  3. off is off: set_drive(f) and then set_drive((0, 0)) (None for an ensemble) equals a handle that never heard of it, on both
     shapes in all families; on is on: with F = (1e-5, 0) the cells differ from the plain run's after one step (this fails
     without the feature, as does every test here that calls set_drive);
  4. identities, by np.array_equal: "multistep" 0, 3 and 8; one run of 10 against 3 + 7; context against member; a member stopped
     by run_until on "av_vels" and on "drag" against a plain run to its count (37x29, four members, four forces);
  5. the reported velocity: the fields of final_state equal _drive_ref.fields bit for bit, and av_vels of a step is the mean |u|
     of the state behind it under the matrix's bound; errors and what keeps the setting;
  6. the three flows of tests/test_drive_restatement_cpu.py end to end under _drive_ref's gates, the figures held to the fixture's
     to 1e-9 relative, the cells after the first 200 steps to 200 restated steps;
  7. a sweep to steady state: eight members, F_x = 1e-7 .. 8e-7, run_until on "av_vels": every member converges and av_vels / F_x
     is one constant.

The comparisons with numpy rest on the device's double-precision division and square root being correctly rounded.  Bits are
asked for, and bits hold: on an MI355X the cells of all 256 matrix cases, of the 6x5 cases and of the error tests equal the
restatement by np.array_equal after every run, and no looser bound is in this module.  The flows of 6 give the fixture's figures
to the digit (deviation 1.462e-12 / 7.082e-13 / 8.729e-13 at Lambda 3/16, 4.115e-03 at 1/4, max |u| 3.93e-16 in the box, sum F_x
5.92e-04 to 1.1e-14), the sweep stops every member at 512 steps with a spread of 4.68e-08.  295 cases, 5.4 s."""
import numpy as np
import pytest

import _dp_matrix as dm
import _drive_ref as ref
from _dp_matrix import FORCES

pytestmark = pytest.mark.gpu

U = dm.U
SHAPES = dm.SHAPES
RUNS = dm.RUNS
FLAGS = dm.flags(5)
once = dm.Once()


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


@pytest.fixture(scope="module")
def fix():
    return ref.fixture()


# ---- 1. the instance matrix --------------------------------------------------------------------------------------------

def matrix_case(lbm, nx, ny, force, trt, opened, wall, les, mode="on"):
    return dm.make_case(lbm, nx, ny, 3, sum(RUNS), force, trt, opened, wall="on" if wall else None, les="on" if les else None,
                        drive=mode)


def test_the_forces_hold_what_they_promise():
    for f in FORCES:
        assert all(1e-6 <= abs(c) <= 1e-4 for c in f)
    assert len({tuple(np.sign(f)) for f in FORCES}) == 4 and len(set(FORCES)) == 4


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", dm.FAMILIES)
@pytest.mark.parametrize("force,trt,opened,wall,les", FLAGS)
def test_every_drive_instance_equals_the_reference(lbm, oracle_f64, force, trt, opened, wall, les, family, nx, ny):
    what = "%s<%d,%d,%d,%d,%d,1> %dx%d" % (family, force, trt, opened, wall, les, nx, ny)
    case = matrix_case(lbm, nx, ny, force, trt, opened, wall, les)
    assert [m.drive for m in case.members] == FORCES[:3]
    # the force changes the flow in the fluid cells alone
    dm.check_every_instance(once, matrix_case, lbm, oracle_f64, case, (force, trt, opened, wall, les), family, nx, ny, what,
                            fluid_alone=True)


# ---- 2. a region wider than the grid -------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["dp_multi", "ensemble", "gated"])
def test_region_wider_than_the_grid(lbm, oracle_f64, family):
    case = dm.narrow_case(lbm, drive="on")
    assert [m.les for m in case.members] == [None] * 3 and [m.drive for m in case.members] == FORCES[:3]
    dm.check_region_wider_than_the_grid(once, lbm, oracle_f64, family, case)


# ---- 3. off is off, on is on ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", dm.FAMILIES)
@pytest.mark.parametrize("force,trt,opened,wall,les", [(1, 0, 0, 0, 0), (1, 1, 1, 1, 1)])
def test_off_is_off_and_on_is_on(lbm, force, trt, opened, wall, les, family, nx, ny):
    what = "%s<%d,%d,%d,%d,%d> %dx%d" % (family, force, trt, opened, wall, les, nx, ny)
    flags = (force, trt, opened, wall, les)
    # with F = (1e-5, 0) in every member the cells differ from the plain run's after one step
    case = matrix_case(lbm, nx, ny, *flags)
    for m in case.members:
        m.drive_on = m.drive = (1e-5, 0.0)
    dm.check_off_is_off(once, matrix_case, lbm, flags, family, nx, ny, what, ("off",), "on", case, finite=True)


# ---- 4. identities -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trt,wall,les", [(0, 0, 0), (1, 1, 1)])
def test_multistep_0_3_and_8_agree(lbm, trt, wall, les):
    nx, ny = SHAPES[0]
    dm.check_multistep_0_3_and_8_agree(once, lbm, ("forms", trt, wall, les), lambda: matrix_case(lbm, nx, ny, 1, trt, 0, wall, les))


@pytest.mark.parametrize("family", dm.FAMILIES)
def test_one_run_of_ten_against_three_and_seven(lbm, family):
    nx, ny = SHAPES[0]
    dm.check_one_run_of_ten_against_three_and_seven(once, lbm, family, lambda: matrix_case(lbm, nx, ny, 1, 1, 0, 1, 0))


@pytest.mark.parametrize("on", ["av_vels", "drag"])
def test_a_member_stopped_by_run_until_is_a_plain_run_to_its_count(lbm, on):
    forces = np.array([(3e-5, 1e-6), (-1e-5, 2e-6), (6e-5, -4e-6), (2e-5, 8e-6)])
    # the force changes it: with another force member 3 is another flow
    dm.check_a_member_stopped_by_run_until(lbm, on, lambda ens: ens.set_drive(forces), lambda sim, k: sim.set_drive(forces[k]),
                                           "channel %dx%d with four forces", (3, lambda sim: sim.set_drive(forces[0])),
                                           final_state=True)


# ---- 5. the reported velocity; errors and what keeps the setting -----------------------------------------------------------

@pytest.mark.parametrize("trt", [0, 1])
def test_reported_velocity_is_the_physical_one(lbm, oracle_f64, trt):
    nx, ny = 33, 19
    case = matrix_case(lbm, nx, ny, 0, trt, 0, 0, 0)
    refs = once.reference_of(oracle_f64, ("matrix", nx, ny, trt, 0, 0, 0), case, sum(RUNS))
    ms = case.members
    with dm.open_ensemble(lbm, case) as ens:
        for t in range(3):
            ens.run(1)
            got = ens.final_state()
            av = ens.download(cells=False)[1]
            re = ens.reynolds()
            for k, m in enumerate(ms):
                want = ref.fields(refs[k].states[t + 1], m.ob, m.p.density, m.drive)
                for a, b, name in zip(got, want, ("u_x", "u_y", "u", "pressure")):
                    assert np.array_equal(a[k], b), (name, k, t, int(np.count_nonzero(a[k] != b)))
                # without the half force the field is another one
                assert not np.array_equal(got[0][k], ref.fields(refs[k].states[t + 1], m.ob, m.p.density, None)[0])
                # av_vels of the step is the mean |u| of the state behind it
                total = float(np.sum(want[2]))
                assert abs(av[k, t] - total * m.p.free_cells_inv) <= nx * ny * U * total, (k, t)
                viscosity = 1.0 / 6.0 * (2.0 / m.p.omega - 1.0)
                assert abs(re[k] - total * m.p.free_cells_inv * m.p.reynolds_dim / viscosity) <= nx * ny * U * abs(re[k])
    # a context reports what the member reports
    m = ms[1]
    with dm.open_context(lbm, case, m, 8) as sim:
        sim.run(3)
        assert all(np.array_equal(a, b[1]) for a, b in zip(sim.final_state(), got))
        assert sim.reynolds() == re[1]


LBM_ERR_ARG, LBM_ERR_STATE = 1, 3


def test_errors_and_what_keeps_the_setting(lbm, oracle_f64):
    lib = lbm.load_library()
    nx, ny = 17, 16
    case = matrix_case(lbm, nx, ny, 0, 0, 0, 0, 0, None)
    m = case.members[0]
    F = (4e-5, -1e-5)

    def one(magic=None, c=None, drive=F, q=m):
        return dm.reference_step(oracle_f64, q.p, q.ob, None, q.cells0, magic, None, None, c, drive)[0]

    want, plain = one(), one(drive=None)
    assert not np.array_equal(want, plain)
    with lbm.LBMDouble(m.p, m.ob) as sim:
        assert sim.drive() == (0.0, 0.0)                                          # off by default
        sim.upload(m.cells0)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], plain)
        assert lib.lbm_ddrive_set(sim.ctx, *F) == LBM_ERR_STATE                   # after a step
        assert b"first step" in lib.lbm_last_error()
        assert sim.drive() == (0.0, 0.0)
        sim.upload(m.cells0)                                                      # accepted again
        sim.set_drive(F)
        assert sim.drive() == F
        for bad in ((float("nan"), 0.0), (1e-5, float("inf")), (-float("inf"), 1e-5)):
            assert lib.lbm_ddrive_set(sim.ctx, *bad) == LBM_ERR_ARG
            assert sim.drive() == F
        assert lib.lbm_ddrive_get(sim.ctx, None, None) == LBM_ERR_ARG
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], want)
        assert lib.lbm_ddrive_set(sim.ctx, 0.0, 0.0) == LBM_ERR_STATE
        sim.upload(m.cells0)                                                      # uploads keep the setting
        sim.upload_obstacles(m.ob)
        assert sim.drive() == F
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], want)
        # the force, TRT and the subgrid model in any order
        magic = 3.0 / 16.0
        all_three = one(magic, 0.17)
        sim.upload(m.cells0)
        sim.set_trt(magic)                                                        # the force first, then TRT, then the model
        sim.set_les(0.17)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], all_three)
    with lbm.LBMDouble(m.p, m.ob) as sim:
        sim.set_les(0.17)                                                         # the model first, then the force, then TRT
        sim.set_drive(F)
        sim.set_trt(magic)
        sim.upload(m.cells0)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], all_three)
        sim.upload(m.cells0)
        sim.set_drive((0.0, 0.0))                                                 # and off again: TRT with the model alone
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], one(magic, 0.17, None))
    # an ensemble: a refused call changes nothing, on the host or on the device
    ms = case.members
    fs = np.array(FORCES[:3])
    start = np.stack([q.cells0 for q in ms])
    wants = np.stack([one(drive=tuple(f), q=q) for q, f in zip(ms, fs)])
    with lbm.EnsembleDouble([q.p for q in ms], np.stack([q.ob for q in ms])) as ens:
        assert not np.any(ens.drive())
        ens.set_drive(fs)
        assert np.array_equal(ens.drive(), fs)
        for member, bad in ((1, (0.0, 0.0)), (2, (float("nan"), 1e-5)), (0, (1e-5, float("inf"))), (2, (-0.0, 0.0))):
            r = fs.copy()
            r[member] = bad
            assert lib.lbm_ddrive_ens_set(ens.ens, r.ctypes.data) == LBM_ERR_ARG
            assert ("member %d" % member) in lib.lbm_last_error().decode()
            assert np.array_equal(ens.drive(), fs)
        assert lib.lbm_ddrive_ens_get(ens.ens, None, None) == LBM_ERR_ARG
        ens.upload(start)
        ens.run(1)
        assert np.array_equal(ens.download(av_vels=False)[0], wants)
        assert lib.lbm_ddrive_ens_set(ens.ens, None) == LBM_ERR_STATE
        assert lib.lbm_ddrive_ens_set(ens.ens, fs.ctypes.data) == LBM_ERR_STATE
        ens.upload(start)                                                         # keeps the setting
        ens.run(1)
        assert np.array_equal(ens.download(av_vels=False)[0], wants)
        ens.upload(start)
        ens.set_drive((4e-5, -1e-5))                                              # one pair for every member
        assert np.array_equal(ens.drive(), np.broadcast_to(F, (3, 2)))
        ens.set_drive(None)                                                       # off: the plain flow
        assert not np.any(ens.drive())
        ens.run(1)
        assert np.array_equal(ens.download(av_vels=False)[0], np.stack([one(drive=None, q=q) for q in ms]))


# ---- 6. the three flows, end to end ----------------------------------------------------------------------------------------

def params_of(lbm, ob, omegas, steps):
    base = lbm.make_dparams(ob.shape[1], ob.shape[0], steps, density=ref.DENSITY, accel=0.0, omega=omegas[0], obstacles=ob)
    return lbm.sweep_dparams(base, omega=list(omegas))


def held(got, want):
    """a figure against the fixture's: 1e-9 relative"""
    return abs(got - want) <= 1e-9 * abs(want)


def restated(ob, omega, magic, drive):
    key = ("start", ob.tobytes(), omega, magic, drive)
    if key not in once.refs:
        once.refs[key] = ref.run(ob, omega, magic, drive, ref.START)
    return once.refs[key]


def context_run(lbm, ob, omega, magic, drive, steps, multistep, force=False):
    """(cells after START steps, cells, fields, force record) of one LBMDouble from rest"""
    with lbm.LBMDouble(params_of(lbm, ob, [omega], steps)[0], ob) as sim:
        sim.set_option("multistep", multistep)
        sim.set_option("force", int(force))
        if magic:
            sim.set_trt(magic)
        sim.set_drive(drive)
        sim.upload(None)
        sim.run(ref.START)
        early = sim.download(av_vels=False)[0]
        sim.run(steps - ref.START)
        return early, sim.download(av_vels=False)[0], sim.final_state(), sim.force_record() if force else None


def ensemble_run(lbm, ob, omegas, magic, drives, steps, force=False):
    """the same of every member of one EnsembleDouble: [n, ...] arrays"""
    with lbm.EnsembleDouble(params_of(lbm, ob, omegas, steps), ob) as ens:
        ens.set_option("force", int(force))
        if magic:
            ens.set_trt([magic] * len(omegas))
        ens.set_drive(drives)
        ens.upload(None)
        ens.run(ref.START)
        early = ens.download(av_vels=False)[0]
        ens.run(steps - ref.START)
        return early, ens.download(av_vels=False)[0], ens.final_state(), ens.force_record() if force else None


@pytest.mark.parametrize("magic", [ref.L316, ref.L14])
def test_poiseuille_flow_one_ensemble_per_magic_parameter(lbm, fix, magic):
    p = ref.POISEUILLE
    ob, drive, omegas = ref.channel_mask(p["nx"], p["ny"]), p["force"], p["omegas"]
    early, _, fields, _ = ensemble_run(lbm, ob, omegas, magic, drive, p["steps"])
    stored = ref.poiseuille_table(fix)
    fig = {}
    for k, w in enumerate(omegas):
        assert np.array_equal(early[k], restated(ob, w, magic, drive)), w
        fig[(magic, w)] = ref.poiseuille_figures(fields[0][k], fields[1][k], fields[3][k], w)
    print("\n".join(ref.poiseuille_gates(fig, stored)))
    for key in fig:
        assert all(held(a, b) for a, b in zip(fig[key], stored[key])), (key, fig[key], stored[key])


@pytest.mark.parametrize("omega,multistep", [(0.6, 0), (1.7, 8), (1.0, 3)])
def test_poiseuille_flow_with_bgk_moves_the_wall(lbm, fix, omega, multistep):
    p = ref.POISEUILLE
    ob, drive = ref.channel_mask(p["nx"], p["ny"]), p["force"]
    early, _, fields, _ = context_run(lbm, ob, omega, None, drive, p["steps"], multistep)
    assert np.array_equal(early, restated(ob, omega, None, drive))
    stored = ref.poiseuille_table(fix)
    fig = {(None, omega): ref.poiseuille_figures(fields[0], fields[1], fields[3], omega)}
    print("\n".join(ref.poiseuille_gates(fig, stored)))
    assert fig[(None, omega)][0] >= 4e-3                                          # not the parabola
    assert all(held(a, b) for a, b in zip(fig[(None, omega)], stored[(None, omega)]))


def test_hydrostatic_balance(lbm, fix):
    h = ref.HYDROSTATIC
    ob, drive = ref.box_mask(h["nx"], h["ny"]), h["force"]
    stored = ref.case_table(fix, "hydrostatic", ("umax", "step_error"))
    (w0, m0), (w1, m1) = h["cases"]
    # TRT 3/16 through LBMDouble at "multistep" 8 and as a member; BGK through LBMDouble
    runs = {"context TRT": (context_run(lbm, ob, w0, m0, drive, h["steps"], 8), w0, m0),
            "context BGK": (context_run(lbm, ob, w1, m1, drive, h["steps"], 8), w1, m1)}
    e, c, f, _ = ensemble_run(lbm, ob, [w0, w0], m0, [drive, (0.0, 2.0 * drive[1])], h["steps"])
    runs["member TRT"] = ((e[0], c[0], tuple(a[0] for a in f), None), w0, m0)
    for name, ((early, _, fields, _), w, magic) in runs.items():
        assert np.array_equal(early, restated(ob, w, magic, drive)), name
        umax, err = ref.hydrostatic_figures(fields[2], fields[3])
        print(name, ref.hydrostatic_gates(umax, err, stored[(magic, w)][0]))
        assert held(umax, stored[(magic, w)][0]) and held(err, stored[(magic, w)][1]), (name, umax, err, stored[(magic, w)])
    assert np.array_equal(runs["member TRT"][0][1], runs["context TRT"][0][1])
    # the second member carries twice the weight: twice the density step, at rest as well
    umax, err = ref.hydrostatic_figures(f[2][1], f[3][1], 2.0 * drive[1])
    assert umax <= 1e-12 and err <= 1e-9


def test_momentum_balance(lbm, fix):
    b = ref.BALANCE
    ob, drive = ref.balance_mask(), b["force"]
    stored = ref.case_table(fix, "balance", ("rel", "lift", "fx"))
    bal = fix["balance"]
    for w, magic in b["cases"]:
        early, _, _, (fx, fy) = context_run(lbm, ob, w, magic, drive, b["steps"], -1, force=True)   # "force" on, no body map
        assert np.array_equal(early, restated(ob, w, magic, drive))
        rel, lift = ref.balance_figures(fx[-1], fy[-1])
        print("omega %.1f %s: sum F_x %.16e" % (w, "BGK" if magic is None else "TRT", fx[-1]), ref.balance_gates(rel, lift, stored[(magic, w)][0]))
        assert held(fx[-1], stored[(magic, w)][2])
    # two members, the second with the mirrored force
    w, magic = b["cases"][0]
    early, _, _, (fx, fy) = ensemble_run(lbm, ob, [w, w], magic, [drive, (-drive[0], 0.0)], b["steps"], force=True)
    assert np.array_equal(early[0], restated(ob, w, magic, drive))
    for k in range(2):
        rel, lift = ref.balance_figures(fx[k, -1], fy[k, -1], (1 - 2 * k) * drive[0])
        print("member %d" % k, ref.balance_gates(rel, lift, stored[(magic, w)][0]))
    print(ref.mirror_gate(fx[0, -1], fx[1, -1], max(bal["mirror_sum"], stored[(magic, w)][0])))
    assert held(fx[0, -1], stored[(magic, w)][2]) and held(fx[1, -1], bal["mirrored"]["fx"])


# ---- 7. a sweep to steady state ------------------------------------------------------------------------------------------

def test_sweep_to_steady_state(lbm, fix):
    s = ref.SWEEP
    ob = ref.balance_mask()
    n = len(s["forces"])
    with lbm.EnsembleDouble(params_of(lbm, ob, [s["omega"]] * n, s["max_steps"]), ob) as ens:
        ens.set_trt([s["magic"]] * n)
        ens.set_drive([(f, 0.0) for f in s["forces"]])
        ens.upload(None)
        steps, conv = ens.run_until(s["max_steps"], window=s["window"], rel_tol=s["rel_tol"], on="av_vels")
        av = ens.download(cells=False)[1]
    print("sweep: stops %s" % steps.tolist())
    assert conv.all() and np.all(steps < s["max_steps"])                          # every member converges
    last = [av[k, steps[k] - 1] for k in range(n)]
    print(ref.sweep_gate(last, s["forces"], fix["sweep"]["spread"]))
    for k, e in enumerate(fix["sweep"]["entries"]):
        assert abs(last[k] - e["av"]) <= 1e-6 * e["av"], (k, last[k], e)          # the restatement's steady value, stops apart

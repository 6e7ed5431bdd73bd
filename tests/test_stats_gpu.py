"""Running statistics (include/lbm.h, "Running statistics"; lbm_dstats_*) on the GPU: dp_stats_sample and the cuts of a run
against a twin handle of the same settings with statistics OFF, bit for bit.

Expected sums never come from the code under test: the twin is advanced with run() in pieces to every sample step, its
final_state() is read there (the output stage the existing tests pin) and accumulated in numpy float64 by tests/_stats_ref.py,
`acc = acc + v` per sample.  Every comparison is np.array_equal.  Because the twin ends at the same step count, cells, av_vels,
the fields, the Reynolds number, the force record, the scalar and its record are compared with it as well: nothing else moves.

The cases are tests/_dp_matrix.py's (make_case: three members, each with its own obstacle map, omega and state; a blocked cell in
column 0 and in column nx - 1) on 19x9 (odd nx: the row's last lane holds one cell), 33x12 (a second 16-cell segment holding one
cell) and 40x20 (crosses the 16x16 LDS tiles in both axes), through LBMDouble at "multistep" 0, 3 and 8 and EnsembleDouble, with
every in {1, 3, 4, 7} and the runs (10, 5, 6) against one run of 21: every = 4 cuts a launch of three steps, every = 7 samples at
7, 14 and 21, the last at a run's end.  On an MI355X the 66 cases take 3 s."""
import numpy as np
import pytest

import _dp_matrix as dm
import _drive_ref as dref
import _stats_ref as ref
from _steady_rule import OMEGAS, TOL, sweep

pytestmark = pytest.mark.gpu

LBM_ERR_ARG, LBM_ERR_STATE = 1, 3
SHAPES = [(19, 9), (33, 12), (40, 20)]
FAMILIES = [0, 3, 8, "ensemble"]
EVERYS = [1, 3, 4, 7]
RUNS = (10, 5, 6)
BS = [(3e-5, -2e-5), (-1e-5, 4e-5), (2e-5, 1e-5)]                              # buoyancy per member (tests/test_buoy_gpu.py)
C_REFS = [1.0, 0.8, 1.2]


def make_case(lbm, nx, ny, steps=40, force=0, trt=0, opened=0, **options):
    return dm.make_case(lbm, nx, ny, 3, steps, force, trt, opened, **options)


def open_handle(lbm, family, case, k=0, record=False, buoy=False):
    """member k as an LBMDouble at "multistep" `family`, or all members as an EnsembleDouble: uploaded, with the case's options"""
    scalar = case.members[0].scalar is not None
    if family == "ensemble":
        h, ks = dm.open_ensemble(lbm, case, scalar=scalar), list(range(case.n))
    else:
        h, ks = dm.open_context(lbm, case, case.members[k], family, scalar=scalar), [k]
    if buoy:
        if len(ks) == 1:
            h.set_buoyancy(BS[k], C_REFS[k])
        else:
            h.set_buoyancy([BS[i] for i in ks], [C_REFS[i] for i in ks])
    if record:
        h.set_scalar_record(True)
    return h


def snapshot(h, case):
    """everything but the statistics, as a flat list of arrays"""
    cells, av = h.download()
    out = [cells, av, np.asarray(h.reynolds())] + list(h.final_state())
    if case.force:
        out += list(h.force_record()) + [np.asarray(v) for v in h.force()]
    if case.members[0].scalar is not None:
        out += [h.scalar_cells(), h.scalar_field()]
        if h.scalar_record_on():
            out += list(h.scalar_record())
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def run_with_stats(h, every, runs, before=0):
    if before:
        h.run(before)
    assert h.stats_state() is None
    h.set_stats(every)
    assert h.stats_state() == (every, before, 0)
    assert not h.stats_sums().any() and not np.signbit(h.stats_sums()).any()       # +0.0
    for r in runs:
        h.run(r)
    return h.stats_state(), h.stats_sums()


def check(lbm, family, case, every, k=0, before=0, splits=(RUNS, (sum(RUNS),)), **how):
    """statistics on against the twin's accumulation, for each split of the run; the splits against each other"""
    got = []
    for runs in splits:
        with open_handle(lbm, family, case, k, **how) as h, open_handle(lbm, family, case, k, **how) as twin:
            state, sums = run_with_stats(h, every, runs, before)
            twin.run(before)
            acc = ref.twin_sums(twin, runs, before, every)
            assert state == (every, before, acc.samples) and acc.samples == len(ref.sample_points(before, sum(runs), before, every))
            assert sums.shape == acc.sums().shape and np.array_equal(sums, acc.sums()), (family, every, runs)
            assert h.steps_done == twin.steps_done == before + sum(runs)
            snap = snapshot(h, case)
            assert same(snap, snapshot(twin, case)), (family, every, runs)          # nothing else moves
            got.append((state, sums, snap))
    for other in got[1:]:
        assert other[0] == got[0][0] and np.array_equal(other[1], got[0][1]) and same(other[2], got[0][2])
    return got[0]


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("every", EVERYS)
def test_sums_equal_the_twins_fields_accumulated(lbm, nx, ny, family, every):
    """run(10); run(5); run(6) and one run of 21, with "force" on so that the force record is among what must not move"""
    case = make_case(lbm, nx, ny, force=1)
    state, sums, _ = check(lbm, family, case, every, k=SHAPES.index((nx, ny)))
    assert state[2] == 21 // every
    # a blocked cell holds 0, 0, samples times density / 3 added up, 0, 0, 0
    ms = case.members if family == "ensemble" else [case.members[SHAPES.index((nx, ny))]]
    for S, m in zip(sums.reshape((len(ms), 6, ny, nx)), ms):
        blocked = m.ob != 0
        pr = 0.0
        for _ in range(state[2]):
            pr = pr + m.p.density * (1.0 / 3.0)
        assert blocked[:, 0].any() and blocked[:, nx - 1].any()
        for v in (0, 1, 3, 4, 5):
            assert not S[v][blocked].any()
        assert np.all(S[2][blocked] == pr)
        assert np.all(S[3][~blocked] > 0.0) and np.all(S[2][~blocked] > 0.0)


@pytest.mark.parametrize("family", [0, 8, "ensemble"])
def test_statistics_start_behind_a_transient(lbm, family):
    """set_stats behind 5 steps: the samples fall on 5 + j every"""
    case = make_case(lbm, 33, 12)
    assert ref.sample_points(5, 11, 5, 3) == [8, 11, 14]
    state, _, _ = check(lbm, family, case, 3, k=1, before=5, splits=((4, 7), (11,)))
    assert state == (3, 5, 3)


COMPOSED = {"body force": dict(drive="on"),
            "open boundaries": dict(opened=1),
            "TRT, a moving wall and LES": dict(trt=1, wall="on", les="on", force=1),
            "passive scalar": dict(scalar=True, drive="on"),
            "buoyancy": dict(scalar=True)}


@pytest.mark.parametrize("family", [0, "ensemble"])
@pytest.mark.parametrize("name", list(COMPOSED))
def test_sums_with_the_flow_options(lbm, name, family):
    case = make_case(lbm, 33, 12, **COMPOSED[name])
    how = dict(record=True) if name == "passive scalar" else dict(buoy=True, record=True) if name == "buoyancy" else {}
    state, sums, _ = check(lbm, family, case, 4, k=2, **how)
    assert state == (4, 0, 5)
    if name == "body force":
        # the half-force correction shows in the sums: the same flow read without it gives other bits
        with open_handle(lbm, family, case, 2) as h:
            h.run(4)
            cells = h.download(av_vels=False)[0].reshape((-1, 9, 12, 33))
        rho = cells.sum(axis=1)
        fluid = np.stack([m.ob == 0 for m in (case.members if family == "ensemble" else [case.members[2]])])
        raw = (cells[:, 1] + cells[:, 5] + cells[:, 8] - cells[:, 3] - cells[:, 6] - cells[:, 7])[fluid] / rho[fluid]
        with open_handle(lbm, family, case, 2) as h:
            first = run_with_stats(h, 4, (4,))[1].reshape((-1, 6, 12, 33))[:, 0][fluid]
        assert np.all(first != raw) and np.allclose(first, raw, rtol=0, atol=1e-3)


def test_a_member_equals_its_context(lbm):
    case = make_case(lbm, 19, 9, force=1, drive="on")
    with open_handle(lbm, "ensemble", case) as ens:
        state, sums = run_with_stats(ens, 3, RUNS)
        snap = snapshot(ens, case)
    for k in range(case.n):
        with open_handle(lbm, (0, 3, 8)[k], case, k) as sim:
            one_state, one_sums = run_with_stats(sim, 3, RUNS)
            assert one_state == state and np.array_equal(one_sums, sums[k]), k
            one = snapshot(sim, case)
        assert same(one, [np.asarray(a)[k] for a in snap])


def test_setting_again_and_the_uploads_start_anew(lbm):
    case = make_case(lbm, 19, 9)
    m = case.members[0]
    for family in (8, "ensemble"):
        with open_handle(lbm, family, case) as h, open_handle(lbm, family, case) as twin:
            assert run_with_stats(h, 2, (6,))[0] == (2, 0, 3)
            h.set_stats(3)                                                         # again: zeros, a new origin, another every
            assert h.stats_state() == (3, 6, 0) and not h.stats_sums().any()
            h.run(7)
            twin.run(6)
            acc = ref.twin_sums(twin, (7,), 6, 3)
            assert h.stats_state() == (3, 6, 2) and np.array_equal(h.stats_sums(), acc.sums())
            # upload(): the setting stays, sums and count start anew, the origin is the step count behind the upload
            cells0 = m.cells0 if family == 8 else np.stack([x.cells0 for x in case.members])
            h.upload(cells0)
            twin.upload(cells0)
            assert h.stats_state() == (3, 0, 0) and not h.stats_sums().any()
            h.run(7)
            acc = ref.twin_sums(twin, (7,), 0, 3)
            assert h.stats_state() == (3, 0, 2) and np.array_equal(h.stats_sums(), acc.sums())
            if family == 8:
                # upload_obstacles(): the same, at the step count as it stands
                ob = case.members[1].ob
                h.upload_obstacles(ob)
                twin.upload_obstacles(ob)
                assert h.stats_state() == (3, 7, 0) and not h.stats_sums().any()
                h.run(6)
                acc = ref.twin_sums(twin, (6,), 7, 3)
                assert h.stats_state() == (3, 7, 2) and np.array_equal(h.stats_sums(), acc.sums())
                assert np.array_equal(h.download()[0], twin.download()[0])
            # off: no state, no sums
            h.set_stats(0)
            assert h.stats_state() is None
            buf = np.full(3 * 6 * 9 * 19, 7.0)
            symbol = h.lib.lbm_dstats if family == 8 else h.lib.lbm_dstats_ens
            assert symbol(getattr(h, h._handle), buf.ctypes.data) == LBM_ERR_STATE
            assert "statistics are off" in h.lib.lbm_last_error().decode() and np.all(buf == 7.0)
            with pytest.raises(lbm.LBMError):
                h.stats()
            h.run(2)                                                               # and runs as one that never had them
            twin.run(2)
            assert same(snapshot(h, case), snapshot(twin, case))


def test_steady_runs_are_refused_while_statistics_are_on(lbm):
    nx, ny = 48, 32
    params, ob = sweep(lbm, nx, ny, OMEGAS[4])
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.set_option("force", 1)
        ens.upload(None)
        ens.set_stats(5)
        ens.run(10)
        state, sums, cells = ens.stats_state(), ens.stats_sums(), ens.download()
        calls = {"lbm_dsteady_run": lambda: ens.lib.lbm_dsteady_run(ens.ens, 50, 7, TOL),
                 "lbm_dbody_steady_run": lambda: ens.lib.lbm_dbody_steady_run(ens.ens, 50, 7, TOL),
                 "lbm_drecord_steady_run": lambda: ens.lib.lbm_drecord_steady_run(ens.ens, 50, 7, TOL, 0)}
        for name, call in calls.items():
            assert call() == LBM_ERR_ARG, name
            msg = ens.lib.lbm_last_error().decode()
            assert name in msg and "statistics" in msg and "lbm_dstats_ens_set" in msg, msg
        # nothing changed by the refusals
        assert ens.steps_done == 10 and ens.stats_state() == state and np.array_equal(ens.stats_sums(), sums)
        assert same(list(ens.download()), list(cells)) and ens.member_steps()[0].tolist() == [10] * 4
        ens.run(5)
        assert ens.stats_state() == (5, 0, 3)
        # off: the steady runs work again, and a ragged ensemble refuses the statistics
        ens.set_stats(0)
        steps, _ = ens.run_until(40, window=7, rel_tol=TOL, on="drag")
        assert 15 < ens.steps_done <= 55 and steps.max() == ens.steps_done
        ens.upload(None)
        steps, _ = ens.run_until(200, window=7, rel_tol=TOL)
        assert len(set(steps.tolist())) > 1
        assert ens.lib.lbm_dstats_ens_set(ens.ens, 3) == LBM_ERR_STATE
        assert "lbm_dens_upload" in ens.lib.lbm_last_error().decode() and ens.stats_state() is None
        ens.set_stats(0)                                                           # off is no change: accepted
        ens.upload(None)
        ens.set_stats(3)
        ens.run(3)
        assert ens.stats_state() == (3, 0, 1)
    # the scalar's criterion on members that carry a scalar and its record: refused, then at work again
    case = make_case(lbm, 19, 9, scalar=True)
    with open_handle(lbm, "ensemble", case, record=True) as ens:
        ens.set_stats(2)
        ens.run(4)
        assert ens.lib.lbm_drecord_steady_run(ens.ens, 6, 3, TOL, 0) == LBM_ERR_ARG
        assert "lbm_dstats_ens_set" in ens.lib.lbm_last_error().decode() and ens.steps_done == 4 and ens.stats_state() == (2, 0, 2)
        ens.set_stats(0)
        steps, _ = ens.run_until(6, window=3, rel_tol=TOL, on="scalar")
        assert 4 < steps.max() <= 10 and ens.steps_done == steps.max()


def test_means_and_covariances_are_the_stated_numpy_statements(lbm):
    case = make_case(lbm, 33, 12)
    for family in (0, "ensemble"):
        with open_handle(lbm, family, case, 1) as h:
            h.set_stats(2)
            with pytest.raises(lbm.LBMError):                                      # zero samples
                h.stats()
            h.run(9)
            S, st = h.stats_sums(), h.stats()
        S = np.moveaxis(S, -3, 0)
        n = 4
        assert st["samples"] == n and sorted(st) == sorted(["samples", "u_x", "u_y", "pressure", "uxux", "uyuy", "uxuy"])
        u_x, u_y = S[0] / n, S[1] / n
        assert np.array_equal(st["u_x"], u_x) and np.array_equal(st["u_y"], u_y) and np.array_equal(st["pressure"], S[2] / n)
        assert np.array_equal(st["uxux"], S[3] / n - u_x * u_x) and np.array_equal(st["uyuy"], S[4] / n - u_y * u_y)
        assert np.array_equal(st["uxuy"], S[5] / n - u_x * u_y)
        assert st["u_x"].shape == ((3, 12, 33) if family == "ensemble" else (12, 33))


def test_variances_of_a_resting_closed_box(lbm):
    """The closed box under gravity of tests/test_drive_gpu.py (test_hydrostatic_balance), at rest to a residual velocity of
    4e-16: a variance formed from raw sums may round below zero, but not beyond rounding.  The bound is -1e-20, set beside the square of
    that residual before anything was measured; on an MI355X the smallest uxux and uyuy are 0.0, the largest 6.3e-33 and 9.0e-32."""
    hs = dref.HYDROSTATIC
    ob = dref.box_mask(hs["nx"], hs["ny"])
    omega, magic = hs["cases"][0]
    p = lbm.make_dparams(hs["nx"], hs["ny"], hs["steps"] + 16, density=dref.DENSITY, accel=0.0, omega=omega, obstacles=ob)
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_option("multistep", 8)
        sim.set_trt(magic)
        sim.set_drive(hs["force"])
        sim.upload(None)
        sim.run(hs["steps"])
        sim.set_stats(1)
        sim.run(16)
        st = sim.stats()
        uu = sim.final_state()[2]
    print("resting box: max |u| %.3e, min uxux %.3e, min uyuy %.3e, max uxux %.3e, max uyuy %.3e" %
          (uu.max(), st["uxux"].min(), st["uyuy"].min(), st["uxux"].max(), st["uyuy"].max()))
    assert st["samples"] == 16 and uu.max() <= 1e-12
    assert st["uxux"].min() >= -1e-20 and st["uyuy"].min() >= -1e-20

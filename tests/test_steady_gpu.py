"""Steady runs on the GPU (lbm_steady_*, lbm_amd.Ensemble.run_until): every member of an ensemble advances until its own
av_vels record has settled, decided on the device.

What is expected never comes from the code under test.  The stop counts come from the record of a plain Ensemble of the
same members after run(max_steps), with the header's criterion applied in numpy float64.  The states come from fresh plain
Ensembles advanced to each distinct stop count c, and a member that stopped at c must equal them bit for bit in cells,
av_vels[:c], the four fields and the Reynolds number.

How the plain Ensemble is advanced to c matters for av_vels only.  The per-tile sums of a launch of 7 steps are added in
another order than those of a launch of 8, so the record of a step depends on the launch split in its last bit (include/lbm.h:
"av_vels agree up to summation order"; cells, fields and Reynolds numbers do not depend on it).  A steady run is DEFINED as legs
of lbm_ens_run(e, window), so the plain Ensemble is advanced by run(window) per leg, which is that split; against the
uninterrupted run(max_steps) record, av_vels[:c] is held to the summation-order bound of test_ensemble_gpu.py.

Case parameters: rel_tol 2e-2, max_steps 400, windows 7 / 16 / 20 on 48x32 and 37x29 channels with 4 and 24 members.  On the
fp32 oracle the 4-member 48x32 sweep stops at 208 / 304 / 400 (converged at the cap's own check point) / 400 (not converged)
with window 16, at 220 / 340 / 400 / 400 with window 20, and at 119 / 168 / 196 / 210 with window 7 (37x29: 176 / 272 / 368 / 400,
200 / 300 / 400 / 400, 112 / 161 / 196 / 210; margins 0.1 to 23 % of rel_tol).  With window 7 the change over 7 steps falls under
2 % long before step 400 for every omega, so no window-7 case at max_steps 400 can have a member at the cap: that condition
of the input is asserted for windows 16 and 20 there, and for window 7 on a further case with max_steps 200 (three stops below
the cap, one member at it, and a last leg of 4 steps)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LBM_ERR_STATE = 3
TOL, CAP = 2e-2, 400
OMEGAS = {4: (0.6, 1.0, 1.4, 1.7), 24: tuple(float(v) for v in np.linspace(0.6, 1.7, 24))}
_cache = {}


def channel(nx, ny):
    """rows 0 and ny-1 blocked plus a 4x4 block"""
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    ob[ny // 2 - 2:ny // 2 + 2, nx // 4:nx // 4 + 4] = 1
    return ob


def sweep(lbm, nx, ny, omegas, max_iters=CAP):
    ob = channel(nx, ny)
    base = lbm.make_params(nx, ny, max_iters, density=0.1, accel=0.005, omega=omegas[0], obstacles=ob)
    return lbm.sweep_params(base, omega=list(omegas)), ob


def rule(av, s0, max_steps, window, rel_tol):
    """the header's criterion on a downloaded record av float32[n, >= s0 + max_steps]: (steps, converged)"""
    n = av.shape[0]
    steps, conv = np.full(n, s0 + max_steps, dtype=np.int32), np.zeros(n, dtype=bool)
    for m in range(n):
        for s in range(s0 + window, s0 + max_steps + 1, window):
            if s - window < 1:
                continue
            a_now, a_then = np.float64(av[m, s - 1]), np.float64(av[m, s - window - 1])
            diff = np.abs(a_now - a_then)
            bound = np.float64(rel_tol) * np.abs(a_now)
            if diff <= bound:
                steps[m], conv[m] = s, True
                break
    return steps, conv


def snapshot(ens):
    cells, av = ens.download()
    return {"cells": cells, "av": av, "fields": ens.final_state(), "re": ens.reynolds()}


def plain_record(lbm, nx, ny, omegas, nsteps=CAP):
    """av_vels of a plain Ensemble after run(nsteps), computed once per sweep"""
    key = ("record", nx, ny, omegas, nsteps)
    if key not in _cache:
        params, ob = sweep(lbm, nx, ny, omegas, max(nsteps, CAP))
        with lbm.Ensemble(params, ob) as ens:
            ens.upload(None)
            ens.run(nsteps)
            _cache[key] = ens.download(cells=False)[1]
        _cache[key].setflags(write=False)
    return _cache[key]


def plain_in_legs(lbm, nx, ny, omegas, c, window, s0=0, ob=None):
    """a fresh plain Ensemble advanced to step count c as the header says a steady run advances: run(s0), then run(window)
    per leg and a shorter last one; computed once per (sweep, c, window, s0)"""
    key = ("legs", nx, ny, omegas, c, window, s0, None if ob is None else ob.tobytes())
    if key not in _cache:
        params, ob0 = sweep(lbm, nx, ny, omegas)
        if ob is not None:   # per-member maps: the channel, or all blocked
            for m in range(len(params)):
                if ob[m].all():
                    params[m].free_cells_inv = 1.0
        with lbm.Ensemble(params, ob0 if ob is None else ob) as ens:
            ens.upload(None)
            if s0:
                ens.run(s0)
            done = s0
            while done < c:
                leg = min(window, c - done)
                ens.run(leg)
                done += leg
            assert ens.steps_done == c
            _cache[key] = snapshot(ens)
    return _cache[key]


def assert_members_equal_plain_runs(lbm, nx, ny, omegas, got, steps, window, s0=0, ob=None, record=None):
    n, top = len(omegas), int(steps.max())
    assert got["av"].shape == (n, top)
    for c in sorted(set(int(v) for v in steps)):
        ref = plain_in_legs(lbm, nx, ny, omegas, c, window, s0, ob)
        for m in np.flatnonzero(steps == c):
            what = "member %d stopped at %d" % (m, c)
            assert np.array_equal(got["cells"][m], ref["cells"][m]), what
            assert np.array_equal(got["av"][m, :c], ref["av"][m, :c]), what
            assert np.all(got["av"][m, c:] == 0.0) and not np.any(np.signbit(got["av"][m, c:])), what
            for a, b in zip(got["fields"], ref["fields"]):
                assert np.array_equal(a[m], b[m]), what
            assert got["re"][m] == ref["re"][m], what
            if record is not None:
                # the uninterrupted run's record: the same numbers up to the order the tiles' sums are added in
                err = float(np.max(np.abs(got["av"][m, :c] - record[m, :c])))
                assert err <= 2e-6 * float(np.max(np.abs(record[m, :c]))) + 1e-12, what


# (window, max_steps): the three windows at 400 steps, and window 7 once more where the cap is in reach (module docstring)
RUNS = [(7, CAP), (16, CAP), (20, CAP), (7, 200)]


@pytest.mark.parametrize("window,max_steps", RUNS)
@pytest.mark.parametrize("n", [4, 24])
@pytest.mark.parametrize("nx,ny", [(48, 32), (37, 29)])
def test_run_until_stops_every_member_where_the_rule_says(lbm, nx, ny, n, window, max_steps):
    omegas = OMEGAS[n]
    record = plain_record(lbm, nx, ny, omegas)
    want_steps, want_conv = rule(record, 0, max_steps, window, TOL)
    print("%dx%d n=%d window=%d max_steps=%d: stops %s converged %s" % (nx, ny, n, window, max_steps, want_steps.tolist(),
                                                                         want_conv.astype(int).tolist()))
    # the case covers what it claims (conditions on the input, taken from the reference record)
    below = sorted(set(int(s) for s, c in zip(want_steps, want_conv) if c and s < max_steps))
    assert len(below) >= 2, below
    if (window, max_steps) != (7, CAP):
        assert np.any((want_steps == max_steps) & ~want_conv)
    if window == 7:
        # one launch per leg: a member that stops after an odd number of legs is held by the second grid array
        assert any((s // 7) % 2 == 1 for s in below) and any((s // 7) % 2 == 0 for s in below), below

    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.Ensemble(params, ob) as ens:
        ens.upload(None)
        steps, conv = ens.run_until(max_steps, window=window, rel_tol=TOL)
        assert steps.dtype == np.int32 and conv.dtype == bool and steps.shape == conv.shape == (n,)
        assert steps.tolist() == want_steps.tolist()
        assert conv.tolist() == want_conv.tolist()
        again_steps, again_conv = ens.member_steps()
        assert again_steps.tolist() == steps.tolist() and again_conv.tolist() == conv.tolist()
        assert ens.steps_done == int(want_steps.max())
        got = snapshot(ens)
        second = snapshot(ens)   # reading a ragged ensemble changes nothing
    assert_members_equal_plain_runs(lbm, nx, ny, omegas, got, steps, window, record=record)
    assert np.array_equal(got["cells"], second["cells"]) and np.array_equal(got["av"], second["av"])
    assert np.array_equal(got["re"], second["re"])


def test_ragged_ensemble_refuses_runs_until_an_upload(lbm):
    nx, ny, omegas, window = 48, 32, OMEGAS[4], 7
    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.Ensemble(params, ob) as ens:
        ens.upload(None)
        steps, _ = ens.run_until(200, window=window, rel_tol=TOL)
        assert len(set(steps.tolist())) > 1
        before = snapshot(ens)
        for call in (lambda: ens.run(1), lambda: ens.run_timed(1), lambda: ens.run_until(7, window=7, rel_tol=TOL)):
            with pytest.raises(lbm.LBMError) as err:
                call()
            assert "code %d" % LBM_ERR_STATE in str(err.value) and "lbm_ens_upload" in str(err.value)
        after = snapshot(ens)
        assert np.array_equal(before["cells"], after["cells"]) and np.array_equal(before["av"], after["av"])
        assert ens.member_steps()[0].tolist() == steps.tolist()
        # an upload makes it an ordinary ensemble again
        ens.upload(None)
        assert ens.steps_done == 0
        s, c = ens.member_steps()
        assert s.tolist() == [0] * 4 and not c.any()
        ens.run(8)
        got = snapshot(ens)
    ref = plain_in_legs(lbm, nx, ny, omegas, 8, 8)
    assert np.array_equal(got["cells"], ref["cells"]) and np.array_equal(got["av"], ref["av"])
    assert np.array_equal(got["re"], ref["re"])


@pytest.mark.parametrize("window", [7, 16])
def test_uniform_result_is_an_ordinary_ensemble_again(lbm, window):
    """a rel_tol that every member meets at the first check point, 2 * window (the first with a record entry one window
    back): all stop there, and run(5) continues as after run(window) twice.  With window 7 that is an even number of
    launches while the host has enqueued further legs by then: the parity must come back from the device."""
    nx, ny, omegas = 37, 29, OMEGAS[4]
    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.Ensemble(params, ob) as ens:
        ens.upload(None)
        steps, conv = ens.run_until(CAP, window=window, rel_tol=1e3)
        assert steps.tolist() == [2 * window] * 4 and conv.all()
        assert ens.steps_done == 2 * window
        at_stop = snapshot(ens)
        ens.run(5)
        assert ens.steps_done == 2 * window + 5 and ens.member_steps()[0].tolist() == [2 * window + 5] * 4
        got = snapshot(ens)
    ref = plain_in_legs(lbm, nx, ny, omegas, 2 * window, window)
    assert np.array_equal(at_stop["cells"], ref["cells"]) and np.array_equal(at_stop["av"], ref["av"])
    # run(window), run(window), run(5): the legs of plain_in_legs with c = 2 * window + 5
    ref = plain_in_legs(lbm, nx, ny, omegas, 2 * window + 5, window)
    assert np.array_equal(got["cells"], ref["cells"]) and np.array_equal(got["av"], ref["av"])
    assert np.array_equal(got["re"], ref["re"])
    for a, b in zip(got["fields"], ref["fields"]):
        assert np.array_equal(a, b)
    # and a plain run(2 * window + 5) in one piece: the same cells
    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.Ensemble(params, ob) as ens:
        ens.upload(None)
        ens.run(2 * window + 5)
        cells, av = ens.download()
    assert np.array_equal(got["cells"], cells)
    assert np.max(np.abs(got["av"] - av)) <= 2e-6 * np.max(np.abs(av)) + 1e-12


def test_resumed_run_counts_its_check_points_from_where_it_starts(lbm):
    nx, ny, omegas, window, s0 = 48, 32, OMEGAS[4], 16, 10
    record = plain_record(lbm, nx, ny, omegas)
    want_steps, want_conv = rule(record, s0, CAP - s0, window, TOL)
    print("resume at %d: stops %s" % (s0, want_steps.tolist()))
    assert all((s - s0) % window == 0 for s, c in zip(want_steps, want_conv) if c) and want_conv.any()
    assert want_steps.tolist() != rule(record, 0, CAP, window, TOL)[0].tolist()
    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.Ensemble(params, ob) as ens:
        ens.upload(None)
        ens.run(s0)
        steps, conv = ens.run_until(CAP - s0, window=window, rel_tol=TOL)
        got = snapshot(ens)
        with pytest.raises(lbm.LBMError) as err:      # ragged, and the record holds max_iters steps
            ens.run_until(1, window=1, rel_tol=TOL)
        assert "code %d" % LBM_ERR_STATE in str(err.value)
    assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
    assert_members_equal_plain_runs(lbm, nx, ny, omegas, got, steps, window, s0=s0, record=record)


def test_all_blocked_member_stops_at_the_first_check_point(lbm):
    nx, ny, omegas, window = 37, 29, OMEGAS[4], 7
    ob = np.stack([channel(nx, ny)] * 4)
    ob[2] = 1
    params, _ = sweep(lbm, nx, ny, omegas)
    params[2].free_cells_inv = 1.0   # 1 / 0 in the reference; any finite value, its av_vels are exactly 0
    with lbm.Ensemble(params, ob) as ens:
        ens.upload(None)
        steps, conv = ens.run_until(200, window=window, rel_tol=TOL)
        got = snapshot(ens)
    assert steps[2] == 2 * window and conv[2]
    assert np.all(got["av"][2] == 0.0) and got["re"][2] == 0.0
    record = plain_record(lbm, nx, ny, omegas)
    want_steps, want_conv = rule(record, 0, 200, window, TOL)
    others = [0, 1, 3]
    assert steps[others].tolist() == want_steps[others].tolist() and conv[others].tolist() == want_conv[others].tolist()
    assert_members_equal_plain_runs(lbm, nx, ny, omegas, got, steps, window, ob=ob)


def test_short_last_leg_is_run_and_not_checked(lbm):
    """max_steps 24 with window 16: step 16 has no entry one window back and step 24 ends a short leg, so no member is
    checked at all, although rel_tol 1e3 would stop every one of them"""
    nx, ny, omegas = 48, 32, OMEGAS[4]
    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.Ensemble(params, ob) as ens:
        ens.upload(None)
        steps, conv = ens.run_until(24, window=16, rel_tol=1e3)
        assert steps.tolist() == [24] * 4 and not conv.any() and ens.steps_done == 24
        got = snapshot(ens)
        ens.run_until(0, window=16, rel_tol=1e3)      # a no-op
        assert ens.steps_done == 24
        # the next check points are 24 + 16 (one window back: step 24) ...
        steps, conv = ens.run_until(40, window=16, rel_tol=1e3)
        assert steps.tolist() == [40] * 4 and conv.all()
    assert_members_equal_plain_runs(lbm, nx, ny, omegas, got, np.full(4, 24, dtype=np.int32), 16)


def test_members_are_independent(lbm):
    """member 2's omega changed: no other member's stop count or bits change"""
    nx, ny, window, k = 48, 32, 7, 2

    def run(omegas):
        params, ob = sweep(lbm, nx, ny, omegas)
        with lbm.Ensemble(params, ob) as ens:
            ens.upload(None)
            steps, conv = ens.run_until(200, window=window, rel_tol=TOL)
            return steps, conv, snapshot(ens)

    steps_a, conv_a, a = run(OMEGAS[4])
    changed = (0.6, 1.0, 1.15, 1.7)
    steps_b, conv_b, b = run(changed)
    assert steps_a[k] != steps_b[k]
    top = min(a["av"].shape[1], b["av"].shape[1])
    for m in range(4):
        same = (steps_a[m] == steps_b[m] and conv_a[m] == conv_b[m] and np.array_equal(a["cells"][m], b["cells"][m]) and
                np.array_equal(a["av"][m, :top], b["av"][m, :top]) and a["re"][m] == b["re"][m])
        assert same == (m != k), "member %d" % m
    assert_members_equal_plain_runs(lbm, nx, ny, changed, b, steps_b, window)

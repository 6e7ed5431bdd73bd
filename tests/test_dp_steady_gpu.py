"""Steady runs of double-precision ensembles on the GPU (lbm_dsteady_*, lbm_amd.EnsembleDouble.run_until): every member
advances until its own av_vels record has settled, decided on the device.

What is expected never comes from run_until.  The stop counts come from the record of a plain EnsembleDouble of the same
members after one run(max_steps), with the header's criterion applied in numpy float64.  The states come from fresh plain
EnsembleDoubles advanced by ONE run(c) per distinct stop count c and, for the 4-member cases, from LBMDouble contexts, one per
member, run(c): a member that stopped at c must equal them bit for bit in cells, av_vels[:c], the four fields and the Reynolds
number.  In fp64 a step's segment sums are added in one order whatever the depth of the launch, so no reference is advanced
in legs and no tolerance appears anywhere: np.array_equal throughout, with equal_nan only where a NaN is the expected value
(the record and Reynolds number of a member without a free cell whose free_cells_inv is inf).

Inputs: the channel sweep of test_steady_gpu.py in fp64 (rows 0 and ny-1 blocked plus a 4x4 block, density 0.1, accel 0.005,
rest state, rel_tol 2e-2, cap 400) on 48x32 and 37x29 (no multiple of the 16x16 tile in either direction) with 4 and 24
members.  With 3 steps per launch a window of 7 is 3 launches per leg and 20 is 7, so members stop on either grid array; 16 is
6 launches.  STOPS holds the 4-member stop counts of the fp64 CPU oracle; the smallest distance of any check from the
threshold is 1.7e-4 of rel_tol against rounding differences of order 1e-16, so the device's record must give the same."""
import numpy as np
import pytest

from _steady_rule import CAP, OMEGAS, TOL, channel, rule, sweep

pytestmark = pytest.mark.gpu

LBM_ERR_STATE = 3
# (nx, ny, window, max_steps) -> the 4-member stops on the fp64 oracle
STOPS = {(48, 32, 7, 400): [119, 168, 196, 210], (48, 32, 16, 400): [208, 304, 400, 400], (48, 32, 20, 400): [220, 340, 400, 400],
         (48, 32, 7, 200): [119, 168, 196, 200], (37, 29, 7, 400): [112, 161, 196, 210], (37, 29, 16, 400): [176, 272, 368, 400],
         (37, 29, 20, 400): [200, 300, 400, 400], (37, 29, 7, 200): [112, 161, 196, 200]}
_cache = {}


def members(lbm, nx, ny, omegas, ob=None, inv=None):
    """(params, obstacles) of a sweep; ob: per-member maps instead of the channel; inv: {member: free_cells_inv}"""
    params, ob0 = sweep(lbm, nx, ny, omegas)
    for m, v in (inv or {}).items():
        params[m].free_cells_inv = v
    return params, (ob0 if ob is None else ob)


def snapshot(sim):
    with np.errstate(all="ignore"):
        cells, av = sim.download()
        return {"cells": cells, "av": av, "fields": sim.final_state(), "re": sim.reynolds()}


def key_of(nx, ny, omegas, ob, inv):
    return (nx, ny, omegas, None if ob is None else ob.tobytes(), tuple(sorted((inv or {}).items())))


def plain_record(lbm, nx, ny, omegas, ob=None, inv=None):
    """av_vels of a plain EnsembleDouble after one run(CAP), computed once per sweep"""
    key = ("record",) + key_of(nx, ny, omegas, ob, inv)
    if key not in _cache:
        params, obs = members(lbm, nx, ny, omegas, ob, inv)
        with lbm.EnsembleDouble(params, obs) as ens:
            ens.upload(None)
            ens.run(CAP)
            with np.errstate(all="ignore"):
                _cache[key] = ens.download(cells=False)[1]
        _cache[key].setflags(write=False)
    return _cache[key]


def plain_at(lbm, nx, ny, omegas, c, ob=None, inv=None):
    """a fresh plain EnsembleDouble advanced to step count c by ONE run(c); computed once per (sweep, c)"""
    key = ("plain", c) + key_of(nx, ny, omegas, ob, inv)
    if key not in _cache:
        params, obs = members(lbm, nx, ny, omegas, ob, inv)
        with lbm.EnsembleDouble(params, obs) as ens:
            ens.upload(None)
            ens.run(c)
            assert ens.steps_done == c
            _cache[key] = snapshot(ens)
    return _cache[key]


def context_at(lbm, nx, ny, omega, c):
    """an LBMDouble of one member of the channel sweep after one run(c); computed once per (grid, omega, c)"""
    key = ("context", nx, ny, omega, c)
    if key not in _cache:
        ob = channel(nx, ny)
        p = lbm.make_dparams(nx, ny, CAP, density=0.1, accel=0.005, omega=omega, obstacles=ob)
        with lbm.LBMDouble(p, ob) as sim:
            sim.upload(None)
            sim.run(c)
            _cache[key] = snapshot(sim)
    return _cache[key]


def same(a, b, nan=False):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=nan)


def assert_members_equal_plain_runs(lbm, nx, ny, omegas, got, steps, ob=None, inv=None, contexts=False, nan_members=()):
    n, top = len(omegas), int(steps.max())
    assert got["av"].shape == (n, top) and got["av"].dtype == np.float64 and got["cells"].dtype == np.float64
    for c in sorted(set(int(v) for v in steps)):
        ref = plain_at(lbm, nx, ny, omegas, c, ob, inv)
        for m in np.flatnonzero(steps == c):
            what = "member %d stopped at %d" % (m, c)
            nan = m in nan_members
            assert same(got["cells"][m], ref["cells"][m]), what
            assert same(got["av"][m, :c], ref["av"][m, :c], nan), what
            assert np.all(got["av"][m, c:] == 0.0) and not np.any(np.signbit(got["av"][m, c:])), what
            for a, b in zip(got["fields"], ref["fields"]):
                assert same(a[m], b[m]), what
            assert same(got["re"][m], ref["re"][m], nan), what
            if contexts:
                ctx = context_at(lbm, nx, ny, omegas[m], c)
                assert same(got["cells"][m], ctx["cells"]) and same(got["av"][m, :c], ctx["av"]), what + " (LBMDouble)"
                for a, b in zip(got["fields"], ctx["fields"]):
                    assert same(a[m], b), what + " (LBMDouble)"
                assert got["re"][m] == ctx["re"], what + " (LBMDouble)"


# (window, max_steps): the three windows at 400 steps, and window 7 once more where the cap is in reach and the last leg is 4 steps
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
        # a member that stops after an odd number of legs of 3 launches is held by the second grid array
        assert any((s // 7) % 2 == 1 for s in below) and any((s // 7) % 2 == 0 for s in below), below
    if n == 4:
        assert want_steps.tolist() == STOPS[(nx, ny, window, max_steps)]   # the fp64 oracle's

    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.EnsembleDouble(params, ob) as ens:
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
    assert_members_equal_plain_runs(lbm, nx, ny, omegas, got, steps, contexts=(n == 4))
    # the uninterrupted run's record, bit for bit
    for m in range(n):
        assert same(got["av"][m, :steps[m]], record[m, :steps[m]]), m
    assert same(got["cells"], second["cells"]) and same(got["av"], second["av"]) and same(got["re"], second["re"])
    for a, b in zip(got["fields"], second["fields"]):
        assert same(a, b)


def test_ragged_ensemble_refuses_runs_until_an_upload(lbm):
    nx, ny, omegas, window = 48, 32, OMEGAS[4], 7
    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.upload(None)
        steps, _ = ens.run_until(200, window=window, rel_tol=TOL)
        assert len(set(steps.tolist())) > 1
        before = snapshot(ens)
        for call in (lambda: ens.run(1), lambda: ens.run_timed(1), lambda: ens.run_until(7, window=7, rel_tol=TOL)):
            with pytest.raises(lbm.LBMError) as err:
                call()
            assert "code %d" % LBM_ERR_STATE in str(err.value) and "lbm_dens_upload" in str(err.value)
        after = snapshot(ens)
        assert same(before["cells"], after["cells"]) and same(before["av"], after["av"]) and same(before["re"], after["re"])
        assert ens.member_steps()[0].tolist() == steps.tolist() and ens.steps_done == int(steps.max())
        # an upload makes it an ordinary ensemble again
        ens.upload(None)
        assert ens.steps_done == 0
        s, c = ens.member_steps()
        assert s.tolist() == [0] * 4 and not c.any()
        ens.run(8)
        got = snapshot(ens)
    ref = plain_at(lbm, nx, ny, omegas, 8)
    assert same(got["cells"], ref["cells"]) and same(got["av"], ref["av"]) and same(got["re"], ref["re"])
    for a, b in zip(got["fields"], ref["fields"]):
        assert same(a, b)


@pytest.mark.parametrize("window", [7, 16])
def test_uniform_result_is_an_ordinary_ensemble_again(lbm, window):
    """a rel_tol that every member meets at the first check point, 2 * window (the first with a record entry one window
    back): all stop there, and run(5) continues.  The host has enqueued further legs by then (with window 7, an odd number
    of launches each): the parity must come back from the device."""
    nx, ny, omegas = 37, 29, OMEGAS[4]
    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.upload(None)
        steps, conv = ens.run_until(CAP, window=window, rel_tol=1e3)
        assert steps.tolist() == [2 * window] * 4 and conv.all()
        assert ens.steps_done == 2 * window
        at_stop = snapshot(ens)
        ens.run(5)
        assert ens.steps_done == 2 * window + 5 and ens.member_steps()[0].tolist() == [2 * window + 5] * 4
        got = snapshot(ens)
    for snap, c in ((at_stop, 2 * window), (got, 2 * window + 5)):
        ref = plain_at(lbm, nx, ny, omegas, c)   # ONE run(c) of a fresh ensemble
        assert same(snap["cells"], ref["cells"]) and same(snap["av"], ref["av"]) and same(snap["re"], ref["re"])
        for a, b in zip(snap["fields"], ref["fields"]):
            assert same(a, b)


def test_resumed_run_counts_its_check_points_from_where_it_starts(lbm):
    nx, ny, omegas, window, s0 = 48, 32, OMEGAS[4], 16, 10
    record = plain_record(lbm, nx, ny, omegas)
    want_steps, want_conv = rule(record, s0, CAP - s0, window, TOL)
    print("resume at %d: stops %s" % (s0, want_steps.tolist()))
    assert want_steps.tolist() == [202, 298, 394, 400]   # the fp64 oracle's
    assert all((s - s0) % window == 0 for s, c in zip(want_steps, want_conv) if c) and want_conv.any()
    assert want_steps.tolist() != rule(record, 0, CAP, window, TOL)[0].tolist()
    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.upload(None)
        ens.run(s0)
        steps, conv = ens.run_until(CAP - s0, window=window, rel_tol=TOL)
        got = snapshot(ens)
        with pytest.raises(lbm.LBMError) as err:      # ragged, and the record holds max_iters steps
            ens.run_until(1, window=1, rel_tol=TOL)
        assert "code %d" % LBM_ERR_STATE in str(err.value)
    assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
    assert_members_equal_plain_runs(lbm, nx, ny, omegas, got, steps, contexts=True)


@pytest.mark.parametrize("inv", [1.0, float("inf")])
def test_member_without_a_free_cell(lbm, inv):
    """free_cells_inv 1.0 (any finite value): a record of exact zeros, stopped at the first check point.  inf, as the
    reference's 1 / 0 gives: 0 * inf, a record of NaNs, which never meets the criterion - to the cap, not converged."""
    nx, ny, omegas, window, k = 37, 29, OMEGAS[4], 7, 2
    ob = np.stack([channel(nx, ny)] * 4)
    ob[k] = 1
    params, obs = members(lbm, nx, ny, omegas, ob, {k: inv})
    with lbm.EnsembleDouble(params, obs) as ens:
        ens.upload(None)
        steps, conv = ens.run_until(200, window=window, rel_tol=TOL)
        got = snapshot(ens)
    if np.isinf(inv):
        assert steps[k] == 200 and not conv[k]
        assert np.all(np.isnan(got["av"][k])) and np.isnan(got["re"][k])
    else:
        assert steps[k] == 2 * window and conv[k]
        assert np.all(got["av"][k] == 0.0) and not np.any(np.signbit(got["av"][k])) and got["re"][k] == 0.0
    # the rule on this ensemble's own plain record says the same of member k, and the others are the channel sweep's
    want_steps, want_conv = rule(plain_record(lbm, nx, ny, omegas, ob, {k: inv}), 0, 200, window, TOL)
    assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
    channel_steps, channel_conv = rule(plain_record(lbm, nx, ny, omegas), 0, 200, window, TOL)
    others = [m for m in range(4) if m != k]
    assert steps[others].tolist() == channel_steps[others].tolist() and conv[others].tolist() == channel_conv[others].tolist()
    assert_members_equal_plain_runs(lbm, nx, ny, omegas, got, steps, ob=ob, inv={k: inv}, nan_members=(k,) if np.isinf(inv) else ())
    for c in sorted(set(int(steps[m]) for m in others)):   # ... bit for bit
        ref = plain_at(lbm, nx, ny, omegas, c)
        for m in others:
            if steps[m] == c:
                assert same(got["cells"][m], ref["cells"][m]) and same(got["av"][m, :c], ref["av"][m]), m


def test_short_last_leg_is_run_and_not_checked(lbm):
    """max_steps 24 with window 16: step 16 has no entry one window back and step 24 ends a short leg, so no member is
    checked at all, although rel_tol 1e3 would stop every one of them"""
    nx, ny, omegas = 48, 32, OMEGAS[4]
    params, ob = sweep(lbm, nx, ny, omegas)
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.upload(None)
        steps, conv = ens.run_until(24, window=16, rel_tol=1e3)
        assert steps.tolist() == [24] * 4 and not conv.any() and ens.steps_done == 24
        got = snapshot(ens)
        ens.run_until(0, window=16, rel_tol=1e3)      # a no-op
        assert ens.steps_done == 24
        # the next check point is 24 + 16 (one window back: step 24)
        steps, conv = ens.run_until(40, window=16, rel_tol=1e3)
        assert steps.tolist() == [40] * 4 and conv.all() and ens.steps_done == 40
        later = snapshot(ens)
    assert_members_equal_plain_runs(lbm, nx, ny, omegas, got, np.full(4, 24, dtype=np.int32), contexts=True)
    assert_members_equal_plain_runs(lbm, nx, ny, omegas, later, np.full(4, 40, dtype=np.int32))


def test_members_are_independent(lbm):
    """member 2's omega changed: no other member's stop count or bits change"""
    nx, ny, window, k = 48, 32, 7, 2

    def run(omegas):
        params, ob = sweep(lbm, nx, ny, omegas)
        with lbm.EnsembleDouble(params, ob) as ens:
            ens.upload(None)
            steps, conv = ens.run_until(200, window=window, rel_tol=TOL)
            return steps, conv, snapshot(ens)

    steps_a, conv_a, a = run(OMEGAS[4])
    changed = (0.6, 1.0, 1.15, 1.7)
    steps_b, conv_b, b = run(changed)
    top = min(a["av"].shape[1], b["av"].shape[1])
    for m in range(4):
        equal = (steps_a[m] == steps_b[m] and conv_a[m] == conv_b[m] and same(a["cells"][m], b["cells"][m]) and
                 same(a["av"][m, :top], b["av"][m, :top]) and a["re"][m] == b["re"][m])
        assert equal == (m != k), "member %d" % m
    assert_members_equal_plain_runs(lbm, nx, ny, changed, b, steps_b)


def test_plain_ensemble_interleaved_with_a_steady_run_of_another(lbm):
    """two ensembles on one device, each on its own stream: a plain one advanced before, between and after the legs of
    another's steady runs computes what it computes alone, and so does the steady one"""
    nx, ny, omegas, window = 37, 29, OMEGAS[4], 7
    record = plain_record(lbm, nx, ny, omegas)
    want_steps, want_conv = rule(record, 0, 200, window, TOL)
    params, ob = sweep(lbm, nx, ny, omegas)
    changed = (0.7, 1.1, 1.3, 1.6)
    other, _ = sweep(lbm, nx, ny, changed)
    with lbm.EnsembleDouble(params, ob) as steady, lbm.EnsembleDouble(other, ob) as plain:
        plain.upload(None)
        steady.upload(None)
        plain.run(5)                      # asynchronous: still in flight when the steady run starts
        steps, conv = steady.run_until(200, window=window, rel_tol=TOL)
        plain.run(6)
        got_steady = snapshot(steady)
        plain.run(10)
        got_plain = snapshot(plain)
    assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
    assert_members_equal_plain_runs(lbm, nx, ny, omegas, got_steady, steps)
    ref = plain_at(lbm, nx, ny, changed, 21)
    assert same(got_plain["cells"], ref["cells"]) and same(got_plain["av"], ref["av"]) and same(got_plain["re"], ref["re"])
    for a, b in zip(got_plain["fields"], ref["fields"]):
        assert same(a, b)

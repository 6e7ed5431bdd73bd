"""Drag of a body on the GPU: the force on chosen blocked cells (lbm_dbody_*, LBMDouble / EnsembleDouble .set_body() and
.body()) and steady runs that stop each member on its body's drag (run_until(on="drag")).

The reference value is tests/_force_ref.py's `body_restatement`: its `restatement` with `counted &= body`, on states downloaded
from the GPU and accelerated with the fp64 oracle's accelerate_flow.  Gates:
  1. record against the restatement, per component 8 L 2^-53 sum|link terms| with L and the sum over the BODY's links (the
     gate of test_force_gpu, derived there: four times the bound between two summation orders of the same terms);
  2. additivity of two disjoint bodies on one state: the same gate over all links;
  3. - 6. bit identity (np.array_equal), stop counts and error codes: no tolerance.
Shapes 16x16, 33x19, 48x35 and 3x3 at multistep 0, 3 and 8: a wrap in x and y, rows ny-1 .. ny-3, a tile seam at 15 | 16, a row
shorter than a segment and a lone cell.  Bodies per shape, on _force_ref.force_mask:
  a  the cells of the 4x5 block (on 3x3: the lone blocked cell, which is then every blocked cell)
  b  the other blocked cells
  c  every blocked cell
  d  no cell
  e  a blocked cell S with a blocked neighbour B in the body and a blocked neighbour N outside it (at the tile seam, (15, 15),
     where the grid has one; a corner of the block on 16x16), and the cell at x = 0 facing fluid across the wrap (not on 3x3)
The drag criterion's wanted stops never come from run_until: they are the header's rule in numpy float64 on the F_x record of
a plain EnsembleDouble run to the cap."""
import numpy as np
import pytest

from _force_ref import SHAPES, U, accelerated, block_body, body_restatement, case, force_mask, restatement, single_steps
from _steady_rule import OMEGAS, TOL, rule, sweep

pytestmark = pytest.mark.gpu

LBM_ERR_ARG, LBM_ERR_STATE = 1, 3
BODY_SHAPES = [s for s in SHAPES if s != (128, 128)]
STEPS = 12
CAP = 400


def block_rect(nx, ny):
    return slice(ny // 2 - 2, ny // 2 + 2), slice(nx // 4, nx // 4 + 5)


def seam_cells(ob):
    """body e's S, B, N: S blocked with a fluid neighbour, B and N two of its blocked neighbours"""
    ny, nx = ob.shape
    s = (15, 15) if nx > 16 and ny > 16 else (ny // 2 - 2, nx // 4)
    near = [((s[0] + dy) % ny, (s[1] + dx) % nx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
    blocked = [c for c in near if ob[c]]
    assert ob[s] and len(blocked) >= 2 and len(blocked) < 8, (s, blocked)
    return s, blocked[0], blocked[1]


def bodies(nx, ny):
    """{name: int32[ny, nx]} on force_mask(nx, ny), each asserted to be what it claims"""
    ob = force_mask(nx, ny)
    blocked = ob != 0
    out = {"c": blocked.astype(np.int32), "d": np.zeros((ny, nx), dtype=np.int32)}
    a = np.zeros((ny, nx), dtype=bool)
    if (nx, ny) == (3, 3):
        a[1, 1] = True
        assert np.array_equal(a, blocked)
    else:
        a[block_rect(nx, ny)] = True
        a &= blocked
        assert 18 <= np.count_nonzero(a) <= 20 and np.count_nonzero(blocked & ~a) > 0          # the block, and walls besides
        s, b, n = seam_cells(ob)
        e = np.zeros((ny, nx), dtype=bool)
        e[s] = e[b] = e[ny // 2, 0] = True
        assert blocked[s] and blocked[b] and blocked[n] and not e[n]                           # B in the body, N blocked outside it
        assert blocked[ny // 2, 0] and not blocked[ny // 2, nx - 1]                            # x = 0 facing fluid across the wrap
        if nx > 16 and ny > 16:
            assert s == (15, 15) and (b[1] == 16 or n[1] == 16 or b[0] == 16 or n[0] == 16)     # across the 15 | 16 seam
        assert np.count_nonzero(e) == 3 and not np.any(e & ~blocked)
        out["e"] = e.astype(np.int32)
    out["a"] = a.astype(np.int32)
    out["b"] = (blocked & ~a).astype(np.int32)
    assert not np.any(out["a"] & out["b"]) and np.array_equal(out["a"] | out["b"], out["c"])
    assert np.count_nonzero(out["a"]) > 0 and not np.any(out["d"])
    return out


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def test_bodies_hold_what_they_promise():
    for nx, ny in BODY_SHAPES:
        b = bodies(nx, ny)
        assert ("e" in b) == ((nx, ny) != (3, 3))
    f = np.random.default_rng(3).random((9, 19, 33))
    ob = force_mask(33, 19)
    assert body_restatement(f, ob, bodies(33, 19)["c"]) == restatement(f, ob)      # every blocked cell: the restatement itself


# ---- 1. record against the restatement ---------------------------------------------------------------------------------

_single = {}


def body_single_steps(lbm, nx, ny, multistep, name):
    """12 steps one at a time with body `name`: the state before each step, and the record.  Computed once per case."""
    key = (nx, ny, multistep, name)
    if key not in _single:
        p, ob, cells0 = case(lbm, nx, ny, STEPS)
        states = []
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("multistep", multistep)
            sim.set_option("force", 1)
            sim.set_body(bodies(nx, ny)[name])
            sim.upload(cells0)
            for _ in range(STEPS):
                states.append(sim.download(av_vels=False)[0])
                sim.run(1)
            fx, fy = sim.force_record()
        _single[key] = (p, ob, states, fx, fy)
    return _single[key]


# a 3x3 grid has one blocked cell: body a is the case there
RECORD_CASES = [(nx, ny, multistep, name) for nx, ny in BODY_SHAPES for multistep in (0, 3, 8) for name in ("a", "e")
                if (nx, ny, name) != (3, 3, "e")]


@pytest.mark.parametrize("nx,ny,multistep,name", RECORD_CASES)
def test_record_equals_the_restatement(lbm, oracle_f64, nx, ny, multistep, name):
    body = bodies(nx, ny)[name]
    p, ob, states, fx, fy = body_single_steps(lbm, nx, ny, multistep, name)
    _, _, none_states, nfx, nfy = single_steps(lbm, nx, ny, multistep)
    whole = np.array_equal(body != 0, ob != 0)
    assert whole == ((nx, ny) == (3, 3))
    for t in range(STEPS):
        assert np.array_equal(states[t], none_states[t])                       # the same states with and without a body
        rx, ry, links, mag = body_restatement(accelerated(oracle_f64, p, ob, states[t]), ob, body)
        tol = 8.0 * links * U * mag
        assert links > 0 and mag > 0.0
        print("%dx%d multistep %d body %s step %d: F = (%.6e, %.6e)  |dFx| %.2e |dFy| %.2e  tol %.2e  links %d  no body (%.6e, %.6e)"
              % (nx, ny, multistep, name, t, fx[t], fy[t], abs(fx[t] - rx), abs(fy[t] - ry), tol, links, nfx[t], nfy[t]))
        assert abs(fx[t] - rx) <= tol and abs(fy[t] - ry) <= tol, (t, fx[t], rx, fy[t], ry, tol)
        if whole:
            assert fx[t] == nfx[t] and fy[t] == nfy[t]
        else:
            # a kernel that ignores the body fails here
            assert max(abs(fx[t] - nfx[t]), abs(fy[t] - nfy[t])) > tol, (t, fx[t], nfx[t], fy[t], nfy[t], tol)
    # a kernel that counts nothing fails here
    assert max(np.max(np.abs(fx)), np.max(np.abs(fy))) > 1e-6, (fx, fy)


# ---- 2. additivity -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", BODY_SHAPES)
def test_two_disjoint_bodies_add_up_to_the_whole(lbm, oracle_f64, nx, ny):
    p, ob, cells0 = case(lbm, nx, ny, 8)
    b = bodies(nx, ny)
    with lbm.LBMDouble(p, ob) as sim:
        sim.upload(cells0)
        sim.run(5)
        state = sim.download(av_vels=False)[0]
        none = sim.force()
        sim.set_body(b["a"])
        fa = sim.force()
        sim.set_body(b["b"])
        fb = sim.force()
        sim.set_body(None)
        assert sim.force() == none
        assert np.array_equal(sim.download(av_vels=False)[0], state)
    _, _, links, mag = restatement(accelerated(oracle_f64, p, ob, state), ob)
    tol = 8.0 * links * U * mag
    print("%dx%d: a (%.6e, %.6e) + b (%.6e, %.6e) against (%.6e, %.6e), tol %.2e" % ((nx, ny) + fa + fb + none + (tol,)))
    assert links > 0
    for c in range(2):
        assert abs((fa[c] + fb[c]) - none[c]) <= tol, (c, fa, fb, none, tol)
    if (nx, ny) != (3, 3):
        assert fa != none and fb != none and fa != fb


# ---- 3. bit identity ---------------------------------------------------------------------------------------------------

RUNS = (1, 9, 5, 3)


def record_of(lbm, p, ob, cells0, multistep, runs, body, with_force=False):
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_option("multistep", multistep)
        sim.set_option("force", 1)
        if body is not False:
            sim.set_body(body)
        sim.upload(cells0)
        now = []
        for r in runs:
            now.append((sim.steps_done, sim.force()))
            sim.run(r)
        fx, fy = sim.force_record()
        last = sim.force()
    return (fx, fy, now, last) if with_force else (fx, fy)


def plus_zero(v):
    v = np.asarray(v)
    return bool(np.all(v == 0.0) and not np.any(np.signbit(v)))


@pytest.mark.parametrize("multistep", [0, 3, 8])
@pytest.mark.parametrize("nx,ny", BODY_SHAPES)
def test_every_blocked_cell_and_no_cell(lbm, nx, ny, multistep):
    steps = sum(RUNS)
    p, ob, cells0 = case(lbm, nx, ny, steps)
    b = bodies(nx, ny)
    nfx, nfy, nnow, nlast = record_of(lbm, p, ob, cells0, multistep, RUNS, False, True)
    cfx, cfy, cnow, clast = record_of(lbm, p, ob, cells0, multistep, RUNS, b["c"], True)
    assert np.array_equal(cfx, nfx) and np.array_equal(cfy, nfy) and cnow == nnow and clast == nlast
    assert np.array_equal(np.signbit(cfx), np.signbit(nfx)) and np.array_equal(np.signbit(cfy), np.signbit(nfy))
    assert np.any(nfx != 0.0)
    dfx, dfy, dnow, dlast = record_of(lbm, p, ob, cells0, multistep, RUNS, b["d"], True)
    assert dfx.shape == (steps,) and plus_zero(dfx) and plus_zero(dfy) and plus_zero(dlast)
    assert all(plus_zero(f) for _, f in dnow)


@pytest.mark.parametrize("nx,ny", BODY_SHAPES)
def test_record_with_a_body_is_bit_identical_between_forms_splits_runs_and_members(lbm, nx, ny):
    steps = sum(RUNS)
    p, ob, cells0 = case(lbm, nx, ny, steps + 1)
    b = bodies(nx, ny)
    ref = record_of(lbm, p, ob, cells0, 0, [steps], b["a"])
    assert ref[0].shape == (steps,) and np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1]))
    for multistep in (0, 3, 8):
        for runs in ([steps], RUNS):
            got = record_of(lbm, p, ob, cells0, multistep, runs, b["a"])
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (multistep, len(runs))
    fx, fy, now, last = record_of(lbm, p, ob, cells0, 8, RUNS + (1,), b["a"], True)          # a second run, one step more
    assert np.array_equal(fx[:steps], ref[0]) and np.array_equal(fy[:steps], ref[1])
    # force() equals the record entry the next step writes
    assert [t for t, _ in now] == [0, 1, 10, 15, 18]
    for t, (gx, gy) in now:
        assert gx == fx[t] and gy == fy[t], (t, gx, fx[t], gy, fy[t])
        assert np.signbit(gx) == np.signbit(fx[t]) and np.signbit(gy) == np.signbit(fy[t])
    refb = record_of(lbm, p, ob, cells0, 0, [steps], b["b"])
    # two members with different bodies in one ensemble: each a context with that body
    params = lbm.sweep_dparams(p, omega=[p.omega, p.omega])
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.set_option("force", 1)
        ens.set_body(np.stack([b["a"], b["b"]]))
        assert np.array_equal(ens.body(), np.stack([b["a"], b["b"]]))
        ens.upload(np.stack([cells0, cells0]))
        for r in RUNS:
            ens.run(r)
        efx, efy = ens.force_record()
        enow = ens.force()
        ens.run(1)
        nfx, nfy = ens.force_record()
    assert np.array_equal(efx[0], ref[0]) and np.array_equal(efy[0], ref[1])
    assert np.array_equal(efx[1], refb[0]) and np.array_equal(efy[1], refb[1])
    assert np.array_equal(enow[0], nfx[:, steps]) and np.array_equal(enow[1], nfy[:, steps])
    assert enow[0][0] == fx[steps] and enow[1][0] == fy[steps]
    if (nx, ny) != (3, 3):
        assert not np.array_equal(efx[0], efx[1])


# ---- 4. nothing else moves ---------------------------------------------------------------------------------------------

def snapshot(sim):
    cells, av = sim.download()
    return [cells, av] + list(sim.final_state()) + [sim.reynolds()]


@pytest.mark.parametrize("force", [0, 1])
@pytest.mark.parametrize("multistep", [0, 3])
def test_context_computes_the_same_with_a_body(lbm, multistep, force):
    p, ob, cells0 = case(lbm, 48, 35, 40)
    snaps = []
    for body in (None, bodies(48, 35)["a"]):
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("multistep", multistep)
            sim.set_option("force", force)
            sim.set_body(body)
            sim.upload(cells0)
            for r in (1, 9, 30):
                sim.run(r)
            snaps.append(snapshot(sim))
    for a, b in zip(*snaps):
        assert np.array_equal(a, b)


def test_ensemble_computes_the_same_with_a_body(lbm):
    p, ob, cells0 = case(lbm, 48, 35, 40)
    params = lbm.sweep_dparams(p, omega=[1.2, 1.7, 0.9])
    b = bodies(48, 35)
    snaps = []
    for body in (None, np.stack([b["a"], b["e"], b["d"]])):
        with lbm.EnsembleDouble(params, ob) as ens:
            ens.set_option("force", 1)
            ens.set_body(body)
            ens.upload(np.stack([cells0] * 3))
            for r in (1, 9, 30):
                ens.run(r)
            snaps.append(snapshot(ens))
    for x, y in zip(*snaps):
        assert np.array_equal(x, y)


# ---- 5. state rules ----------------------------------------------------------------------------------------------------

def test_state_rules(lbm):
    lib = lbm.load_library()
    nx, ny = 33, 19
    p, ob, cells0 = case(lbm, nx, ny, 8)
    b = bodies(nx, ny)
    with lbm.LBMDouble(p, ob) as sim:
        assert np.array_equal(sim.body(), b["c"])                       # the default: every blocked cell
        sim.set_body(b["a"])
        assert np.array_equal(sim.body(), b["a"]) and sim.body().dtype == np.int32      # round trip
        sim.set_body(7 * b["a"])                                        # any non-zero value
        assert np.array_equal(sim.body(), b["a"])
        sim.upload(cells0)                                              # an upload keeps it
        assert np.array_equal(sim.body(), b["a"])
        sim.run(2)
        fa = sim.force()
        sim.set_body(b["e"])                                            # "force" off: accepted after steps
        fe = sim.force()
        sim.set_body(b["a"])
        assert sim.force() == fa and fe != fa
        # a non-zero on a fluid cell: refused, the message names the cell, nothing changes
        bad = b["a"].copy()
        y, x = [int(v[0]) for v in np.nonzero(ob == 0)]
        bad[y, x] = 1
        bad[ny - 1, nx - 1] = 1 if ob[ny - 1, nx - 1] == 0 else 0
        assert lib.lbm_dbody_set(sim.ctx, bad.ctypes.data) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "y %d, x %d" % (y, x) in msg and "fluid" in msg, msg
        assert np.array_equal(sim.body(), b["a"]) and sim.force() == fa
        # upload_obstacles resets the body to the blocked cells
        sim.upload_obstacles(ob)
        assert np.array_equal(sim.body(), b["c"])
        other = ob.copy()
        other[ny // 2, nx - 2] = 1
        sim.set_body(b["a"])
        sim.upload_obstacles(other)
        assert np.array_equal(sim.body(), (other != 0).astype(np.int32))
        sim.upload_obstacles(ob)
        # with "force" on only before the first step
        sim.upload(cells0)
        sim.set_option("force", 1)
        sim.set_body(b["a"])
        sim.run(1)
        assert lib.lbm_dbody_set(sim.ctx, b["e"].ctypes.data) == LBM_ERR_STATE
        assert lib.lbm_dbody_set(sim.ctx, None) == LBM_ERR_STATE
        assert np.array_equal(sim.body(), b["a"])
        with pytest.raises(lbm.LBMError) as err:
            sim.set_body(b["e"])
        assert "code %d" % LBM_ERR_STATE in str(err.value)
        sim.upload(cells0)
        sim.set_body(b["e"])                                            # accepted again
        assert np.array_equal(sim.body(), b["e"])
    params = lbm.sweep_dparams(p, omega=[1.2, 1.7])
    with lbm.EnsembleDouble(params, ob) as ens:
        assert np.array_equal(ens.body(), np.stack([b["c"]] * 2))
        ens.set_body(b["a"])                                            # one map for all members
        assert np.array_equal(ens.body(), np.stack([b["a"]] * 2))
        ens.upload(None)                                                # keeps it
        assert np.array_equal(ens.body(), np.stack([b["a"]] * 2))
        ens.run(1)
        ens.set_body(np.stack([b["a"], b["e"]]))                        # "force" off: any time
        bad = np.stack([b["a"], b["e"]])
        bad[1, y, x] = 3
        assert lib.lbm_dbody_ens_set(ens.ens, bad.ctypes.data) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "member 1, y %d, x %d" % (y, x) in msg, msg
        assert np.array_equal(ens.body(), np.stack([b["a"], b["e"]]))
        ens.upload(None)
        ens.set_option("force", 1)
        ens.run(1)
        assert lib.lbm_dbody_ens_set(ens.ens, None) == LBM_ERR_STATE
        assert np.array_equal(ens.body(), np.stack([b["a"], b["e"]]))
        ens.upload(None)
        ens.set_body(None)
        assert np.array_equal(ens.body(), np.stack([b["c"]] * 2))


# ---- 6. drag criterion -------------------------------------------------------------------------------------------------


def drag_ensemble(lbm, nx, ny, body):
    params, ob = sweep(lbm, nx, ny, OMEGAS[4], max_iters=CAP)
    ens = lbm.EnsembleDouble(params, ob)
    ens.set_option("force", 1)
    ens.set_body(body)
    ens.upload(None)
    return ens


def drag_snapshot(ens):
    cells, av = ens.download()
    fx, fy = ens.force_record()
    return {"cells": cells, "av": av, "fx": fx, "fy": fy, "fields": ens.final_state()}


_plain = {}


def plain_at(lbm, nx, ny, c):
    """a fresh ensemble with the body and the record, advanced to c by ONE run(c); computed once per (grid, c)"""
    if (nx, ny, c) not in _plain:
        with drag_ensemble(lbm, nx, ny, block_body(nx, ny)) as ens:
            ens.run(c)
            _plain[(nx, ny, c)] = drag_snapshot(ens)
    return _plain[(nx, ny, c)]


@pytest.mark.parametrize("nx,ny,window", [(48, 32, 7), (48, 32, 16), (37, 29, 16)])
def test_run_until_on_drag_stops_every_member_where_the_rule_says(lbm, nx, ny, window):
    body = block_body(nx, ny)
    whole = plain_at(lbm, nx, ny, CAP)
    assert whole["fx"].shape == (4, CAP) and np.all(np.isfinite(whole["fx"]))
    want_steps, want_conv = rule(whole["fx"], 0, CAP, window, TOL)
    av_steps, av_conv = rule(whole["av"], 0, CAP, window, TOL)
    print("%dx%d window %d: drag stops %s converged %s; av_vels stops %s" %
          (nx, ny, window, want_steps.tolist(), want_conv.astype(int).tolist(), av_steps.tolist()))
    # conditions on the input
    assert len(set(want_steps.tolist())) >= 2 and np.any(want_conv) and np.any(~want_conv)
    assert np.all(want_steps[~want_conv] == CAP)
    assert want_steps.tolist() != av_steps.tolist()          # the two criteria stop these members at different counts

    with drag_ensemble(lbm, nx, ny, body) as ens:
        steps, conv = ens.run_until(CAP, window=window, rel_tol=TOL, on="drag")
        assert steps.dtype == np.int32 and conv.dtype == bool
        assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
        again = ens.member_steps()
        assert again[0].tolist() == steps.tolist() and again[1].tolist() == conv.tolist()
        assert ens.steps_done == int(want_steps.max())
        got = drag_snapshot(ens)
        # the same ensemble on its av_vels record: where the existing rule says, unchanged
        ens.upload(None)
        steps_av, conv_av = ens.run_until(CAP, window=window, rel_tol=TOL, on="av_vels")
        assert steps_av.tolist() == av_steps.tolist() and conv_av.tolist() == av_conv.tolist()
        ens.upload(None)
        steps_default, _ = ens.run_until(CAP, window=window, rel_tol=TOL)
        assert steps_default.tolist() == av_steps.tolist()
    for m in range(4):
        c = int(steps[m])
        ref = plain_at(lbm, nx, ny, c)
        what = "member %d stopped at %d" % (m, c)
        assert np.array_equal(got["cells"][m], ref["cells"][m]), what
        for key in ("av", "fx", "fy"):
            assert np.array_equal(got[key][m, :c], ref[key][m, :c]), (what, key)
            assert np.array_equal(got[key][m, :c], whole[key][m, :c]), (what, key)
        for key in ("fx", "fy"):
            assert plus_zero(got[key][m, c:]), (what, key)
        for x, y in zip(got["fields"], ref["fields"]):
            assert np.array_equal(x[m], y[m]), what


def test_drag_criterion_needs_the_record_and_an_empty_body_stops_at_once(lbm):
    nx, ny, window = 37, 29, 7
    params, ob = sweep(lbm, nx, ny, OMEGAS[4], max_iters=CAP)
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.set_body(block_body(nx, ny))
        ens.upload(None)
        with pytest.raises(lbm.LBMError) as err:
            ens.run_until(CAP, window=window, rel_tol=TOL, on="drag")
        assert "code %d" % LBM_ERR_STATE in str(err.value) and "before the first step" in str(err.value)
        assert ens.steps_done == 0
        with pytest.raises(ValueError):
            ens.run_until(CAP, window=window, rel_tol=TOL, on="lift")
        assert ens.steps_done == 0
    with drag_ensemble(lbm, nx, ny, np.zeros((ny, nx), dtype=np.int32)) as ens:
        steps, conv = ens.run_until(CAP, window=window, rel_tol=TOL, on="drag")
        assert steps.tolist() == [2 * window] * 4 and conv.all()         # the first check point with an entry one window back
        fx, fy = ens.force_record()
        assert fx.shape == (4, 2 * window) and plus_zero(fx) and plus_zero(fy)
        ens.run(3)                                                       # all at one count: an ordinary ensemble again
        assert ens.steps_done == 2 * window + 3

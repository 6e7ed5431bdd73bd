"""Drag and lift on the GPU: the momentum-exchange force on the blocked cells (option "force", lbm_dforce_*,
LBMDouble / EnsembleDouble .force() and .force_record()).

The reference value is tests/_force_ref.py's `restatement`: include/lbm.h's definition in numpy float64, np.roll per speed over the
mask, evaluated on states downloaded from the GPU and accelerated with the fp64 oracle's accelerate_flow; the masks, cases and
single-step states are that module's too.  Gates:
  1. record against the restatement, per component 8 L 2^-53 sum|link terms| (L links): four times the bound between two
     summation orders of the same terms; a missing or doubled link is 1e-3 to 1e-2 of the total, ten orders above it;
  2. momentum balance, independent of the restatement: fluid momentum after step t minus fluid momentum of the accelerated
     state before it equals -F[t] within 2 9N 2^-53 sum|f| (N cells);
  3. - 8. bit identity (np.array_equal) and error codes: no tolerance.
Masks: a partial wall, a 4x5 block, 3 % random cells, a blocked cell at x = 0 facing fluid at x = nx-1 across the wrap and the
same in y, blocked cells on rows ny-1, ny-2, ny-3 with fluid beside them on ny-2, an isolated blocked cell, a blocked cell with
all eight neighbours blocked, blocked cells at x = 15 | 16 and y = 15 | 16 (tile seams)."""
import numpy as np
import pytest

from _dp_states import CASES, RUNS, make_members
from _force_ref import SHAPES, SINGLE_STEPS, U, accelerated, case, fluid_momentum, force_mask, restatement, single_steps
from _steady_rule import OMEGAS, TOL, sweep

pytestmark = pytest.mark.gpu

LBM_ERR_ARG, LBM_ERR_STATE = 1, 3


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def test_masks_hold_what_they_promise():
    for nx, ny in SHAPES[:-1]:
        ob = force_mask(nx, ny) != 0
        assert ob[ny // 2, 0] and not ob[ny // 2, nx - 1]                        # wrap in x
        assert ob[0, 1] and not ob[ny - 1, 1]                                    # wrap in y
        assert ob[ny - 1, nx // 2] and ob[ny - 2, nx // 2 + 1] and ob[ny - 3, nx // 2] and not ob[ny - 2, nx // 2]
        if nx >= 16 and ny >= 12:
            y, x = ny - 7, nx - 5
            assert ob[y, x] and np.count_nonzero(ob[y - 1:y + 2, x - 1:x + 2]) == 1
            assert np.all(ob[3:6, nx - 7:nx - 4])
        if nx > 16 and ny > 19:
            assert ob[15, 15] and ob[15, 16] and ob[16, 15] and ob[16, 16]


# ---- 1. record against the restatement, 2. momentum balance --------------------------------------------------------------

@pytest.mark.parametrize("multistep", [0, 3, 8])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_record_equals_the_restatement(lbm, oracle_f64, nx, ny, multistep):
    p, ob, states, fx, fy = single_steps(lbm, nx, ny, multistep)
    worst = 0.0
    for t in range(SINGLE_STEPS):
        rx, ry, links, mag = restatement(accelerated(oracle_f64, p, ob, states[t]), ob)
        tol = 8.0 * links * U * mag
        assert links > 0 and mag > 0.0
        worst = max(worst, abs(fx[t] - rx) / tol, abs(fy[t] - ry) / tol)
        print("%dx%d multistep %d step %d: F = (%.6e, %.6e)  |dFx| %.2e |dFy| %.2e  tol %.2e  links %d" %
              (nx, ny, multistep, t, fx[t], fy[t], abs(fx[t] - rx), abs(fy[t] - ry), tol, links))
        assert abs(fx[t] - rx) <= tol and abs(fy[t] - ry) <= tol, (t, fx[t], rx, fy[t], ry, tol)
    # the forces are not trivially small: a missing link would show
    assert max(np.max(np.abs(fx)), np.max(np.abs(fy))) > 1e-4, (fx, fy, worst)


@pytest.mark.parametrize("multistep", [0, 3, 8])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_momentum_balance(lbm, oracle_f64, nx, ny, multistep):
    p, ob, states, fx, fy = single_steps(lbm, nx, ny, multistep)
    for t in range(SINGLE_STEPS):
        before = accelerated(oracle_f64, p, ob, states[t])
        after = states[t + 1]
        tol = 2.0 * 9 * nx * ny * U * float(np.sum(np.abs(before)))
        bx, by = fluid_momentum(before, ob)
        ax, ay = fluid_momentum(after, ob)
        print("%dx%d multistep %d step %d: residual (%.2e, %.2e)  tol %.2e" %
              (nx, ny, multistep, t, abs(ax - bx + fx[t]), abs(ay - by + fy[t]), tol))
        assert abs((ax - bx) + fx[t]) <= tol and abs((ay - by) + fy[t]) <= tol, (t, ax - bx, fx[t], ay - by, fy[t], tol)


# ---- 3. bit identity ---------------------------------------------------------------------------------------------------

def record_of(lbm, p, ob, cells0, multistep, runs):
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_option("multistep", multistep)
        sim.set_option("force", 1)
        sim.upload(cells0)
        for r in runs:
            sim.run(r)
        return sim.force_record()


@pytest.mark.parametrize("nx,ny", [(33, 19), (48, 35), (128, 128)])
def test_record_is_bit_identical_between_forms_splits_and_runs(lbm, nx, ny):
    steps = sum(RUNS)
    p, ob, cells0 = case(lbm, nx, ny, steps)
    ref = record_of(lbm, p, ob, cells0, 0, [steps])
    assert ref[0].shape == (steps,) and np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1]))
    for multistep in (0, 3, 8, -1):
        for runs in ([steps], RUNS):
            got = record_of(lbm, p, ob, cells0, multistep, runs)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (multistep, len(runs))
    again = record_of(lbm, p, ob, cells0, 8, RUNS)
    assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])


# ---- 4. force() equals the record ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("multistep", [0, 8])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_force_equals_the_record_entry_of_the_next_step(lbm, nx, ny, multistep):
    p, ob, cells0 = case(lbm, nx, ny, 16)
    with lbm.LBMDouble(p, ob) as sim, lbm.LBMDouble(p, ob) as off:
        sim.set_option("multistep", multistep)
        sim.set_option("force", 1)
        off.set_option("multistep", multistep)
        sim.upload(cells0)
        off.upload(cells0)
        now = []
        for advance in (0, 1, 5, 3):
            sim.run(advance)
            off.run(advance)
            before = sim.download(av_vels=False)[0]
            now.append((sim.steps_done, sim.force()))
            assert np.array_equal(sim.download(av_vels=False)[0], before)       # the state is not modified
            assert off.force() == now[-1][1]                                    # with or without the option
        sim.run(1)
        fx, fy = sim.force_record()
    for t, (gx, gy) in now:
        assert gx == fx[t] and gy == fy[t], (t, gx, fx[t], gy, fy[t])
        assert np.signbit(gx) == np.signbit(fx[t]) and np.signbit(gy) == np.signbit(fy[t])


# ---- 5. ensemble members -----------------------------------------------------------------------------------------------

ENS_RUNS = RUNS[:10] + [20]      # 1, 1, 9, 2..8, 20: launches of every depth, two-launch splits and a tail, 66 steps


@pytest.mark.parametrize("name", list(CASES))
def test_members_equal_dp_contexts_bit_for_bit(lbm, name):
    nx, ny, n, masks = CASES[name]
    steps = sum(ENS_RUNS)
    params, obs, cells0 = make_members(lbm, nx, ny, n, 1000 * nx + ny, max_iters=steps, masks=masks)
    with np.errstate(all="ignore"):
        with lbm.EnsembleDouble(params, obs) as ens:
            ens.set_option("force", 1)
            assert ens.get_option("force") == 1
            ens.upload(cells0)
            for r in ENS_RUNS[:-1]:
                ens.run(r)
            mid = ens.force()
            ens.run(ENS_RUNS[-1])
            efx, efy = ens.force_record()
            end = ens.force()
        assert efx.shape == efy.shape == (n, steps) and mid[0].shape == (n,)
        for k in range(n):
            with lbm.LBMDouble(params[k], obs[k]) as sim:
                sim.set_option("force", 1)
                sim.upload(cells0[k])
                sim.run(steps - ENS_RUNS[-1])
                assert sim.force() == (mid[0][k], mid[1][k]), (name, k)
                sim.run(ENS_RUNS[-1])
                fx, fy = sim.force_record()
                assert sim.force() == (end[0][k], end[1][k]), (name, k)
            assert np.array_equal(efx[k], fx) and np.array_equal(efy[k], fy), (name, k)
            if not np.any(obs[k]) or np.all(obs[k]):
                for v in (efx[k], efy[k], mid[0][k], mid[1][k], end[0][k], end[1][k]):
                    assert np.all(v == 0.0) and not np.any(np.signbit(v)), (name, k)       # exactly +0.0
            elif name != "3x3":
                assert np.any(efx[k] != 0.0) and np.any(efy[k] != 0.0), (name, k)
    if "blocked" in name:
        assert np.all(obs[1]) and not np.any(obs[2])       # the all-blocked and the all-free member were there


# ---- 6. steady run -----------------------------------------------------------------------------------------------------

def test_steady_run_records_every_member_up_to_its_own_count(lbm):
    nx, ny, window, cap = 64, 48, 16, 400
    omegas = OMEGAS[24][::3]
    assert len(omegas) == 8
    params, ob = sweep(lbm, nx, ny, omegas, max_iters=cap)
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.set_option("force", 1)
        ens.upload(None)
        steps, conv = ens.run_until(cap, window=window, rel_tol=TOL)
        efx, efy = ens.force_record()
        now = ens.force()
        _, av = ens.download(cells=False)
    print("stops", steps.tolist(), conv.tolist())
    assert len(set(steps.tolist())) > 1 and np.any(conv)             # the members stopped at different counts
    assert efx.shape == efy.shape == (8, int(steps.max()))
    for m in range(8):
        c = int(steps[m])
        with lbm.LBMDouble(params[m], ob) as sim:
            sim.set_option("force", 1)
            sim.upload(None)
            sim.run(c)
            fx, fy = sim.force_record()
            assert sim.force() == (now[0][m], now[1][m]), m
            assert np.array_equal(sim.download(cells=False)[1], av[m, :c])
        assert np.array_equal(efx[m, :c], fx) and np.array_equal(efy[m, :c], fy), m
        for tail in (efx[m, c:], efy[m, c:]):
            assert np.all(tail == 0.0) and not np.any(np.signbit(tail)), m       # +0.0 beyond its own count
        assert np.any(fx != 0.0)


# ---- 7. nothing else moves ---------------------------------------------------------------------------------------------

def snapshot(sim):
    cells, av = sim.download()
    return [cells, av] + list(sim.final_state()) + [sim.reynolds()]


@pytest.mark.parametrize("multistep", [0, 8])
def test_context_computes_the_same_with_the_option_on(lbm, multistep):
    p, ob, cells0 = case(lbm, 48, 35, 40)
    snaps = []
    for on in (0, 1):
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("multistep", multistep)
            sim.set_option("force", on)
            sim.upload(cells0)
            for r in (1, 9, 30):
                sim.run(r)
            snaps.append(snapshot(sim))
    for a, b in zip(*snaps):
        assert np.array_equal(a, b)


def test_ensemble_computes_the_same_with_the_option_on(lbm):
    nx, ny, n, masks = CASES["all-blocked and all-free members 64x48"]
    params, obs, cells0 = make_members(lbm, nx, ny, n, 5, max_iters=64, masks=masks)
    snaps, stops = [], []
    with np.errstate(all="ignore"):
        for on in (0, 1):
            with lbm.EnsembleDouble(params, obs) as ens:
                ens.set_option("force", on)
                ens.upload(cells0)
                ens.run(8)
                stops.append(ens.run_until(56, window=8, rel_tol=5e-2)[0])
                snaps.append(snapshot(ens))
    assert np.array_equal(stops[0], stops[1])
    for a, b in zip(*snaps):
        assert np.array_equal(a, b, equal_nan=True)


# ---- 8. errors ---------------------------------------------------------------------------------------------------------

def test_errors(lbm):
    lib = lbm.load_library()
    p, ob, cells0 = case(lbm, 16, 16, 8)
    buf = np.zeros(8)
    with lbm.LBMDouble(p, ob) as sim:
        assert sim.get_option("force") == 0
        sim.upload(cells0)
        sim.run(1)
        assert lib.lbm_dforce_record(sim.ctx, buf.ctypes.data, buf.ctypes.data) == LBM_ERR_STATE      # the option is off
        assert b"force" in lib.lbm_last_error()
        assert lib.lbm_dp_set_option(sim.ctx, b"force", 1) == LBM_ERR_STATE                           # after a step
        assert sim.get_option("force") == 0
        with pytest.raises(lbm.LBMError):
            sim.force_record()
        sim.upload(cells0)                                                                            # accepted again
        sim.set_option("force", 1)
        assert lib.lbm_dp_set_option(sim.ctx, b"force", 2) == LBM_ERR_ARG
        assert lib.lbm_dp_set_option(sim.ctx, b"forces", 1) == LBM_ERR_ARG
        sim.run(2)
        assert lib.lbm_dp_set_option(sim.ctx, b"force", 0) == LBM_ERR_STATE
        fx, fy = sim.force_record()
        assert fx.shape == (2,)
        only = np.zeros(2)
        assert lib.lbm_dforce_record(sim.ctx, None, only.ctypes.data) == 0 and np.array_equal(only, fy)
        assert lib.lbm_dforce_record(sim.ctx, None, None) == LBM_ERR_ARG
        sim.upload(cells0)
        sim.set_option("force", 0)                                                                    # and off again
        sim.run(1)
        with pytest.raises(lbm.LBMError):
            sim.force_record()
    params = lbm.sweep_dparams(p, omega=[1.2, 1.7])
    with lbm.EnsembleDouble(params, ob) as ens:
        assert ens.get_option("force") == 0
        ens.upload(None)
        ens.run(1)
        assert lib.lbm_dforce_ens_record(ens.ens, buf.ctypes.data, buf.ctypes.data) == LBM_ERR_STATE
        assert lib.lbm_dforce_ens_set_option(ens.ens, b"force", 1) == LBM_ERR_STATE
        v = __import__("ctypes").c_long()
        assert lib.lbm_dforce_ens_set_option(ens.ens, b"multistep", 1) == LBM_ERR_ARG
        assert lib.lbm_dforce_ens_get_option(ens.ens, b"multistep", __import__("ctypes").byref(v)) == LBM_ERR_ARG
        fx, fy = ens.force()                                                                          # needs no option
        assert fx.shape == (2,) and np.all(np.isfinite(fx))
        ens.upload(None)
        ens.set_option("force", 1)
        ens.run(3)
        assert ens.force_record()[0].shape == (2, 3)
        assert lib.lbm_dforce_ens(ens.ens, None, None) == LBM_ERR_ARG

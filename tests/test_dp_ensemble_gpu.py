"""Double-precision ensembles on the GPU (lbm_dens_*, lbm_amd.EnsembleDouble).

No tolerance is invented here: every gate is bit-identity to existing code, or a gate tests/test_dp_gpu.py states.
  1. every member equals, bit for bit, an LBMDouble on the same inputs (cells, av_vels, the four fields, the Reynolds number),
     at the LBMDouble's default form and at one step per launch, after 1, 2, 11 and 1000 cumulative steps reached by runs that
     give launches of every depth and a tail;
  2. full-length runs of the shipped 128x128 and 128x256 inputs as member 0 of a sweep against the golden files, at
     test_dp_gpu.py's gates;
  3. members are independent of their neighbours and of the ensemble's size; identical runs give identical bits;
  4. an fp32 Ensemble and an LBMDouble interleaved with an EnsembleDouble compute what they compute alone;
  5. state errors."""
import numpy as np
import pytest

from conftest import golden_cols, input_files
from _dp_states import (CASES, CHECKPOINTS, FULL, PRINT_PRECISION_PCNT, RE_REL, RUNS, VEL_ABS, make_members, max_pcnt,
                        reynolds_ref)

pytestmark = pytest.mark.gpu

LBM_ERR_STATE = 3


def same(a, b):
    """bit-identical values; a NaN in both at the same place (av_vels and Reynolds number of a member without a free cell:
    0 * inf) counts equal, as in max_abs of test_dp_gpu.py"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def snapshot(sim):
    cells, av = sim.download()
    return cells, av, sim.final_state(), sim.reynolds()


def track(sim, cells0, runs=RUNS, checkpoints=CHECKPOINTS):
    """snapshots of `sim` at each checkpoint, reached through `runs`"""
    sim.upload(cells0)
    out, done = [], 0
    with np.errstate(all="ignore"):
        for r in runs:
            sim.run(r)
            done += r
            if done in checkpoints:
                assert sim.steps_done == done
                out.append(snapshot(sim))
    assert len(out) == len(checkpoints)
    return out


def assert_member_equals(ens_snap, k, ref_snap, what):
    ec, eav, ef, ere = ens_snap
    rc, rav, rf, rre = ref_snap
    assert ec[k].shape == rc.shape and eav[k].shape == rav.shape
    assert same(ec[k], rc), what + ": cells"
    assert same(eav[k], rav), what + ": av_vels"
    for name, a, b in zip(("u_x", "u_y", "u", "pressure"), ef, rf):
        assert same(a[k], b), what + ": " + name
    assert same(ere[k], rre), what + ": Reynolds number"


# ---- 1. members equal double-precision contexts, bit for bit -----------------------------------------------------------


@pytest.mark.parametrize("name", list(CASES))
def test_members_equal_dp_contexts_bit_for_bit(lbm, name):
    nx, ny, n, masks = CASES[name]
    params, obs, cells0 = make_members(lbm, nx, ny, n, 1000 * nx + ny, masks=masks)
    with lbm.EnsembleDouble(params, obs) as ens:
        got = track(ens, cells0)
    assert got[-1][1].shape == (n, CHECKPOINTS[-1])
    if "blocked" not in name and name != "3x3":
        assert np.all(np.isfinite(got[-1][0])) and np.all(got[-1][1] > 0.0)
    for k in range(n):
        for multistep in (-1, 0):       # the LBMDouble at its default form (LDS tiles on these sizes) and at one step per launch
            with lbm.LBMDouble(params[k], obs[k]) as sim:
                sim.set_option("multistep", multistep)
                ref = track(sim, cells0[k])
            for steps, e, r in zip(CHECKPOINTS, got, ref):
                assert_member_equals(e, k, r, "%s member %d after %d steps, multistep %d" % (name, k, steps, multistep))


# ---- 2. golden files, full length ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", ["128x128", "128x256"])
def test_full_length_golden_member(lbm, size):
    p, ob = lbm.read_inputs_double(*input_files(size))
    assert p.max_iters == FULL[size]       # the shipped length: the run is not shortened
    members = lbm.sweep_dparams(p, omega=[p.omega, 1.0, 1.4, 1.7])
    assert members[0].omega == p.omega and members[0].max_iters == FULL[size]
    with lbm.EnsembleDouble(members, ob) as ens:
        ens.upload(None)
        ens.run(p.max_iters)
        assert ens.steps_done == FULL[size]
        _, av = ens.download(cells=False)
        ux, uy, u, pr = (f[0] for f in ens.final_state())
        re = ens.reynolds()
    assert av.shape == (4, FULL[size]) and np.all(np.isfinite(av)) and np.all(np.isfinite(re))
    e_av = max_pcnt(golden_cols("%s.av_vels.dat" % size, [1]), av[0])
    ref = golden_cols("%s.final_state.dat" % size, [2, 3, 4, 5, 6])
    e_pr = max_pcnt(ref[:, 3].reshape(p.ny, p.nx), pr)
    e_vel = [float(np.max(np.abs(ref[:, i].reshape(p.ny, p.nx) - got))) for i, got in enumerate((ux, uy, u))]
    e_re = abs(re[0] / reynolds_ref(size) - 1.0)
    print("%s member 0: av_vels %.3e %%  pressure %.3e %%  u_x/u_y/u %.3e %.3e %.3e  Re %.3e" %
          ((size, e_av, e_pr) + tuple(e_vel) + (e_re,)))
    assert e_av < PRINT_PRECISION_PCNT
    assert e_pr < PRINT_PRECISION_PCNT
    assert max(e_vel) <= VEL_ABS
    assert e_re < RE_REL
    # the sweep did something: another omega, another flow
    assert not np.array_equal(av[0], av[1])


# ---- 3. members are independent -----------------------------------------------------------------------------------------

def test_members_are_independent_of_the_ensemble(lbm):
    n, steps, runs = 9, 50, [1, 5, 44]
    params, obs, cells0 = make_members(lbm, 128, 128, n, 77, max_iters=steps)
    with lbm.EnsembleDouble(params, obs) as ens:
        whole = track(ens, cells0, runs, [steps])[0]
    with lbm.EnsembleDouble(params, obs) as ens:
        again = track(ens, cells0, runs, [steps])[0]
    assert same(whole[0], again[0]) and same(whole[1], again[1]) and same(whole[3], again[3])
    assert all(same(a, b) for a, b in zip(whole[2], again[2]))
    for k in (0, n // 2, n - 1):
        with lbm.EnsembleDouble([params[k]], obs[k:k + 1]) as one:
            assert one.n == 1
            single = track(one, cells0[k:k + 1], runs, [steps])[0]
        assert same(whole[0][k], single[0][0]) and same(whole[1][k], single[1][0]), k
        assert all(same(a[k], b[0]) for a, b in zip(whole[2], single[2])), k
        assert same(whole[3][k], single[3][0]), k


# ---- 4. beside other contexts -------------------------------------------------------------------------------------------

def test_other_contexts_unaffected_by_dp_ensemble(lbm):
    steps, rounds = 50, 4
    p32, ob = lbm.read_inputs(*input_files("128x128"))
    p32.max_iters = steps * rounds
    members32 = lbm.sweep_params(p32, omega=[1.2, 1.5, float(p32.omega)])
    pdp, _ = lbm.read_inputs_double(*input_files("128x128"))
    pdp.max_iters = steps * rounds
    members64 = lbm.sweep_dparams(pdp, omega=[pdp.omega, 1.3, 1.6, 1.1])

    def run_rounds(*sims):
        for s in sims:
            s.upload(None)
        for _ in range(rounds):      # the same runs alone and beside: an fp32 record depends on how a run is cut into launches
            for s in sims:
                s.run(steps)
        for s in sims:
            s.sync()
        return [snapshot(s) for s in sims]

    with lbm.Ensemble(members32, ob) as e32:
        alone32, = run_rounds(e32)
    with lbm.LBMDouble(pdp, ob) as dp:
        alone_dp, = run_rounds(dp)
    with lbm.EnsembleDouble(members64, ob) as e64:
        alone64, = run_rounds(e64)
    with lbm.EnsembleDouble(members64, ob) as e64, lbm.Ensemble(members32, ob) as e32, lbm.LBMDouble(pdp, ob) as dp:
        beside64, beside32, beside_dp = run_rounds(e64, e32, dp)
    for alone, beside in ((alone32, beside32), (alone_dp, beside_dp), (alone64, beside64)):
        assert same(alone[0], beside[0]) and same(alone[1], beside[1]) and same(alone[3], beside[3])
        assert all(same(a, b) for a, b in zip(alone[2], beside[2]))
    # and member 0 of the double ensemble is the double context
    assert_member_equals(beside64, 0, beside_dp, "member 0 beside the context")


# ---- 5. state errors ----------------------------------------------------------------------------------------------------

def test_state_errors(lbm):
    params, obs, cells0 = make_members(lbm, 32, 24, 3, 5, max_iters=10)
    lib = lbm.load_library()
    with lbm.EnsembleDouble(params, obs) as ens:
        assert lib.lbm_dens_members(ens.ens) == 3
        ens.upload(cells0)
        ens.run(7)
        assert lib.lbm_dens_run(ens.ens, 4) == LBM_ERR_STATE       # 7 + 4 > max_iters
        assert b"max_iters" in lib.lbm_last_error()
        with pytest.raises(lbm.LBMError):
            ens.run(4)
        with pytest.raises(lbm.LBMError):
            ens.run(-1)
        assert ens.steps_done == 7
        ens.run(3)                                                  # still usable
        assert ens.steps_done == 10
        first = snapshot(ens)
        assert first[1].shape == (3, 10)
        ens.upload(cells0)                                          # resets the step counter
        assert ens.steps_done == 0
        _, av = ens.download(cells=False)
        assert av.shape == (3, 0)
        ens.run(10)
        second = snapshot(ens)
        assert same(first[0], second[0]) and same(first[1], second[1]) and same(first[3], second[3])

"""The two-relaxation-time collision on the GPU (lbm_dtrt_*, LBMDouble / EnsembleDouble .set_trt() and .trt()).

The reference is tests/_trt_ref.py: include/lbm.h's statements in numpy float64, held to the fp64 oracle in BGK mode by
tests/test_trt_restatement_cpu.py.  Gates:
  1. cells after a step against the restatement of the state before it (downloaded, accelerated with the fp64 oracle's
     accelerate_flow): np.array_equal.  av_vels against the restatement's sum|u| * free_cells_inv within N 2^-53 sum|u|, the bound
     between two summation orders of N terms;
  2. - 5. bit identity (np.array_equal) and stop counts: no tolerance;
  6. error codes; 7. mass drift within test_dp_gpu's MASS_REL.
Inputs: test_force_gpu's shapes 3x3 (wraps), 16x16 (one tile), 33x19 (ragged tiles and seams), 48x35 (3x3 tiles) with its
force_mask; density 0.1, accel 0.005, omega 1.7, Lambda 3/16, states from random_state."""
import ctypes
import math

import numpy as np
import pytest

import _trt_ref
from _dp_states import MASS_REL, RUNS, random_state
from _force_ref import accelerated, block_body, case, force_mask
from _steady_rule import CAP, OMEGAS, TOL, rule, sweep

pytestmark = pytest.mark.gpu

LBM_ERR_ARG, LBM_ERR_STATE = 1, 3
U = 2.0 ** -53
SHAPES = [(3, 3), (16, 16), (33, 19), (48, 35)]
MAGIC = 3.0 / 16.0
SINGLE_STEPS = 12
ENS_OMEGAS = [float(v) for v in np.linspace(1.0, 1.85, 5)]
ENS_MAGICS = [3.0 / 16.0, 1.0 / 4.0, 1.0 / 12.0, 1.0 / 6.0, 3.0 / 16.0]
ENS_RUNS = RUNS[:10] + [20]      # 1, 1, 9, 2..8, 20: launches of every depth, two-launch splits and a tail, 66 steps


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


# ---- 1. single steps against the restatement ---------------------------------------------------------------------------

_single = {}


def single_steps(lbm, nx, ny, multistep):
    """12 steps one at a time: the state before each step and after the last, and av_vels.  Computed once per case."""
    key = (nx, ny, multistep)
    if key not in _single:
        p, ob, cells0 = case(lbm, nx, ny, SINGLE_STEPS)
        states = []
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("multistep", multistep)
            sim.set_trt(MAGIC)
            sim.upload(cells0)
            for _ in range(SINGLE_STEPS):
                states.append(sim.download(av_vels=False)[0])
                sim.run(1)
            cells, av = sim.download()
            states.append(cells)
        _single[key] = (p, ob, states, av)
    return _single[key]


@pytest.mark.parametrize("multistep", [0, 3, 8])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_single_steps_equal_the_restatement_bit_for_bit(lbm, oracle_f64, nx, ny, multistep):
    p, ob, states, av = single_steps(lbm, nx, ny, multistep)
    assert p.omega == 1.7 and av.shape == (SINGLE_STEPS,)
    om = _trt_ref.omega_minus(p.omega, MAGIC)
    apart = 0.0
    for t in range(SINGLE_STEPS):
        f = accelerated(oracle_f64, p, ob, states[t])
        want, u = _trt_ref.step(f, ob, p.omega, om)
        differs = int(np.count_nonzero(want != states[t + 1]))
        total = float(np.sum(u))
        err, tol = abs(av[t] - total * p.free_cells_inv), nx * ny * U * total
        print("%dx%d multistep %d step %d: %d values differ; av_vels %.17e  |d| %.2e  tol %.2e" %
              (nx, ny, multistep, t, differs, av[t], err, tol))
        assert np.array_equal(states[t + 1], want), (t, differs)
        assert total > 0.0 and err <= tol, (t, av[t], total * p.free_cells_inv, tol)
        bgk, _ = _trt_ref.step(f, ob, p.omega)
        apart = max(apart, float(np.max(np.abs(want - bgk) / np.abs(bgk))))
    print("%dx%d: the TRT step is up to %.1f %% from the BGK step of the same state" % (nx, ny, 100.0 * apart))
    assert apart > 1e-3            # another operator, not BGK under a new name


# ---- 2. forms, launch splits, runs -------------------------------------------------------------------------------------

def run_of(lbm, p, ob, cells0, multistep, runs, magic=MAGIC):
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_option("multistep", multistep)
        sim.set_option("force", 1)
        sim.set_trt(magic)
        sim.upload(cells0)
        for r in runs:
            sim.run(r)
        return sim.download() + sim.force_record()


@pytest.mark.parametrize("nx,ny", SHAPES[1:])
def test_bit_identical_between_forms_splits_and_runs(lbm, nx, ny):
    steps = sum(RUNS)
    p, ob, cells0 = case(lbm, nx, ny, steps)
    ref = run_of(lbm, p, ob, cells0, 0, [steps])
    assert ref[1].shape == (steps,) and all(np.all(np.isfinite(v)) for v in ref)
    for multistep in (0, 3, 8):
        for runs in ([steps], RUNS):
            got = run_of(lbm, p, ob, cells0, multistep, runs)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)), (multistep, len(runs))
    again = run_of(lbm, p, ob, cells0, 8, RUNS)
    assert all(np.array_equal(a, b) for a, b in zip(again, ref))
    bgk = run_of(lbm, p, ob, cells0, 8, RUNS, magic=0.0)
    assert not np.array_equal(bgk[0], ref[0]) and not np.array_equal(bgk[1], ref[1])


# ---- 3. ensemble members -----------------------------------------------------------------------------------------------

def snapshot(sim):
    cells, av = sim.download()
    return [cells, av] + list(sim.final_state()) + [sim.reynolds()] + list(sim.force_record()) + list(sim.force())


@pytest.mark.parametrize("nx,ny", [(33, 19), (48, 35)])
def test_members_equal_dp_contexts_bit_for_bit(lbm, nx, ny):
    n, steps = len(ENS_OMEGAS), sum(ENS_RUNS)
    ob = force_mask(nx, ny)
    body = np.zeros_like(ob)
    body[ny // 2 - 2:ny // 2 + 2, nx // 4:nx // 4 + 5] = 1            # force_mask's 4x5 block, where it is still blocked
    body &= ob
    assert 16 <= np.count_nonzero(body) < np.count_nonzero(ob)
    base = lbm.make_dparams(nx, ny, steps, density=0.1, accel=0.005, omega=1.7, obstacles=ob)
    params = lbm.sweep_dparams(base, omega=ENS_OMEGAS)
    rng = np.random.default_rng(100 * nx + ny)
    cells0 = np.stack([random_state(rng, 0.1, ny, nx) for _ in range(n)])
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.set_option("force", 1)
        ens.set_body(body)
        ens.set_trt(ENS_MAGICS)
        magic, om = ens.trt()
        assert magic.tolist() == ENS_MAGICS
        assert om.tolist() == [_trt_ref.omega_minus(w, m) for w, m in zip(ENS_OMEGAS, ENS_MAGICS)]
        ens.upload(cells0)
        for r in ENS_RUNS:
            ens.run(r)
        got = snapshot(ens)
    assert np.all(np.isfinite(got[0])) and got[1].shape == (n, steps) and np.any(got[7] != 0.0)
    for k in range(n):
        with lbm.LBMDouble(params[k], ob) as sim:
            sim.set_option("force", 1)
            sim.set_body(body)
            sim.set_trt(ENS_MAGICS[k])
            sim.upload(cells0[k])
            sim.run(steps)
            ref = snapshot(sim)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert np.array_equal(a[k], b), (k, i)


# ---- 4. steady runs ----------------------------------------------------------------------------------------------------

STEADY_MAGICS = [3.0 / 16.0, 1.0 / 4.0, 1.0 / 12.0, 3.0 / 16.0]


def steady_ensemble(lbm, nx, ny):
    params, ob = sweep(lbm, nx, ny, OMEGAS[4], max_iters=CAP)
    ens = lbm.EnsembleDouble(params, ob)
    ens.set_option("force", 1)
    ens.set_body(block_body(nx, ny))
    ens.set_trt(STEADY_MAGICS)
    ens.upload(None)
    return ens, params, ob


@pytest.mark.parametrize("on", ["av_vels", "drag"])
def test_run_until_stops_every_member_where_the_rule_says(lbm, on):
    nx, ny, window = 48, 32, 7
    ens, params, ob = steady_ensemble(lbm, nx, ny)
    with ens:
        ens.run(CAP)
        whole = {"av": ens.download(cells=False)[1], "fx": ens.force_record()[0]}
        assert whole["av"].shape == (4, CAP) and np.all(np.isfinite(whole["av"])) and np.all(np.isfinite(whole["fx"]))
        # the stop decisions, on the host from the downloaded record
        want_steps, want_conv = rule(whole["av" if on == "av_vels" else "fx"], 0, CAP, window, TOL)
        print("TRT %dx%d window %d on %s: stops %s converged %s" % (nx, ny, window, on, want_steps.tolist(), want_conv.tolist()))
        assert np.any(want_conv) and len(set(want_steps.tolist())) >= 2
        ens.upload(None)
        steps, conv = ens.run_until(CAP, window=window, rel_tol=TOL, on=on)
        assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
        cells, av = ens.download()
        fx, fy = ens.force_record()
        fields, re, now = ens.final_state(), ens.reynolds(), ens.force()
    for m in range(4):
        c = int(steps[m])
        with lbm.LBMDouble(params[m], ob) as sim:
            sim.set_option("force", 1)
            sim.set_body(block_body(nx, ny))
            sim.set_trt(STEADY_MAGICS[m])
            sim.upload(None)
            sim.run(c)
            rc, rav = sim.download()
            rfx, rfy = sim.force_record()
            assert np.array_equal(cells[m], rc), m
            assert np.array_equal(av[m, :c], rav) and np.array_equal(av[m, :c], whole["av"][m, :c]), m
            assert np.array_equal(fx[m, :c], rfx) and np.array_equal(fy[m, :c], rfy), m
            assert all(np.array_equal(a[m], b) for a, b in zip(fields, sim.final_state())), m
            assert re[m] == sim.reynolds() and (now[0][m], now[1][m]) == sim.force(), m


# ---- 5. on and off again -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("multistep", [0, 8])
def test_set_and_unset_at_step_0_leaves_the_bgk_bits(lbm, multistep):
    p, ob, cells0 = case(lbm, 48, 35, 40)
    snaps = []
    for touch in (False, True):
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("multistep", multistep)
            sim.set_option("force", 1)
            if touch:
                sim.set_trt(MAGIC)
                assert sim.trt() == (MAGIC, _trt_ref.omega_minus(p.omega, MAGIC))
                sim.set_trt(0.0)
            assert sim.trt() == (0.0, p.omega)
            sim.upload(cells0)
            for r in (1, 9, 30):
                sim.run(r)
            snaps.append(sim.download() + sim.force_record())
    assert all(np.array_equal(a, b) for a, b in zip(*snaps))
    params = lbm.sweep_dparams(p, omega=[1.2, 1.7])
    snaps = []
    for touch in (False, True):
        with lbm.EnsembleDouble(params, ob) as ens:
            ens.set_option("force", 1)
            if touch:
                ens.set_trt(MAGIC)
                assert ens.trt()[0].tolist() == [MAGIC, MAGIC]
                ens.set_trt(None)
            magic, om = ens.trt()
            assert magic.tolist() == [0.0, 0.0] and om.tolist() == [1.2, 1.7]
            ens.upload(np.stack([cells0, cells0]))
            ens.run(40)
            snaps.append(ens.download() + ens.force_record())
    assert all(np.array_equal(a, b) for a, b in zip(*snaps))


# ---- 6. errors ---------------------------------------------------------------------------------------------------------

def test_errors_and_what_keeps_the_setting(lbm):
    lib = lbm.load_library()
    p, ob, cells0 = case(lbm, 16, 16, 8)
    om = _trt_ref.omega_minus(p.omega, MAGIC)
    magic_out, om_out = ctypes.c_double(), ctypes.c_double()
    with lbm.LBMDouble(p, ob) as sim:
        assert sim.trt() == (0.0, p.omega)                                            # the default: BGK, omega_minus is omega
        sim.upload(cells0)
        sim.run(1)
        bgk = sim.download(av_vels=False)[0]
        assert lib.lbm_dtrt_set(sim.ctx, MAGIC) == LBM_ERR_STATE                      # after a step
        assert sim.trt() == (0.0, p.omega)
        sim.upload(cells0)                                                            # accepted again
        sim.set_trt(MAGIC)
        assert sim.trt() == (MAGIC, om)
        assert lib.lbm_dtrt_get(sim.ctx, None, ctypes.byref(om_out)) == 0 and om_out.value == om
        assert lib.lbm_dtrt_get(sim.ctx, ctypes.byref(magic_out), None) == 0 and magic_out.value == MAGIC
        assert lib.lbm_dtrt_get(sim.ctx, None, None) == LBM_ERR_ARG
        assert b"magic_out" in lib.lbm_last_error() and b"omega_minus_out" in lib.lbm_last_error()
        for bad in (-0.25, float("nan"), float("inf")):
            assert lib.lbm_dtrt_set(sim.ctx, bad) == LBM_ERR_ARG
        assert sim.trt() == (MAGIC, om)
        sim.run(1)
        trt = sim.download(av_vels=False)[0]
        assert not np.array_equal(trt, bgk)
        assert lib.lbm_dtrt_set(sim.ctx, 0.0) == LBM_ERR_STATE
        sim.upload(cells0)                                                            # uploads keep the setting
        sim.upload_obstacles(ob)
        assert sim.trt() == (MAGIC, om)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], trt)
    p2 = lbm.make_dparams(16, 16, 8, omega=2.0, obstacles=ob)
    with lbm.LBMDouble(p2, ob) as sim:
        assert lib.lbm_dtrt_set(sim.ctx, MAGIC) == LBM_ERR_ARG                        # 1/omega - 1/2 <= 0
        assert b"omega" in lib.lbm_last_error()
        sim.set_trt(0.0)                                                              # BGK has no such limit
        assert sim.trt() == (0.0, 2.0)

    params = lbm.sweep_dparams(p, omega=[1.2, 1.7, 1.0])

    def magics(*v):
        return np.array(v, dtype=np.float64)

    with lbm.EnsembleDouble(params, ob) as ens:
        ens.set_trt(magics(MAGIC, 0.25, 1.0 / 12.0))
        before = ens.trt()
        for bad, member in ((magics(MAGIC, 0.0, 0.25), b"member 1"), (magics(MAGIC, 0.25, float("nan")), b"member 2"),
                            (magics(-1.0, 0.25, 0.25), b"member 0"), (magics(MAGIC, float("inf"), 0.25), b"member 1")):
            assert lib.lbm_dtrt_ens_set(ens.ens, bad.ctypes.data) == LBM_ERR_ARG
            assert member in lib.lbm_last_error(), lib.lbm_last_error()
        after = ens.trt()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert lib.lbm_dtrt_ens_get(ens.ens, None, None) == LBM_ERR_ARG
        ens.upload(np.stack([cells0] * 3))
        ens.run(2)
        cells = ens.download(av_vels=False)[0]
        assert lib.lbm_dtrt_ens_set(ens.ens, None) == LBM_ERR_STATE
        assert lib.lbm_dtrt_ens_set(ens.ens, magics(0.25, 0.25, 0.25).ctypes.data) == LBM_ERR_STATE
        ens.upload(np.stack([cells0] * 3))                                            # keeps the setting
        assert np.array_equal(ens.trt()[0], before[0])
        ens.run(2)
        assert np.array_equal(ens.download(av_vels=False)[0], cells)
    # nothing on the device changes after a refusal: the members run on as the contexts with the setting before it
    for k in range(3):
        with lbm.LBMDouble(params[k], ob) as sim:
            sim.set_trt(float(before[0][k]))
            sim.upload(cells0)
            sim.run(2)
            assert np.array_equal(sim.download(av_vels=False)[0], cells[k]), k
    params[1].omega = 2.0
    with lbm.EnsembleDouble(params, ob) as ens:
        assert lib.lbm_dtrt_ens_set(ens.ens, magics(MAGIC, MAGIC, MAGIC).ctypes.data) == LBM_ERR_ARG
        assert b"member 1" in lib.lbm_last_error() and b"omega" in lib.lbm_last_error()
        assert ens.trt()[0].tolist() == [0.0, 0.0, 0.0]


# ---- 7. mass -----------------------------------------------------------------------------------------------------------

def test_mass_is_conserved(lbm):
    p, ob, cells0 = case(lbm, 48, 35, 200)
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_trt(MAGIC)
        sim.upload(cells0)
        sim.run(200)
        cells, av = sim.download()
    assert np.all(np.isfinite(cells)) and np.all(cells > 0.0) and np.all(np.isfinite(av))
    rel = abs(math.fsum(cells.ravel().tolist()) / math.fsum(cells0.ravel().tolist()) - 1.0)
    print("48x35 after 200 TRT steps: total density relative error %.3e" % rel)
    assert rel <= MASS_REL

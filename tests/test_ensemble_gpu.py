"""Ensembles on the GPU (lbm_ens_*, lbm_amd.Ensemble): N independent grids advanced by one launch per (up to) eight steps.

The standing rule of the project holds member by member: the cells of every member are bit-identical to the same inputs
advanced by single steps in an ordinary context (which is itself checked against the oracle), av_vels agree up to the
summation order (the bound test_lds_multistep_equals_single_steps uses) and with the fp32 oracle to RTOL_AV."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, input_files
from test_gpu_parity import RTOL_AV, RTOL_CELLS, SINGLE, check_outputs, max_rel, oracle_params

pytestmark = pytest.mark.gpu

W = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float64).reshape(9, 1, 1)


def member_case(lbm, rng, nx, ny, max_iters, blocked=0.08):
    """one member: random obstacles, a perturbed positive state around its own density, its own omega and accel"""
    density = float(rng.uniform(0.08, 0.12))
    ob = (rng.random((ny, nx)) < blocked).astype(np.int32)
    cells = (W * density * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5))).astype(np.float32)
    p = lbm.make_params(nx, ny, max_iters, density=density, accel=float(rng.uniform(0.002, 0.01)),
                        omega=float(rng.uniform(1.0, 1.9)), obstacles=ob)
    if ob.all():
        p.free_cells_inv = 1.0
    return p, ob, cells


def build_members(lbm, seed, nx, ny, n, max_iters):
    rng = np.random.default_rng(seed)
    cases = [member_case(lbm, rng, nx, ny, max_iters, blocked=0.08 if nx * ny > 30 else 0.0) for _ in range(n)]
    return [c[0] for c in cases], np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])


def solo(lbm, p, ob, cells0, nsteps, options=SINGLE, fields=False):
    """the same member in an ordinary context, on single steps unless told otherwise"""
    with lbm.LBM(p, ob) as sim:
        for k, v in (options or {}).items():
            sim.set_option(k, v)
        sim.upload(cells0)
        sim.run(nsteps)
        cells, av = sim.download()
        if fields:
            return cells, av, sim.final_state(), sim.reynolds()
        return cells, av


def assert_av_close(av, av_ref, what):
    err, bound = float(np.max(np.abs(av - av_ref))), 2e-6 * float(np.max(np.abs(av_ref))) + 1e-12
    print("%s: av_vels max|d| %.3e (bound %.3e)" % (what, err, bound))
    assert err <= bound, what


# (nx, ny, members, steps): the shapes of test_lds_multistep_equals_single_steps (tiles that hang over the grid edge, regions
# that wrap around tiny grids several times), one member alone, more members than CUs (several rounds of tiles), step counts
# 1, 8 (one full launch), 21 (7 + 7 + 7) and 300 (more than the ring of partial sums holds: flushed mid-run)
CASES = [(128, 128, 7, 21), (128, 256, 3, 8), (256, 256, 4, 21), (33, 17, 5, 300), (100, 70, 2, 1), (3, 3, 9, 21),
         (512, 48, 2, 8), (130, 31, 1, 21), (64, 64, 300, 21), (128, 128, 7, 1), (100, 70, 2, 300), (5, 4, 3, 8)]


@pytest.mark.parametrize("nx,ny,n,nsteps", CASES)
def test_ensemble_equals_single_step_contexts(lbm, oracle_f32_omp, nx, ny, n, nsteps):
    params, obs, cells0 = build_members(lbm, 1000 + nx * 31 + ny + 7 * n + nsteps, nx, ny, n, nsteps)
    with lbm.Ensemble(params, obs) as ens:
        ens.upload(cells0)
        ens.run(nsteps)
        assert ens.steps_done == nsteps
        cells, av = ens.download()
        fields = ens.final_state()
        re = ens.reynolds()
    assert cells.shape == (n, 9, ny, nx) and av.shape == (n, nsteps) and re.shape == (n,)
    for m in range(n):
        ref_cells, ref_av, ref_fields, ref_re = solo(lbm, params[m], obs[m], cells0[m], nsteps, fields=True)
        assert np.array_equal(cells[m], ref_cells), "member %d" % m
        assert_av_close(av[m], ref_av, "%dx%d member %d" % (nx, ny, m))
        for got, ref in zip(fields, ref_fields):
            assert np.array_equal(got[m], ref), "member %d" % m
        print("member %d: Re %.9e  solo %.9e" % (m, re[m], ref_re))
        assert re[m] == ref_re if ref_re == 0 else abs(re[m] / ref_re - 1.0) < 1e-4
    # member 0 against the fp32 oracle
    po = oracle_params(oracle_f32_omp, params[0], obs[0])
    ref = cells0[0].copy()
    av_ref = oracle_f32_omp.run(po, ref, obs[0], nsteps)
    assert max_rel(cells[0], ref) < RTOL_CELLS
    assert np.max(np.abs(av[0] - av_ref)) <= RTOL_AV * np.max(np.abs(av_ref)) + 1e-12


def test_split_runs_count_steps_and_keep_the_record(lbm, oracle_f32_omp):
    nx, ny, n = 100, 70, 4
    params, obs, cells0 = build_members(lbm, 77, nx, ny, n, 21)
    with lbm.Ensemble(params, obs) as ens:
        ens.upload(cells0)
        done = 0
        for part in (7, 3, 11):
            ens.run(part)
            done += part
            assert ens.steps_done == done
        ens.sync()
        with pytest.raises(lbm.LBMError):     # the record holds max_iters steps
            ens.run(1)
        assert ens.steps_done == 21
        cells, av = ens.download()
        # an upload starts the count again
        ens.upload(cells0)
        assert ens.steps_done == 0
        ens.run(21)
        cells_once, av_once = ens.download()
    assert av.shape == (n, 21)
    assert np.array_equal(cells, cells_once)
    for m in range(n):
        ref_cells, ref_av = solo(lbm, params[m], obs[m], cells0[m], 21)
        assert np.array_equal(cells[m], ref_cells)
        assert_av_close(av[m], ref_av, "split run, member %d" % m)
        assert_av_close(av_once[m], ref_av, "one run, member %d" % m)
    po = oracle_params(oracle_f32_omp, params[1], obs[1])
    ref = cells0[1].copy()
    av_ref = oracle_f32_omp.run(po, ref, obs[1], 21)
    assert np.max(np.abs(av[1] - av_ref)) <= RTOL_AV * np.max(np.abs(av_ref)) + 1e-12


def test_device_side_rest_state_equals_upload(lbm):
    nx, ny, n, nsteps = 128, 128, 5, 9
    params, obs, _ = build_members(lbm, 5, nx, ny, n, nsteps)
    # every member's host-side rest state from its own density (d2q9-bgk.c:529-550, fp32 like the host's)
    rest = np.empty((n, 9, ny, nx), dtype=np.float32)
    for m, p in enumerate(params):
        d = np.float32(p.density)
        rest[m, 0] = d * np.float32(4.0) / np.float32(9.0)
        rest[m, 1:5] = d / np.float32(9.0)
        rest[m, 5:9] = d / np.float32(36.0)
    with lbm.Ensemble(params, obs) as ens:
        ens.upload(None)
        at_rest, _ = ens.download(av_vels=False)
        ens.run(nsteps)
        a_cells, a_av = ens.download()
        ens.upload(rest)
        ens.run(nsteps)
        b_cells, b_av = ens.download()
    assert np.array_equal(at_rest, rest)
    assert np.array_equal(a_cells, b_cells) and np.array_equal(a_av, b_av)
    ref_cells, ref_av = solo(lbm, params[3], obs[3], None, nsteps)
    assert np.array_equal(a_cells[3], ref_cells)
    assert_av_close(a_av[3], ref_av, "rest state, member 3")


def test_all_blocked_and_none_blocked_members(lbm, oracle_f32):
    nx, ny, n, nsteps = 64, 16, 4, 13
    params, obs, cells0 = build_members(lbm, 3, nx, ny, n, nsteps)
    obs[1] = 1
    obs[2] = 0
    params[2] = lbm.make_params(nx, ny, nsteps, density=params[2].density, accel=params[2].accel, omega=params[2].omega,
                                obstacles=obs[2])
    params[1].free_cells_inv = 1.0  # 1/0 in the reference; any finite value, av_vels must be exactly 0
    with lbm.Ensemble(params, obs) as ens:
        ens.upload(cells0)
        ens.run(nsteps)
        cells, av = ens.download()
        fields = ens.final_state()
        re = ens.reynolds()
    for m in range(n):
        ref_cells, ref_av, ref_fields, ref_re = solo(lbm, params[m], obs[m], cells0[m], nsteps, fields=True)
        assert np.array_equal(cells[m], ref_cells), "member %d" % m
        assert_av_close(av[m], ref_av, "member %d" % m)
        for got, ref in zip(fields, ref_fields):
            assert np.array_equal(got[m], ref)
        assert re[m] == ref_re if ref_re == 0 else abs(re[m] / ref_re - 1.0) < 1e-4
    assert np.all(av[1] == 0.0) and re[1] == 0.0
    # the all-blocked member is a pure bounce-back permutation: bit-exact against the oracle
    po = oracle_params(oracle_f32, params[1], obs[1])
    po.free_cells_inv = 1.0
    ref = cells0[1].copy()
    oracle_f32.run(po, ref, obs[1], nsteps)
    assert np.array_equal(cells[1], ref)
    po = oracle_params(oracle_f32, params[2], obs[2])
    ref = cells0[2].copy()
    av_ref = oracle_f32.run(po, ref, obs[2], nsteps)
    assert max_rel(cells[2], ref) < RTOL_CELLS and max_rel(av[2], av_ref) < RTOL_AV


def test_members_are_independent(lbm):
    """member k's omega and obstacle map changed: every other member's cells AND av_vels stay bit-identical (same launch
    shape, hence the same summation order)"""
    nx, ny, n, nsteps, k = 128, 128, 6, 21, 2

    def run(params, obs):
        with lbm.Ensemble(params, obs) as ens:
            ens.upload(cells0)
            ens.run(nsteps)
            return ens.download()

    params, obs, cells0 = build_members(lbm, 11, nx, ny, n, nsteps)
    cells_a, av_a = run(params, obs)
    obs_b = obs.copy()
    obs_b[k] = (np.random.default_rng(12).random((ny, nx)) < 0.2).astype(np.int32)
    params_b = list(params)
    params_b[k] = lbm.make_params(nx, ny, nsteps, density=params[k].density, accel=params[k].accel, omega=1.23, obstacles=obs_b[k])
    cells_b, av_b = run(params_b, obs_b)
    for m in range(n):
        same = np.array_equal(cells_a[m], cells_b[m]) and np.array_equal(av_a[m], av_b[m])
        assert same == (m != k), "member %d" % m
    ref_cells, ref_av = solo(lbm, params_b[k], obs_b[k], cells0[k], nsteps)
    assert np.array_equal(cells_b[k], ref_cells)
    assert_av_close(av_b[k], ref_av, "changed member")


def test_broadcast_obstacle_map_and_sweep(lbm):
    p, obst = lbm.read_inputs(*input_files("128x128"))
    p.max_iters = 16
    omegas = [1.0, 1.3, float(p.omega)]
    with lbm.Ensemble(lbm.sweep_params(p, omega=omegas), obst) as ens:   # one [ny, nx] map for all members
        ens.upload(None)
        ens.run(16)
        cells, av = ens.download()
    for m, om in enumerate(omegas):
        pm = lbm.make_params(p.nx, p.ny, 16, p.reynolds_dim, p.density, p.accel, om, obst)
        ref_cells, ref_av = solo(lbm, pm, obst, None, 16)
        assert np.array_equal(cells[m], ref_cells)
        assert_av_close(av[m], ref_av, "omega %g" % om)


def test_full_run_of_a_sweep_passes_the_reference_checker(lbm, tmp_path):
    """eight members of the shipped 128x128 input, member 0 with the shipped constants and the others with omega swept, for the
    full 40 000 steps: member 0 passes check.py against the golden files like the ordinary context does
    (test_full_run_passes_reference_checker) and equals the solo run of the shipped input bit for bit"""
    p, obst = lbm.read_inputs(*input_files("128x128"))
    omegas = [float(p.omega)] + [float(v) for v in np.linspace(1.0, 1.9, 7)]
    with lbm.Ensemble(lbm.sweep_params(p, omega=omegas), obst) as ens:
        ens.upload(None)
        ens.run(p.max_iters)
        cells, av = ens.download()
        fields = ens.final_state()
        re = ens.reynolds()
    avd, fsd = check_outputs(tmp_path, "128x128", av[0], [f[0] for f in fields], obst)
    print("member 0: av_vels %.4f %%  final_state %.4f %%  Re %.9f" % (avd["max_diff_pcnt"], fsd["max_diff_pcnt"], re[0]))
    assert abs(avd["max_diff_pcnt"]) < 0.5 and abs(fsd["max_diff_pcnt"]) < 0.5
    assert abs(re[0] / 9.763598020526 - 1.0) < 5e-3
    solo_cells, solo_av = solo(lbm, p, obst, None, p.max_iters, options=None)
    assert np.array_equal(cells[0], solo_cells)
    assert_av_close(av[0], solo_av, "member 0 against the solo run")


def test_ensemble_beats_separate_contexts(lbm):
    """the condition the feature has to meet: 64 members of the shipped 128x128 input take less time per step as an ensemble
    than as 64 ordinary contexts with library defaults, every run issued before the first sync (tools/ensemble_ab.py: the same
    two timings, alternated, medians)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ensemble_ab
    r = ensemble_ab.measure("128x128", 64, steps=2000, reps=5)
    print(r)
    assert r["ensemble_us_per_step"]["median"] < r["contexts_us_per_step"]["median"]

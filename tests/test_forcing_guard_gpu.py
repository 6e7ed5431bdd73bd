"""The forcing guard's refusing branch in every kernel family.

accelerate_flow forces a free cell of row ny-2 only if f3 - aw1 > 0, f6 - aw2 > 0 and f7 - aw2 > 0: the one data-dependent
branch of the physics, restated in accelerate_cell (collide4: d2q9_step, step2/3/4, d2q9_multi, the ensembles), accelerate_pair
(collide2: d2q9_deep, d2q9_deep_twin, d2q9_resident), dp_accelerate_cell and the first-step row kernels.  On every other
input of the suite all three clauses hold in every cell.  The cases here (tests/_guard_case.py) refuse 8 to 150 cells of the
row at every step, each clause alone among them, at density 0.37, accel 0.2, omega 1.4; tests/test_forcing_guard_cpu.py holds
the conditions that make a comparison on them sound.

  1. one step per launch against the fp64 oracle.  Norm: max |got - ref64| per plane over that plane's mean |ref64| (next to
     the zero crossings of these states an elementwise relative error means nothing), the same for av_vels.  Gate:
     ORACLE_FORMS_FACTOR = 4 (tests/test_dp_gpu.py) times the larger norm of the two fp32 oracle forms against the fp64 oracle.
     And the cells forced in the first step are exactly the audited ones: with omega = 0 the step is streaming alone, so
     f1 of a forced cell arrives at its east neighbour as f1 + aw1 to the bit.
  2. every other fp32 form is bit-identical to single steps on the same case (av_vels to the 2e-6 of the sibling tests).
  3. row slabs (the forcing row in the top slab, its image recomputed in the neighbours' halos), ensembles (fp32, gated,
     fp64: refusing members beside one that never refuses) and double-precision contexts, as their sibling tests assert.

Every comparison of sections 2 and 3 also holds the single-step state of its own case and step count against the fp64 oracle
at the gate of section 1: the kernels share accelerate_cell / accelerate_pair / dp_accelerate_cell, and a defect there moves
single steps and the form under test alike.

Measured on an MI355X (v_rcp_f32 / v_sqrt_f32 in the collision), error over gate at ORACLE_FORMS_FACTOR = 4: the largest is 0.547
(256x37 after 23 steps, gate 4.9e-5 of a plane's mean), every other case and step count <= 0.31 (gates 3.5e-6 .. 7e-6).
fp64: 0.19 .. 0.30 (errors of 1 to 2e-16).  The factor stays at 4.  With the f7 clause deleted from accelerate_cell,
accelerate_pair and dp_accelerate_cell (a scratch build) 206 of the 212 cases fail.  The 6 that pass run one step only
(test_first_step_forces_exactly_the_audited_cells and the nsteps = 1 cases of test_single_steps_against_the_oracle): the
first step's forcing goes through the stand-alone row kernel, which the deletion does not touch."""
import numpy as np
import pytest

import _guard_case as G
from _dp_states import ORACLE_FORMS_FACTOR
from test_gpu_parity import SINGLE, max_rel, random_case

pytestmark = pytest.mark.gpu

_cache = {}


def params(lbm, name, nsteps, make=None):
    nx, ny, _, _ = G.CASES[name]
    density, accel, omega, ob, cells0 = G.case(name)
    return (make or lbm.make_params)(nx, ny, nsteps, density=density, accel=accel, omega=omega, obstacles=ob), ob, cells0


def run(lbm, name, nsteps, options, split=0, **kw):
    p, ob, cells0 = params(lbm, name, nsteps)
    with lbm.LBM(p, ob, **kw) as sim:
        for k, v in options.items():
            sim.set_option(k, v)
        if not kw:      # one slab: the kernel asked for is the kernel that runs
            for k in ("fuse", "multistep", "free_sweeps") + (("pair",) if options.get("fuse", 0) >= 4 else ()):
                if options.get(k, -1) >= 0 and not (k == "fuse" and options.get("multistep", 0) > 0):
                    assert sim.get_option(k) == options[k], (k, options[k])
        if options.get("nt_stores") == 1 and options.get("fuse", 0) >= 6:
            assert sim.get_option("steady") == 1     # launches of exactly 6, 7 or 8 steps run the per-depth kernels
        sim.upload(cells0)
        if split:
            sim.run(split)
            sim.sync()
        sim.run(nsteps - split)
        return sim.download()


def single(lbm, name, nsteps):
    """the case advanced by one step per launch on one slab, computed once per (case, step count) and left unchanged"""
    key = ("single", name, nsteps)
    if key not in _cache:
        cells, av = run(lbm, name, nsteps, SINGLE)
        cells.setflags(write=False)
        av.setflags(write=False)
        _cache[key] = (cells, av)
    return _cache[key]


# ---- the anchor: single steps against the oracle, on every case ------------------------------------------------------------
# The kernels share accelerate_cell / accelerate_pair / dp_accelerate_cell, so a defect there makes single steps and the form
# under test go wrong alike.  Every comparison with single steps below therefore also holds the single-step state of ITS case
# and step count against the fp64 oracle: got == single and single ~ oracle, hence got ~ oracle.

@pytest.fixture(scope="module")
def forms(oracle_f32_omp, oracle_f64_omp, tmp_path_factory):
    """(the two fp32 forms, the fp64 oracle, its FMA form)"""
    d = tmp_path_factory.mktemp("oracle_forms")
    return (oracle_f32_omp, G.oracle_form(d, "f32", 0, "fast")), oracle_f64_omp, G.oracle_form(d, "f64", 1, "fast")


plane_norm = G.plane_norm


def reference(forms, name, nsteps):
    """(fp64 oracle state after nsteps, its av_vels, spread, the fp32 oracle's audit); spread = the larger plane_norm of the two
    fp32 oracle forms against the fp64 oracle, over cells and av_vels; computed once per (case, step count)"""
    key = ("reference", name, nsteps)
    if key not in _cache:
        (f32_a, f32_b), f64, _ = forms
        density, accel, omega, ob, cells0 = G.case(name)
        assert nsteps <= G.CASES[name][2]       # the CPU file vouches for the case this far only
        _, ref, ref_av = G.guard_audit(f64, density, accel, omega, ob, cells0, nsteps, (nsteps,))
        spread, steps = 0.0, None
        for orc in (f32_a, f32_b):
            st, states, av = G.guard_audit(orc, density, accel, omega, ob, cells0, nsteps, (nsteps,))
            steps = steps or st
            spread = max(spread, plane_norm(states[nsteps], ref[nsteps]), plane_norm(av, ref_av))
        _cache[key] = (ref[nsteps], ref_av, spread, steps)
    return _cache[key]


def anchor(lbm, forms, name, nsteps):
    """single steps of the case against the fp64 oracle: (error, gate), computed once"""
    key = ("anchor", name, nsteps)
    if key not in _cache:
        ref, av_ref, spread, _ = reference(forms, name, nsteps)
        got, av = single(lbm, name, nsteps)
        err_cells, err_av = plane_norm(got, ref), plane_norm(av, av_ref)
        gate = ORACLE_FORMS_FACTOR * spread
        print("guard case %s, %d single steps: gpu error cells %.3e av_vels %.3e; fp32 oracle forms' spread %.3e, gate %.3e, ratio %.3f" %
              (name, nsteps, err_cells, err_av, spread, gate, max(err_cells, err_av) / gate))
        _cache[key] = (max(err_cells, err_av), gate)
    return _cache[key]


def assert_equals_single(lbm, forms, name, nsteps, got, av):
    err, gate = anchor(lbm, forms, name, nsteps)
    assert err <= gate, "single steps miss the oracle on this case"
    one, av_one = single(lbm, name, nsteps)
    assert np.all(np.isfinite(one))
    assert np.array_equal(got, one)
    assert max_rel(av, av_one) < 2e-6


# ---- 1. one step per launch against the oracle ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["260x33", "132x40", "1024x8"])
@pytest.mark.parametrize("nsteps", [1, 2, 11])
def test_single_steps_against_the_oracle(lbm, forms, name, nsteps):
    err, gate = anchor(lbm, forms, name, nsteps)
    assert err <= gate


@pytest.mark.parametrize("name", ["260x33", "132x40", "1024x8"])
def test_first_step_forces_exactly_the_audited_cells(lbm, forms, name):
    nx, ny, _, _ = G.CASES[name]
    density, accel, _, ob, cells0 = G.case(name)
    want = reference(forms, name, 1)[3][0]["accepted"]
    p = lbm.make_params(nx, ny, 1, density=density, accel=accel, omega=0.0, obstacles=ob)
    with lbm.LBM(p, ob) as sim:
        for k, v in SINGLE.items():
            sim.set_option(k, v)
        sim.upload(cells0)
        sim.run(1)
        got, _ = sim.download()
    row = ny - 2
    east = (np.arange(nx) + 1) % nx
    # without relaxation f1 of (x, row) lands in f1 of its east neighbour, or in f3 there if that cell is blocked
    arrived = np.where(ob[row, east] != 0, got[3, row, east], got[1, row, east])
    sent = cells0[1, row, :]
    aw1, _ = G.thresholds(density, accel, np.float32)
    grew = arrived != sent
    assert np.array_equal(arrived[grew], (sent + aw1)[grew])
    assert np.array_equal(grew, want)
    assert want.sum() >= 8 and (~want & (ob[row] == 0)).sum() >= 8


# ---- 2. every other fp32 form against single steps -----------------------------------------------------------------------

FUSED_SHAPES = [("256x37", 5), ("260x33", 4), ("1024x50", 7)]


@pytest.mark.parametrize("name,chunk", FUSED_SHAPES)
@pytest.mark.parametrize("nsteps", [5, 10])
def test_two_steps_per_launch(lbm, forms, name, chunk, nsteps):
    got, av = run(lbm, name, nsteps, {"multistep": 0, "fuse": 1, "chunk_rows": chunk})
    assert_equals_single(lbm, forms, name, nsteps, got, av)


@pytest.mark.parametrize("name,chunk", FUSED_SHAPES)
@pytest.mark.parametrize("nsteps", [5, 10])
@pytest.mark.parametrize("windows,bufs,pair", [(1, 1, 1), (1, 1, 0), (-1, 0, -1)])
def test_three_steps_per_launch(lbm, forms, name, chunk, nsteps, windows, bufs, pair):
    got, av = run(lbm, name, nsteps, {"multistep": 0, "fuse": 3, "windows": windows, "load_bufs": bufs, "pair": pair,
                                      "chunk_rows": chunk})
    assert_equals_single(lbm, forms, name, nsteps, got, av)


@pytest.mark.parametrize("name,chunk", FUSED_SHAPES)
@pytest.mark.parametrize("nsteps", [5, 10])
@pytest.mark.parametrize("pair", [1, 0])
def test_four_steps_per_launch(lbm, forms, name, chunk, nsteps, pair):
    got, av = run(lbm, name, nsteps, {"multistep": 0, "fuse": 4, "pair": pair, "chunk_rows": chunk})
    assert_equals_single(lbm, forms, name, nsteps, got, av)


@pytest.mark.parametrize("name", ["33x17", "130x31", "128x128"])
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("nsteps", [8, 21])
def test_lds_multistep(lbm, forms, name, T, nsteps):
    got, av = run(lbm, name, nsteps, {"multistep": T})
    err, gate = anchor(lbm, forms, name, nsteps)
    assert err <= gate, "single steps miss the oracle on this case"
    one, av_one = single(lbm, name, nsteps)
    assert np.array_equal(got, one)
    assert np.max(np.abs(av - av_one)) <= 2e-6 * np.max(np.abs(av_one)) + 1e-12


@pytest.mark.parametrize("name,bh", [("128x6", 2), ("132x64", 2), ("260x512", 2), ("1024x1024", 4)])
@pytest.mark.parametrize("nsteps,split", [(7, 3), (23, 0)])
def test_resident_kernel(lbm, forms, name, bh, nsteps, split):
    p, ob, cells0 = params(lbm, name, nsteps)
    with lbm.LBM(p, ob) as sim:
        sim.set_option("resident", 1)
        assert sim.get_option("resident") == bh
        sim.upload(cells0)
        if split:
            sim.run(split)
            sim.sync()
        sim.run(nsteps - split)
        got, av = sim.download()
    assert_equals_single(lbm, forms, name, nsteps, got, av)


# Grids this small run as one round of units, which fuse_schedule cuts into chunks of two rows whatever chunk_rows asks for:
# the forcing row ny-2 is the last row of its chunk on 37 and 33 rows (35 and 31 are odd) and the first on 50 rows
# (open top: the forcing row and its neighbours hold no blocked cell, so with obst_paths = 1 its waves take the obstacle-free path)
@pytest.mark.parametrize("name,chunk", FUSED_SHAPES + [("256x37 open top", 5)])
@pytest.mark.parametrize("nsteps", [8, 13, 23])
@pytest.mark.parametrize("depth,obst_paths,pair,nt", [(6, 0, 0, -1), (8, 1, 0, -1), (8, 0, 1, -1), (7, 1, 1, -1), (8, 1, -1, -1),
                                                      (8, 1, 0, 1), (7, 1, 0, 1), (6, 1, 0, 1), (8, 1, 1, 1), (8, 1, -1, 1)])
def test_deep_window_kernel(lbm, forms, name, chunk, nsteps, depth, obst_paths, pair, nt):
    opts = {"multistep": 0, "fuse": depth, "chunk_rows": chunk, "obst_paths": obst_paths, "pair": pair, "nt_stores": nt}
    if pair == 1:
        opts["twin_steps"] = depth
    got, av = run(lbm, name, nsteps, opts)
    assert_equals_single(lbm, forms, name, nsteps, got, av)


@pytest.mark.parametrize("nsteps", [8, 23])
@pytest.mark.parametrize("pair", [0, 1])
def test_deep_window_kernel_free_sweeps(lbm, forms, nsteps, pair):
    """no blocked cell at all: every wave runs collide2<false>, where the guard's obstacle operand folds away"""
    opts = {"multistep": 0, "fuse": 8, "chunk_rows": 24, "pair": pair, "nt_stores": 1, "free_sweeps": 1}
    if pair == 1:
        opts["twin_steps"] = 8
    got, av = run(lbm, "2048x260 free", nsteps, opts)
    assert_equals_single(lbm, forms, "2048x260 free", nsteps, got, av)


def test_balanced_wall_strips(lbm, forms):
    name, nsteps = "2048x260 walls", 8
    p, ob, cells0 = params(lbm, name, nsteps)
    with lbm.LBM(p, ob) as sim:
        for k, v in {"multistep": 0, "fuse": 8, "pair": 1, "nt_stores": 1, "balance": -1, "twin_steps": 8}.items():
            sim.set_option(k, v)
        assert sim.get_option("fuse") == 8 and sim.get_option("pair") == 1 and sim.get_option("balance") == 2
        sim.upload(cells0)
        sim.run(nsteps)
        got, av = sim.download()
    assert_equals_single(lbm, forms, name, nsteps, got, av)


# ---- 3. row slabs, ensembles, double precision ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["single", "fused2", "fused3", "multi8", "multi3", "auto"])
def test_row_slabs(lbm, forms, mode):
    opts = {"single": SINGLE, "fused2": {"fuse": 1, "multistep": 0}, "fused3": {"fuse": 3, "multistep": 0},
            "multi8": {"multistep": 8}, "multi3": {"multistep": 3}, "auto": {}}[mode]
    got, av = run(lbm, "260x50", 23, opts, devices=[0, 0, 0])
    assert_equals_single(lbm, forms, "260x50", 23, got, av)


@pytest.mark.parametrize("transport", ["peer", "copy"])
def test_row_slabs_deep_kernel(lbm, forms, transport, halo_defaults):
    halo_defaults(halo_depth=8, transport=transport)
    name, nsteps = "256x64", 23
    p, ob, cells0 = params(lbm, name, nsteps)
    with lbm.LBM(p, ob, devices=[0, 0]) as sim:
        sim.set_option("multistep", 0)
        sim.set_option("fuse", 8)
        assert sim.get_option("fuse") == 8 and sim.get_option("halo_depth") == 8
        assert sim.get_option("transport") == {"peer": 3, "copy": 2}[transport]
        sim.upload(cells0)
        sim.run(nsteps)
        got, av = sim.download()
    assert_equals_single(lbm, forms, name, nsteps, got, av)


def members(lbm, nsteps, make, real):
    """four guard cases with constants of their own and one plain random case at the default constants"""
    nx, ny = 48, 40
    ps, obs, cells = [], [], []
    for name in G.MEMBERS:
        density, accel, omega, ob, c0 = G.case(name, real=real)
        ps.append(make(nx, ny, nsteps, density=density, accel=accel, omega=omega, obstacles=ob))
        obs.append(ob)
        cells.append(c0)
    ob, c0 = random_case(np.random.default_rng(48), nx, ny)
    ps.append(make(nx, ny, nsteps, obstacles=ob))
    obs.append(ob)
    cells.append(c0.astype(real))
    return ps, np.stack(obs), np.stack(cells)


def solo(ctx, p, ob, c0, nsteps):
    with ctx(p, ob) as sim:
        sim.set_option("multistep", 0)
        if ctx.__name__ == "LBM":
            sim.set_option("fuse", 0)
        sim.upload(c0)
        sim.run(nsteps)
        return sim.download()


def member_reference(lbm, forms, m, ps, obs, cells0, nsteps):
    """member m on single steps in a context of its own; the guard members are held against the oracle as well"""
    if m < len(G.MEMBERS):
        err, gate = anchor(lbm, forms, G.MEMBERS[m], nsteps)
        assert err <= gate, "single steps miss the oracle on member %d" % m
        return single(lbm, G.MEMBERS[m], nsteps)
    return solo(lbm.LBM, ps[m], obs[m], cells0[m], nsteps)


def test_ensemble_members(lbm, forms):
    nsteps = 13
    ps, obs, cells0 = members(lbm, nsteps, lbm.make_params, np.float32)
    with lbm.Ensemble(ps, obs) as ens:
        ens.upload(cells0)
        ens.run(nsteps)
        cells, av = ens.download()
    for m in range(len(ps)):
        ref, av_ref = member_reference(lbm, forms, m, ps, obs, cells0, nsteps)
        assert np.all(np.isfinite(ref))
        assert np.array_equal(cells[m], ref), "member %d" % m
        assert np.max(np.abs(av[m] - av_ref)) <= 2e-6 * np.max(np.abs(av_ref)) + 1e-12, "member %d" % m


def test_gated_ensemble_members(lbm, forms):
    """run_until with a window and tolerance under which some members stop at the first check point and others run on: a
    member that stopped at c equals its single-step context after c steps"""
    from test_steady_gpu import rule
    max_steps, window, tol = G.GATE_MAX_STEPS, G.GATE_WINDOW, G.GATE_TOL
    ps, obs, cells0 = members(lbm, max_steps, lbm.make_params, np.float32)
    with lbm.Ensemble(ps, obs) as ens:
        ens.upload(cells0)
        ens.run(max_steps)
        record = ens.download(cells=False)[1]
    want_steps, want_conv = rule(record, 0, max_steps, window, tol)
    print("gated guard ensemble: stops %s converged %s" % (want_steps.tolist(), want_conv.astype(int).tolist()))
    with lbm.Ensemble(ps, obs) as ens:
        ens.upload(cells0)
        steps, conv = ens.run_until(max_steps, window=window, rel_tol=tol)
        cells, av = ens.download()
    assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
    assert len(set(steps[:len(G.MEMBERS)].tolist())) > 1      # some guard members stop early, others run on
    for m in range(len(ps)):
        c = int(steps[m])
        ref, av_ref = member_reference(lbm, forms, m, ps, obs, cells0, c)
        assert np.array_equal(cells[m], ref), "member %d stopped at %d" % (m, c)
        assert np.max(np.abs(av[m, :c] - av_ref)) <= 2e-6 * np.max(np.abs(av_ref)) + 1e-12, "member %d" % m


def test_double_precision_ensemble_members(lbm, forms):
    from _dp_states import max_abs, oracle_track
    _, f64, f64_fma = forms
    nsteps = 13
    ps, obs, cells0 = members(lbm, nsteps, lbm.make_dparams, np.float64)
    with lbm.EnsembleDouble(ps, obs) as ens:
        ens.upload(cells0)
        ens.run(nsteps)
        cells, av = ens.download()
    for m in range(len(ps)):
        ref, av_ref = solo(lbm.LBMDouble, ps[m], obs[m], cells0[m], nsteps)
        assert np.all(np.isfinite(ref))
        assert np.array_equal(cells[m], ref), "member %d" % m
        assert np.array_equal(av[m], av_ref), "member %d" % m
        if m < len(G.MEMBERS):      # the context itself against the fp64 oracle, at test_against_fp64_oracle's gate
            a, b = (oracle_track(o, ps[m], obs[m], cells0[m], [nsteps])[0] for o in (f64, f64_fma))
            gate = ORACLE_FORMS_FACTOR * max(max_abs(a[0], b[0]), max_abs(a[1], b[1]))
            err = max(max_abs(ref, a[0]), max_abs(av_ref, a[1]))
            print("guard member %d fp64, %d steps: max|gpu - oracle| %.3e, gate %.3e, ratio %.3f" % (m, nsteps, err, gate, err / gate))
            assert err <= gate, "member %d" % m


@pytest.mark.parametrize("name", list(G.DOUBLE_CASES))
def test_double_precision_against_the_oracle(lbm, forms, name):
    """the pattern of test_against_fp64_oracle (gate: 4 x what the fp64 oracle's two forms differ by, max |a - b| over cells and
    av_vels) at checkpoints 1, 2, 11 and 19, and the two kernel forms bit-identical (section 4 of that file)"""
    from _dp_states import gpu_track, max_abs, oracle_track
    _, oracle_f64_omp, fma = forms
    checkpoints = [1, 2, 11, 19]
    nx, ny, _, _ = G.CASES[name]
    density, accel, omega, ob, cells0 = G.case(name, real=np.float64)
    p = lbm.make_dparams(nx, ny, checkpoints[-1], density=density, accel=accel, omega=omega, obstacles=ob)
    ref = oracle_track(oracle_f64_omp, p, ob, cells0, checkpoints)
    alt = oracle_track(fma, p, ob, cells0, checkpoints)
    spread = max(max(max_abs(a[0], b[0]), max_abs(a[1], b[1])) for a, b in zip(ref, alt))
    gate = ORACLE_FORMS_FACTOR * spread
    got = {ms: gpu_track(lbm, p, ob, cells0, checkpoints, ms) for ms in (0, 8)}
    for ms in (0, 8):
        err = [max(max_abs(g[0], r[0]), max_abs(g[1], r[1])) for g, r in zip(got[ms], ref)]
        print("guard case %s fp64 multistep %d: max|gpu - oracle| at %s steps = %s; oracle forms differ by %.3e, gate %.3e, ratio %.3f" %
              (name, ms, checkpoints, ["%.3e" % e for e in err], spread, gate, max(err) / gate))
        assert max(err) <= gate, (name, ms)
    for a, b in zip(got[0], got[8]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

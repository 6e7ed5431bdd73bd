"""The output and read-back side on the GPU: final_state(), reynolds(), the av_vels record and download() in every context form.

(a) Fields and Reynolds number.  Upload, 9 steps, download the cells; final_state() and reynolds() against fields() of
    tests/_fields_ref.py (numpy float64) on those very cells, so only the output arithmetic differs.  Blocked cells exact
    (0, 0, 0, real(density) * real(1/3)); pressure of free cells to 10 * 2^-24 relative (nine fp32 additions, one multiply;
    fp64 forms 10 * 2^-53); velocities (max absolute error over the case's largest speed) and Reynolds number within 4 x the
    fp32 oracle's own distance from fields() on the same case (tests/test_output_stage_cpu.py measures it; Reynolds number
    never below 16 * 2^-24); fp64 forms 1e-12.
(b) The last av_vels entry against the mean speed (fields(), float64) of the state downloaded after the run: within 4 x the
    fp32 oracle's own distance between its record and fields() of its own states (the largest over the steps of the run and the
    oracle's two forms; fp64 forms 1e-12), on shapes where ncells * gate < 0.5: one lost or doubled average cell is two gates.
(c) Read-back stages in the grid that is not current.  run(a); download(); final_state(); reynolds(); run(b) must leave cells
    and the whole av_vels record array_equal to run(a); sync(); run(b), in every kernel family, and equal to single steps.

Spreads of the fp32 oracle (tests/test_output_stage_cpu.py, pytest -s): u_x, u_y, u 5.5e-7 .. 2.2e-6 of the largest speed after
9 steps (the ragged ensemble after 208 .. 400 steps: up to 4.2e-6); Reynolds number 3e-9 .. 8.5e-6 (the largest on 1030x511,
where the oracle adds 480 000 speeds one after the other in fp32); av_vels 2.3e-8 (256x37, 4 steps) .. 2.7e-6 (3x3).
Measured on an MI355X, largest error over gate per form:
  (a) LBM on one slab 0.46 (1024x520: pressure 2.8e-7 of 6.0e-7; velocities <= 0.31, Reynolds number <= 0.46 on 3x3: 1.4e-6 of
      3.1e-6), row slabs 0.44, Ensemble 0.50 (pressure 3.0e-7), ragged ensemble 0.43, LBMDouble and EnsembleDouble 0.20
      (pressure 2.2e-16 of 1.1e-15; velocities 2.9e-15, Reynolds number 4.4e-16 against 1e-12);
  (b) single steps 0.32 (30x17, step 9: 2.9e-7 of 8.9e-7; 512x24 <= 0.17, the four load variants to the digit), the other
      families 0.40 (fuse 1: 3.6e-8 of 9.1e-8, the narrowest gate), Ensemble 0.28, gated ensemble 0.15, fp64 <= 2.2e-16;
  (c) every continuation bit-identical on the unmodified library: no family reads a row of the other grid before writing it.
Scratch builds with one defect each, failures among the 87 cases: f[8] with the wrong sign in final_fields' ux 15; mask
ignored there 17; nx for row_stride there 17; the grid-stride loop's second trip one element late 2 (1030x511, 1024x520); the last
cell of a row left out of d2q9_step's velocity sum 19; pack_planes staging into the current grid 60; reynolds_dim dropped from
lbm_reynolds 15."""
import ctypes

import numpy as np
import pytest

import _fields_ref as F
from _guard_case import oracle_form
from test_gpu_parity import SINGLE, max_rel

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module")
def f32_forms(oracle_f32_omp, tmp_path_factory):
    """the fp32 oracle of the Makefile and its other honest form (momenta left to right, FMA contraction on)"""
    return oracle_f32_omp, oracle_form(tmp_path_factory.mktemp("oracle_forms"), "f32", 0, "fast")


def params(make, c, nsteps, ob):
    p = make(c["nx"], c["ny"], nsteps, reynolds_dim=c["reynolds_dim"], density=c["density"], accel=c["accel"],
             omega=c["omega"], obstacles=ob)
    if not (ob == 0).any():
        p.free_cells_inv = 1.0
    return p


def set_options(sim, opts, expect=None):
    for k, v in (opts or {}).items():
        sim.set_option(k, v)
    plan = {k: sim.get_option(k) for k in ("fuse", "multistep", "resident", "pair", "launch_steps", "nslabs", "halo_depth",
                                           "compact", "free_sweeps", "balance", "variant")}
    for k, v in (expect or {}).items():
        assert (plan[k] > 0) if v == "on" else (plan[k] == v), (k, plan)
    return plan


# ---- (a) fields and Reynolds number ------------------------------------------------------------------------------------------

def check_fields(what, got, re, cells, ob, c, gate, real=np.float32):
    """the four columns and the Reynolds number against fields() of the downloaded cells"""
    ref = F.fields(cells, ob, real(c["density"]), real(c["omega"]), c["reynolds_dim"])
    blocked = ob != 0
    for a in got:
        assert a.dtype == real
    for a in got[:3]:
        assert np.all(a[blocked] == 0.0) and not np.any(np.signbit(a[blocked]))
    assert np.all(got[3][blocked] == real(c["density"]) * real(1.0 / 3.0))
    err = F.field_errors(got, ref, ob)
    err["reynolds"] = abs(float(re) / ref["reynolds"] - 1.0)
    lim = dict(gate, pressure=F.PRESSURE_F32 if real is np.float32 else F.PRESSURE_F64)
    print("fields %-30s error (gate): %s; worst ratio %.3f" %
          (what, "  ".join("%s %.2e (%.2e)" % (k, err[k], lim[k]) for k in ("u_x", "u_y", "u", "pressure", "reynolds")),
           max(err[k] / lim[k] for k in err)))
    for k in err:
        assert err[k] <= lim[k], (what, k, err[k], lim[k])
    assert F.max_speed(ref) > 1e-3


F64_GATES = {"u_x": F.F64_GATE, "u_y": F.F64_GATE, "u": F.F64_GATE, "reynolds": F.F64_GATE, "av": F.F64_GATE}


def field_gates(f32_forms, c):
    return F.gates(F.oracle_spreads(f32_forms, c, F.FIELD_STEPS))


@pytest.mark.parametrize("name", list(F.ONE_SLAB))
def test_fields_one_slab(lbm, f32_forms, name):
    c = F.ONE_SLAB[name]
    ob, cells0 = F.inputs(c)
    with lbm.LBM(params(lbm.make_params, c, F.FIELD_STEPS, ob), ob) as sim:
        sim.upload(cells0)
        sim.run(F.FIELD_STEPS)
        cells, _ = sim.download()
        got, re = sim.final_state(), sim.reynolds()
    check_fields(name, got, re, cells, ob, c, field_gates(f32_forms, c))


@pytest.mark.parametrize("name", list(F.SLABS))
def test_fields_row_slabs(lbm, f32_forms, name):
    c = F.SLABS[name]
    ob, cells0 = F.inputs(c)
    with lbm.LBM(params(lbm.make_params, c, F.FIELD_STEPS, ob), ob, devices=[0] * c["nslabs"]) as sim:
        assert sim.get_option("nslabs") == c["nslabs"]
        sim.upload(cells0)
        sim.run(F.FIELD_STEPS)
        cells, _ = sim.download()
        got, re = sim.final_state(), sim.reynolds()
    check_fields(name, got, re, cells, ob, c, field_gates(f32_forms, c))


def members(make, cases, nsteps, real):
    obs, cells0 = zip(*(F.inputs(c, real) for c in cases))
    return [params(make, c, nsteps, ob) for c, ob in zip(cases, obs)], np.stack(obs), np.stack(cells0)


@pytest.mark.parametrize("name", list(F.ENSEMBLES))
def test_fields_ensemble(lbm, f32_forms, name):
    cases = F.ENSEMBLES[name]
    ps, obs, cells0 = members(lbm.make_params, cases, F.FIELD_STEPS, np.float32)
    with lbm.Ensemble(ps, obs) as ens:
        ens.upload(cells0)
        ens.run(F.FIELD_STEPS)
        cells, _ = ens.download()
        got, re = ens.final_state(), ens.reynolds()
    for m, c in enumerate(cases):
        check_fields("%s member %d" % (name, m), [a[m] for a in got], re[m], cells[m], obs[m], c, field_gates(f32_forms, c))


def ragged_run(lbm):
    """the channel sweep run to every member's own steady state: (members' cases, map, stops, cells, av, fields, Re)"""
    if "ragged" not in _cache:
        r = F.RAGGED
        ob = F.ragged_channel(r["nx"], r["ny"])
        cases = [F.case(r["nx"], r["ny"], 0, density=r["density"], omega=o, reynolds_dim=r["reynolds_dim"], accel=r["accel"])
                 for o in r["omegas"]]
        ps = [params(lbm.make_params, c, r["max_steps"], ob) for c in cases]
        with lbm.Ensemble(ps, ob) as ens:
            ens.upload(None)
            steps, _ = ens.run_until(r["max_steps"], window=r["window"], rel_tol=r["rel_tol"])
            cells, av = ens.download()
            _cache["ragged"] = (cases, ob, steps, cells, av, ens.final_state(), ens.reynolds())
    return _cache["ragged"]


def ragged_spread(f32_forms, c, ob, steps):
    r = F.RAGGED
    cells0 = np.ascontiguousarray(np.broadcast_to(F.W * r["density"], (9, r["ny"], r["nx"])).astype(np.float32))
    return F.oracle_spreads(f32_forms, c, steps, ob, cells0, av_window=r["window"])


def test_fields_ragged_ensemble(lbm, f32_forms):
    cases, ob, steps, cells, _, got, re = ragged_run(lbm)
    assert len(set(steps.tolist())) > 1, steps
    for m, c in enumerate(cases):
        gate = F.gates(ragged_spread(f32_forms, c, ob, int(steps[m])))
        check_fields("ragged member %d at %d" % (m, steps[m]), [a[m] for a in got], re[m], cells[m], ob, c, gate)


@pytest.mark.parametrize("name", list(F.DOUBLE))
def test_fields_double(lbm, name):
    c = F.DOUBLE[name]
    ob, cells0 = F.inputs(c, np.float64)
    with lbm.LBMDouble(params(lbm.make_dparams, c, F.FIELD_STEPS, ob), ob) as sim:
        sim.upload(cells0)
        sim.run(F.FIELD_STEPS)
        cells, _ = sim.download()
        got, re = sim.final_state(), sim.reynolds()
    check_fields("fp64 " + name, got, re, cells, ob, c, F64_GATES, np.float64)


def test_fields_double_ensemble(lbm):
    cases = F.DOUBLE_ENSEMBLE
    ps, obs, cells0 = members(lbm.make_dparams, cases, F.FIELD_STEPS, np.float64)
    with lbm.EnsembleDouble(ps, obs) as ens:
        ens.upload(cells0)
        ens.run(F.FIELD_STEPS)
        cells, _ = ens.download()
        got, re = ens.final_state(), ens.reynolds()
    for m, c in enumerate(cases):
        check_fields("fp64 ensemble member %d" % m, [a[m] for a in got], re[m], cells[m], obs[m], c, F64_GATES, np.float64)


@pytest.mark.parametrize("form", ["LBM", "LBM slabs", "Ensemble", "LBMDouble", "EnsembleDouble"])
def test_all_blocked_gives_reynolds_zero(lbm, form):
    """a grid (a member) without a free cell, free_cells_inv = 1: Reynolds number exactly 0, every cell reports 0, 0, 0, density / 3"""
    double = "Double" in form
    real, make = (np.float64, lbm.make_dparams) if double else (np.float32, lbm.make_params)
    c = F.case(64, 16, 70)
    _, cells0 = F.inputs(c, real)
    ob = np.ones((16, 64), np.int32)
    p = params(make, c, 4, ob)
    assert p.free_cells_inv == 1.0
    if "Ensemble" in form:
        c2 = F.case(64, 16, 71)
        ob2, cells2 = F.inputs(c2, real)
        with (lbm.EnsembleDouble if double else lbm.Ensemble)([p, params(make, c2, 4, ob2)], np.stack([ob, ob2])) as ens:
            ens.upload(np.stack([cells0, cells2]))
            ens.run(3)
            got, re = [a[0] for a in ens.final_state()], ens.reynolds()
        assert re[1] > 0.0
        re = re[0]
    else:
        kw = {"devices": [0, 0]} if form == "LBM slabs" else {}
        with (lbm.LBMDouble if double else lbm.LBM)(p, ob, **kw) as sim:
            sim.upload(cells0)
            sim.run(3)
            got, re = sim.final_state(), sim.reynolds()
    assert re == 0.0 and not np.signbit(re)
    assert all(np.all(a == 0.0) for a in got[:3])
    assert np.all(got[3] == real(c["density"]) * real(1.0 / 3.0))


@pytest.mark.parametrize("name,nslabs", [("132x40", 1), ("130x50 / 3", 3)])
def test_final_state_with_missing_columns(lbm, name, nslabs):
    """lbm_final_state with NULL columns: every column alone, and all but the pressure, are bit-identical to the four-column call;
    the rest of the caller's block keeps its sentinel"""
    lib = lbm.load_library()
    c = F.ONE_SLAB[name] if nslabs == 1 else F.SLABS[name]
    ob, cells0 = F.inputs(c)
    n = c["nx"] * c["ny"]
    sentinel = np.float32(-7.5)
    with lbm.LBM(params(lbm.make_params, c, F.FIELD_STEPS, ob), ob, **({"devices": [0] * nslabs} if nslabs > 1 else {})) as sim:
        sim.upload(cells0)
        sim.run(F.FIELD_STEPS)
        full = np.stack(sim.final_state()).reshape(4, n)
        assert not np.any(full == sentinel)
        for present in ([0], [1], [2], [3], [0, 1, 2]):
            block = np.full((4, n), sentinel, dtype=np.float32)
            args = [ctypes.c_void_p(block[i].ctypes.data) if i in present else None for i in range(4)]
            assert lib.lbm_final_state(sim.ctx, *args) == 0, lib.lbm_last_error()
            for i in range(4):
                assert np.array_equal(block[i], full[i] if i in present else np.full(n, sentinel)), (present, i)
        # and the run goes on from the same state
        assert np.array_equal(np.stack(sim.final_state()).reshape(4, n), full)


# ---- (b) the last av_vels entry against the state it came from ------------------------------------------------------------------

def check_av(what, av_last, cells, ob, c, gate, real=np.float32):
    ref = F.fields(cells, ob, real(c["density"]), real(c["omega"]), c["reynolds_dim"])["mean_u"]
    err = abs(float(av_last) / ref - 1.0)
    print("av_vels %-36s error %.2e gate %.2e ratio %.3f" % (what, err, gate, err / gate))
    assert c["nx"] * c["ny"] * gate < 0.5       # one lost or doubled average cell is at least two gates
    assert err <= gate, (what, err, gate)


@pytest.mark.parametrize("name,variant", [("512x24", 1), ("512x24", 2), ("512x24", 3), ("512x24", 4), ("30x17", 0)])
def test_av_vels_single_steps(lbm, f32_forms, name, variant):
    c, nsteps = F.AV_SINGLE[name]
    ob, cells0 = F.inputs(c)
    gate = F.gates(F.oracle_spreads(f32_forms, c, nsteps))["av"]
    with lbm.LBM(params(lbm.make_params, c, nsteps, ob), ob) as sim:
        set_options(sim, dict(SINGLE, variant=variant), {"fuse": 0, "multistep": 0, "resident": 0, "variant": variant or 1})
        sim.upload(cells0)
        for t in range(1, nsteps + 1):
            sim.run(1)
            cells, av = sim.download()
            assert av.size == t
            check_av("%s variant %d step %d" % (name, variant, t), av[t - 1], cells, ob, c, gate)


DEEP = {"multistep": 0, "fuse": 8, "nt_stores": 1}
# id -> (case of F.AV_CASES, steps, options, creation defaults, devices, expected plan)
AV_FAMILIES = {
    "fuse 1": ("256x37", 4, {"multistep": 0, "fuse": 1, "chunk_rows": 5}, {}, None, {"fuse": 1, "multistep": 0}),
    "fuse 3": ("256x37", 6, {"multistep": 0, "fuse": 3, "chunk_rows": 5}, {}, None, {"fuse": 3, "multistep": 0}),
    "fuse 4": ("256x37", 8, {"multistep": 0, "fuse": 4, "chunk_rows": 5}, {}, None, {"fuse": 4, "multistep": 0}),
    "deep lone": ("512x64", 8, dict(DEEP, pair=0), {}, None, {"fuse": 8, "pair": 0, "launch_steps": 8}),
    "deep twin": ("512x64", 8, dict(DEEP, pair=1, twin_steps=8), {}, None, {"fuse": 8, "pair": 1, "launch_steps": 8}),
    "twin5": ("1024x50", 5, {"multistep": 0, "fuse": 8, "pair": 1}, {}, None, {"fuse": 8, "pair": 1, "launch_steps": 5}),
    "multistep 8 33x17": ("33x17", 8, {"multistep": 8}, {}, None, {"multistep": 8}),
    "multistep 8 130x31": ("130x31", 8, {"multistep": 8}, {}, None, {"multistep": 8}),
    "resident 132x64": ("132x64", 7, {"resident": 1}, {}, None, {"resident": "on"}),
    "resident 128x6": ("128x6", 7, {"resident": 1}, {}, None, {"resident": "on"}),
    "slabs multi8": ("256x67 / 4", 8, {"multistep": 8}, {}, 4, {"multistep": 8, "nslabs": 4}),
    "slabs fused3": ("256x67 / 4", 6, {"multistep": 0, "fuse": 3}, {}, 4, {"fuse": 3, "nslabs": 4}),
    # slabs of 16 rows are too short for the deep window kernel (32): with fuse 8 asked for they run the four-step kernel
    "slabs fuse 8 asked": ("256x67 / 4", 8, {"multistep": 0, "fuse": 8}, {"halo_depth": 8}, 4, {"fuse": 4, "halo_depth": 8}),
    "slabs deep": ("256x64 / 2", 8, {"multistep": 0, "fuse": 8}, {"halo_depth": 8}, 2, {"fuse": 8, "halo_depth": 8}),
}


@pytest.mark.parametrize("family", list(AV_FAMILIES))
def test_av_vels_other_families(lbm, f32_forms, halo_defaults, family):
    name, nsteps, opts, defaults, nslabs, expect = AV_FAMILIES[family]
    c = F.AV_CASES[name][0]
    ob, cells0 = F.inputs(c)
    gate = F.gates(F.oracle_spreads(f32_forms, c, nsteps))["av"]
    halo_defaults(**defaults)
    with lbm.LBM(params(lbm.make_params, c, nsteps, ob), ob, **({"devices": [0] * nslabs} if nslabs else {})) as sim:
        print(family, set_options(sim, opts, expect))
        sim.upload(cells0)
        sim.run(nsteps)
        cells, av = sim.download()
    check_av(family, av[nsteps - 1], cells, ob, c, gate)


def test_av_vels_ensemble(lbm, f32_forms):
    cases = F.ENSEMBLES["37x29"]
    nsteps = 8
    ps, obs, cells0 = members(lbm.make_params, cases, nsteps, np.float32)
    with lbm.Ensemble(ps, obs) as ens:
        ens.upload(cells0)
        ens.run(nsteps)
        cells, av = ens.download()
    for m, c in enumerate(cases):
        gate = F.gates(F.oracle_spreads(f32_forms, c, nsteps))["av"]
        check_av("ensemble member %d" % m, av[m, nsteps - 1], cells[m], obs[m], c, gate)


def test_av_vels_gated_ensemble(lbm, f32_forms):
    cases, ob, steps, cells, av, _, _ = ragged_run(lbm)
    for m, c in enumerate(cases):
        gate = F.gates(ragged_spread(f32_forms, c, ob, int(steps[m])))["av"]
        check_av("gated member %d at %d" % (m, steps[m]), av[m, steps[m] - 1], cells[m], ob, c, gate)


def f64_av_gate(f32_forms, c, nsteps):
    """fp64 forms: the gate of the fp32 forms, and never above the 1e-12 of section (a)"""
    return min(F.gates(F.oracle_spreads(f32_forms, c, nsteps))["av"], F.F64_GATE)


@pytest.mark.parametrize("multistep", [0, 8])
def test_av_vels_double(lbm, f32_forms, multistep):
    for c, nsteps in (F.AV_CASES["127x129"], (F.DOUBLE_TWO_STAGE, 8)):      # one reduction stage, and two (tests/_fields_ref.py)
        name = "%dx%d" % (c["nx"], c["ny"])
        ob, cells0 = F.inputs(c, np.float64)
        with lbm.LBMDouble(params(lbm.make_dparams, c, nsteps, ob), ob) as sim:
            sim.set_option("multistep", multistep)
            sim.upload(cells0)
            sim.run(nsteps)
            cells, av = sim.download()
        check_av("fp64 %s multistep %d" % (name, multistep), av[nsteps - 1], cells, ob, c, f64_av_gate(f32_forms, c, nsteps), np.float64)


def test_av_vels_double_ensemble(lbm, f32_forms):
    nsteps = 8
    for cases in (F.DOUBLE_ENSEMBLE, F.DOUBLE_ENSEMBLE_TWO_STAGE):      # one reduction stage, and two
        ps, obs, cells0 = members(lbm.make_dparams, cases, nsteps, np.float64)
        with lbm.EnsembleDouble(ps, obs) as ens:
            ens.upload(cells0)
            ens.run(nsteps)
            cells, av = ens.download()
        for m, c in enumerate(cases):
            check_av("fp64 ensemble %dx%d member %d" % (c["nx"], c["ny"], m), av[m, nsteps - 1], cells[m], obs[m], c,
                     f64_av_gate(f32_forms, c, nsteps), np.float64)


# ---- (c) read-back does not disturb the run ------------------------------------------------------------------------------------

def walls_state(nx, ny, seed):
    """side walls and twenty blocked cells elsewhere (what makes the deep window kernels balance strips and sweep free waves)"""
    rng = np.random.default_rng(seed)
    ob = np.zeros((ny, nx), np.int32)
    ob[:, 0] = ob[:, -1] = 1
    ob[rng.integers(0, ny, 20), rng.integers(0, nx, 20)] = 1
    cells = (F.W * F.DENSITY * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5))).astype(np.float32)
    return ob, cells


def lbm_inputs(shape, nslabs, seed):
    nx, ny = shape
    c = F.case(nx, ny, seed, nslabs or 1)
    ob, cells0 = walls_state(nx, ny, seed) if shape == (2048, 260) else F.inputs(c)
    return c, ob, cells0


def read_back(sim):
    """everything a caller can look at between two runs"""
    out = sim.download()
    return out + (sim.final_state(), sim.reynolds())


TWIN8 = dict(DEEP, pair=1, twin_steps=8)
BALANCED = {"balance": "on", "free_sweeps": 1, "fuse": 8}
# id -> (shape, options, creation defaults, slabs, expected plan, also with a = b = 8)
LBM_FAMILIES = {
    "single": ((512, 24), SINGLE, {}, None, {"fuse": 0, "multistep": 0, "resident": 0}, False),
    "fuse 1": ((256, 37), {"multistep": 0, "fuse": 1, "chunk_rows": 5}, {}, None, {"fuse": 1}, False),
    "fuse 3": ((256, 37), {"multistep": 0, "fuse": 3, "chunk_rows": 5}, {}, None, {"fuse": 3}, False),
    "fuse 4": ((256, 37), {"multistep": 0, "fuse": 4, "chunk_rows": 5}, {}, None, {"fuse": 4}, True),
    "deep lone": ((512, 64), dict(DEEP, pair=0), {}, None, {"fuse": 8, "pair": 0}, True),
    "deep twin": ((512, 64), TWIN8, {}, None, {"fuse": 8, "pair": 1}, True),
    "deep lone balanced": ((2048, 260), dict(DEEP, pair=0, balance=-1), {}, None, dict(BALANCED, pair=0), True),
    "deep twin balanced": ((2048, 260), dict(TWIN8, balance=-1), {}, None, dict(BALANCED, pair=1), True),
    "multistep": ((130, 31), {"multistep": 8}, {}, None, {"multistep": 8}, True),
    "resident 132x64": ((132, 64), {"resident": 1}, {}, None, {"resident": "on"}, False),
    "resident 1000x600": ((1000, 600), {"resident": 1}, {}, None, {"resident": "on"}, False),
    "slabs deep peer": ((256, 64), {"multistep": 0, "fuse": 8}, {"halo_depth": 8, "transport": "peer"}, 2, {"fuse": 8, "halo_depth": 8}, True),
    "slabs deep copy": ((256, 64), {"multistep": 0, "fuse": 8}, {"halo_depth": 8, "transport": "copy"}, 2, {"fuse": 8, "halo_depth": 8}, True),
    "slabs five halo rows": ((1024, 640), {}, {}, 2, {"fuse": 5, "multistep": 0, "compact": 1, "pair": 1, "launch_steps": 5}, False),
    "slabs four steps": ((256, 50), {"multistep": 0, "fuse": 4}, {"halo_depth": 4}, 3, {"fuse": 4, "halo_depth": 4, "compact": 1}, True),
}
LBM_RUNS = [(f, 7, 9) for f in LBM_FAMILIES] + [(f, 8, 8) for f, v in LBM_FAMILIES.items() if v[5]]


def single_steps(lbm, c, ob, cells0, total):
    key = ("single", tuple(sorted(c.items())), total)
    if key not in _cache:
        with lbm.LBM(params(lbm.make_params, c, total, ob), ob) as sim:
            set_options(sim, SINGLE, {"fuse": 0, "multistep": 0, "resident": 0})
            sim.upload(cells0)
            sim.run(total)
            _cache[key] = sim.download()
        for a in _cache[key]:
            a.setflags(write=False)
    return _cache[key]


@pytest.mark.parametrize("family,a,b", LBM_RUNS)
def test_read_back_between_runs(lbm, halo_defaults, family, a, b):
    shape, opts, defaults, nslabs, expect, _ = LBM_FAMILIES[family]
    c, ob, cells0 = lbm_inputs(shape, nslabs, 80 + len(family))
    halo_defaults(**defaults)
    out = {}
    for looked in (True, False):
        with lbm.LBM(params(lbm.make_params, c, a + b, ob), ob, **({"devices": [0] * nslabs} if nslabs else {})) as sim:
            plan = set_options(sim, opts, expect)
            sim.upload(cells0)
            sim.run(a)
            if looked:
                mid = read_back(sim)
            else:
                sim.sync()
            sim.run(b)
            out[looked] = sim.download()
    print(family, plan)
    assert np.array_equal(out[True][0], out[False][0]), "the state after a read-back differs"
    assert np.array_equal(out[True][1], out[False][1]), "the av_vels record after a read-back differs"
    assert np.array_equal(mid[1], out[True][1][:a])
    if a == 7:      # and neither is wrong: single steps of the same case
        one, av_one = single_steps(lbm, c, ob, cells0, a + b)
        assert np.array_equal(out[True][0], one)
        assert max_rel(out[True][1], av_one) < 2e-6


def test_read_back_before_a_new_obstacle_map(lbm):
    a, b = 7, 9
    c = F.case(256, 96, 90)
    ob_a, cells0 = F.inputs(c)
    ob_b, _ = F.inputs(F.case(256, 96, 91))
    p = params(lbm.make_params, c, a + b, ob_b)
    out = {}
    for looked, opts in ((True, {}), (False, {}), ("single", SINGLE)):
        with lbm.LBM(p, ob_a) as sim:
            set_options(sim, opts)
            sim.upload(cells0)
            sim.run(a)
            if looked is True:
                read_back(sim)
            else:
                sim.sync()
            sim.upload_obstacles(ob_b)
            sim.run(b)
            out[looked] = sim.download()
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])
    assert np.array_equal(out[True][0], out["single"][0]) and max_rel(out[True][1], out["single"][1]) < 2e-6


def solo_single(lbm, c, ob, cells0, total):
    with lbm.LBM(params(lbm.make_params, c, total, ob), ob) as sim:
        set_options(sim, SINGLE)
        sim.upload(cells0)
        sim.run(total)
        return sim.download()


@pytest.mark.parametrize("a,b", [(7, 9), (8, 8)])
@pytest.mark.parametrize("resume", ["run", "run_until"])
def test_read_back_between_ensemble_runs(lbm, a, b, resume):
    """resume = run_until: the second leg is a steady run that no member's record ends (rel_tol 0), so the ensemble stays whole"""
    cases = F.ENSEMBLES["37x29"]
    ps, obs, cells0 = members(lbm.make_params, cases, a + b, np.float32)
    out = {}
    for looked in (True, False):
        with lbm.Ensemble(ps, obs) as ens:
            ens.upload(cells0)
            ens.run(a)
            if looked:
                read_back(ens)
            else:
                ens.sync()
            if resume == "run":
                ens.run(b)
            else:
                steps, conv = ens.run_until(b, window=3, rel_tol=0.0)
                assert steps.tolist() == [a + b] * len(cases) and not conv.any()
            out[looked] = ens.download()
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])
    if (a, resume) == (7, "run"):
        for m, c in enumerate(cases):
            one, av_one = solo_single(lbm, c, obs[m], cells0[m], a + b)
            assert np.array_equal(out[True][0][m], one), m
            assert max_rel(out[True][1][m], av_one) < 2e-6, m


@pytest.mark.parametrize("a,b", [(7, 9), (8, 8)])
@pytest.mark.parametrize("multistep", [0, 8])
def test_read_back_between_double_runs(lbm, multistep, a, b):
    c = F.DOUBLE["127x129"]
    ob, cells0 = F.inputs(c, np.float64)
    out = {}
    for looked, ms in ((True, multistep), (False, multistep), ("plain", 0)):
        with lbm.LBMDouble(params(lbm.make_dparams, c, a + b, ob), ob) as sim:
            sim.set_option("multistep", ms)
            assert sim.get_option("multistep") == ms
            sim.upload(cells0)
            if looked == "plain":       # one step per launch, uninterrupted
                sim.run(a + b)
            else:
                sim.run(a)
                if looked:
                    read_back(sim)
                else:
                    sim.sync()
                sim.run(b)
            out[looked] = sim.download()
    for other in (False, "plain"):
        assert np.array_equal(out[True][0], out[other][0]) and np.array_equal(out[True][1], out[other][1]), other


@pytest.mark.parametrize("a,b", [(7, 9), (8, 8)])
def test_read_back_between_double_ensemble_runs(lbm, a, b):
    cases = F.DOUBLE_ENSEMBLE
    ps, obs, cells0 = members(lbm.make_dparams, cases, a + b, np.float64)
    out = {}
    for looked in (True, False):
        with lbm.EnsembleDouble(ps, obs) as ens:
            ens.upload(cells0)
            ens.run(a)
            if looked:
                read_back(ens)
            else:
                ens.sync()
            ens.run(b)
            out[looked] = ens.download()
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])
    if a == 7:
        for m, c in enumerate(cases):
            with lbm.LBMDouble(ps[m], obs[m]) as sim:
                sim.set_option("multistep", 0)
                sim.upload(cells0[m])
                sim.run(a + b)
                one, av_one = sim.download()
            assert np.array_equal(out[True][0][m], one) and np.array_equal(out[True][1][m], av_one), m

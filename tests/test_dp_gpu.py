"""Double-precision contexts on the GPU (lbm_dp_*, lbm_amd.LBMDouble).

The reference's golden files come from an fp64 code, and any honest fp64 restatement of it lands at their print
precision whatever its operation order or FMA use (the fp64 oracle's two forms: <= 3e-10 % on av_vels, <= 1.1e-13 on the
velocity columns, <= 8e-13 relative on the Reynolds numbers).  So the gates here are pass/fail at print precision, not the
fp32 path's 1 %:
  1. full-length runs of the four shipped inputs against the golden files (av_vels < 1e-8 %, the oracle's own
     PRINT_PRECISION_PCNT; final states, Reynolds numbers);
  2. the same through the reference's checker;
  3. cells and av_vels at 1, 2, 11 and 1000 steps against the fp64 oracle, within 4x what the oracle's two forms differ by
     on the same case;
  4. the two kernel forms (one step per launch, LDS tiles at 1..8 steps per launch) and two identical runs: bit-identical;
  5. mass conservation; 6. a 4096 x 4096 cavity against the oracle; 7. an fp32 context beside an fp64 one is unaffected.
The 1024 x 1024 gates were confirmed on the CPU first: the oracle's pairwise-FMA form run over the full 20 000 steps lands
1.1e-10 % from the golden av_vels, within 0.50 f32 ulp of the stored pressure and 1.9e-13 from its Reynolds number."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

from _dp_states import (FULL, LDS, MASS_REL, ORACLE_FORMS_FACTOR, PRESSURE_ABS_256, PRINT_PRECISION_PCNT, RE_REL, VEL_ABS, gpu_track,
                        max_abs, max_pcnt, oracle_params, oracle_track, random_state, reynolds_ref)
from conftest import GOLDEN, ROOT, golden_cols, golden_path, input_files

pytestmark = pytest.mark.gpu


# ---- the oracle's second fp64 form ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_fma(oracle_f64_omp, tmp_path_factory):
    """oracle/d2q9_oracle.c built with pairwise momenta and FMA contraction (as a GPU compiler contracts), beside the
    fixture's left-to-right no-FMA form: two honest fp64 restatements whose difference sets the gate of section 3"""
    out = str(tmp_path_factory.mktemp("oracle_fma") / "liboracle_f64_fma.so")
    src = os.path.join(ROOT, "oracle", "d2q9_oracle.c")
    subprocess.run(["gcc", "-std=c99", "-O3", "-march=native", "-fPIC", "-DREAL=double", "-DORACLE_PAIRWISE=1",
                    "-ffp-contract=fast", "-fopenmp", "-shared", src, "-o", out, "-lm"], check=True)
    from oracle.oracle import Oracle
    o = Oracle("f64", omp=True)
    base = o.lib
    o.lib = ctypes.CDLL(out)
    for name in ("oracle_load_params", "oracle_load_obstacles", "oracle_init_cells", "oracle_accelerate_flow",
                 "oracle_timestep", "oracle_accelerate_row", "oracle_timestep_rows", "oracle_run", "oracle_av_velocity",
                 "oracle_calc_reynolds", "oracle_total_density", "oracle_final_fields", "oracle_write_values"):
        f, g = getattr(o.lib, name), getattr(base, name)
        f.argtypes, f.restype = g.argtypes, g.restype
    assert o.lib.oracle_pairwise_momentum() == 1 and o.lib.oracle_real_size() == 8
    assert oracle_f64_omp.lib.oracle_pairwise_momentum() == 0
    return o


# ---- 1. golden data at full length ---------------------------------------------------------------------------------

def full_run(lbm, size):
    p, ob = lbm.read_inputs_double(*input_files(size))
    assert p.max_iters == FULL[size]
    with lbm.LBMDouble(p, ob) as sim:
        sim.upload(None)
        sim.run(p.max_iters)
        _, av = sim.download(cells=False)
        fields = sim.final_state()
        re = sim.reynolds()
    return p, ob, av, fields, re


@pytest.mark.parametrize("size", ["128x128", "128x256"])
def test_full_length_golden_final_state(lbm, size):
    p, ob, av, (ux, uy, u, pr), re = full_run(lbm, size)
    e_av = max_pcnt(golden_cols("%s.av_vels.dat" % size, [1]), av)
    ref = golden_cols("%s.final_state.dat" % size, [2, 3, 4, 5, 6])
    e_pr = max_pcnt(ref[:, 3].reshape(p.ny, p.nx), pr)
    e_vel = [float(np.max(np.abs(ref[:, i].reshape(p.ny, p.nx) - got))) for i, got in enumerate((ux, uy, u))]
    e_re = abs(re / reynolds_ref(size) - 1.0)
    print("%s: av_vels %.3e %%  pressure %.3e %%  u_x/u_y/u %.3e %.3e %.3e  Re %.3e" % ((size, e_av, e_pr) + tuple(e_vel) + (e_re,)))
    assert np.array_equal(ref[:, 4].reshape(p.ny, p.nx).astype(np.int32), ob)
    assert e_av < PRINT_PRECISION_PCNT
    assert e_pr < PRINT_PRECISION_PCNT
    assert max(e_vel) <= VEL_ABS
    assert e_re < RE_REL


def test_full_length_golden_256x256(lbm):
    p, ob, av, (_, _, _, pr), re = full_run(lbm, "256x256")
    e_av = max_pcnt(golden_cols("256x256.av_vels.dat", [1]), av)
    d = np.load(os.path.join(GOLDEN, "generated", "256x256.final_state.npz"))
    assert d["pressure"].dtype == np.float64
    e_pr = float(np.max(np.abs(d["pressure"] - pr)))
    with open(os.path.join(GOLDEN, "transcripts.json")) as f:
        pins = json.load(f)["pressure_256x256"]
    e_pin = max(abs(pr[q["ii"], q["jj"]] - q["ref"]) for q in pins)
    e_re = abs(re / reynolds_ref("256x256") - 1.0)
    print("256x256: av_vels %.3e %%  pressure vs npz %.3e  vs pins %.3e  Re %.3e" % (e_av, e_pr, e_pin, e_re))
    assert e_av < PRINT_PRECISION_PCNT
    assert e_pr <= PRESSURE_ABS_256
    assert e_pin <= PRESSURE_ABS_256
    assert e_re < RE_REL


def test_full_length_golden_1024x1024(lbm):
    p, ob, av, (_, _, _, pr), re = full_run(lbm, "1024x1024")
    e_av = max_pcnt(golden_cols("1024x1024.av_vels.dat", [1]), av)
    d = np.load(os.path.join(GOLDEN, "generated", "1024x1024.final_state.npz"))
    stored = d["pressure"]
    assert stored.dtype == np.float32       # make_golden.py keeps this one as f32: the fp64 oracle rounded to f32
    ulps = np.abs(pr - stored.astype(np.float64)) / np.spacing(stored).astype(np.float64)
    e_re = abs(re / reynolds_ref("1024x1024") - 1.0)
    print("1024x1024: av_vels %.3e %%  pressure max %.3f f32 ulp  Re %.3e" % (e_av, float(ulps.max()), e_re))
    assert e_av < PRINT_PRECISION_PCNT
    assert float(ulps.max()) <= 1.0
    assert e_re < RE_REL


# ---- 2. through the reference's checker ------------------------------------------------------------------------------

def test_write_values_passes_reference_checker(lbm, tmp_path):
    import io
    from check.check import run_check
    p, ob = lbm.read_inputs_double(*input_files("128x128"))
    fs, avf = str(tmp_path / "final_state.dat"), str(tmp_path / "av_vels.dat")
    with lbm.LBMDouble(p, ob) as sim:
        sim.upload(None)
        sim.run(p.max_iters)
        sim.write_values(fs, avf)
    out = io.StringIO()
    code, avd, fsd = run_check(golden_path("128x128.av_vels.dat", tmp_path), golden_path("128x128.final_state.dat", tmp_path),
                               avf, fs, 1.0, out)
    print(out.getvalue())
    assert code == 0, out.getvalue()
    assert abs(avd["max_diff_pcnt"]) < PRINT_PRECISION_PCNT and abs(fsd["max_diff_pcnt"]) < PRINT_PRECISION_PCNT


def test_run_double_tool_writes_the_reference_files(tmp_path):
    import sys
    from check.check import run_check
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_double.py"), *input_files("128x128")], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("==done==\nReynolds number:\t\t")
    import io
    code, avd, fsd = run_check(golden_path("128x128.av_vels.dat", tmp_path), golden_path("128x128.final_state.dat", tmp_path),
                               str(tmp_path / "av_vels.dat"), str(tmp_path / "final_state.dat"), 1.0, io.StringIO())
    assert code == 0
    assert abs(avd["max_diff_pcnt"]) < PRINT_PRECISION_PCNT and abs(fsd["max_diff_pcnt"]) < PRINT_PRECISION_PCNT


# ---- 3. against the fp64 oracle --------------------------------------------------------------------------------------

CHECKPOINTS = [1, 2, 11, 1000]


def make_case(lbm, name):
    """(DParams, obstacles, initial cells or None) of one case of section 3"""
    kind, _, arg = name.partition(":")
    if kind == "shipped":
        p, ob = lbm.read_inputs_double(*input_files(arg))
        return p, ob, None
    nx, ny = (int(v) for v in arg.split("x"))
    rng = np.random.default_rng(sum(map(ord, name)))
    if kind == "ragged":
        # the rest state: a random one on 3x3 under acceleration diverges (the oracle itself reaches 1e104 by step 1000,
        # its two forms 1e104 apart), which tests nothing; random states have cases of their own
        ob = (rng.random((ny, nx)) < 0.1).astype(np.int32)
        return lbm.make_dparams(nx, ny, 1000, obstacles=ob), ob, None
    if kind == "random_state":
        ob = np.zeros((ny, nx), dtype=np.int32)
        return lbm.make_dparams(nx, ny, 1000, density=0.11, accel=0.007, omega=1.7, obstacles=ob), ob, \
            random_state(rng, 0.11, ny, nx)
    if kind == "random_mask":
        ob = (rng.random((ny, nx)) < 0.2).astype(np.int32)
        return lbm.make_dparams(nx, ny, 1000, obstacles=ob), ob, None
    if kind == "all_blocked":
        ob = np.ones((ny, nx), dtype=np.int32)
        return lbm.make_dparams(nx, ny, 1000, obstacles=ob), ob, random_state(rng, 0.1, ny, nx)
    if kind == "none_blocked":
        ob = np.zeros((ny, nx), dtype=np.int32)
        return lbm.make_dparams(nx, ny, 1000, obstacles=ob), ob, None
    if kind == "no_accel":
        ob = np.zeros((ny, nx), dtype=np.int32)
        return lbm.make_dparams(nx, ny, 1000, accel=0.0, obstacles=ob), ob, None
    raise ValueError(name)


ORACLE_CASES = ["shipped:128x128", "shipped:128x256", "shipped:256x256", "shipped:1024x1024",
                "ragged:3x3", "ragged:5x7", "ragged:127x129", "ragged:1000x3", "ragged:33x2049",
                "random_state:128x128", "random_state:200x72", "random_mask:256x96", "random_mask:70x50",
                "all_blocked:64x48", "none_blocked:64x48", "no_accel:96x80"]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_against_fp64_oracle(lbm, oracle_f64_omp, oracle_fma, name):
    p, ob, cells0 = make_case(lbm, name)
    p.max_iters = CHECKPOINTS[-1]
    start = cells0 if cells0 is not None else oracle_f64_omp.init_cells(oracle_params(oracle_f64_omp, p))
    ref = oracle_track(oracle_f64_omp, p, ob, start, CHECKPOINTS)
    alt = oracle_track(oracle_fma, p, ob, start, CHECKPOINTS)
    spread = max(max(max_abs(a[0], b[0]), max_abs(a[1], b[1])) for a, b in zip(ref, alt))
    gate = ORACLE_FORMS_FACTOR * spread
    for ms in (0, LDS):
        got = gpu_track(lbm, p, ob, cells0, CHECKPOINTS, ms)
        err = [max(max_abs(g[0], r[0]), max_abs(g[1], r[1])) for g, r in zip(got, ref)]
        print("%s multistep %d: max|gpu - oracle| at %s steps = %s; oracle forms differ by %.3e, gate %.3e" %
              (name, ms, CHECKPOINTS, ["%.3e" % e for e in err], spread, gate))
        assert max(err) <= gate, (name, ms)
        if name.startswith("no_accel"):
            # the rest state without acceleration stays exactly at rest: one value per plane, and opposite speeds equal,
            # so the momentum (pairwise differences) is exactly zero in every cell
            cells, av = got[-1]
            assert all(np.all(cells[k] == cells[k].flat[0]) for k in range(9))
            assert all(np.array_equal(cells[a], cells[b]) for a, b in ((1, 3), (2, 4), (5, 7), (6, 8), (5, 6)))
            assert float(np.max(np.abs(av))) <= 1e-15


# ---- 4. the two kernel forms are bit-identical -----------------------------------------------------------------------

def random_case(lbm, nx, ny, seed, steps):
    rng = np.random.default_rng(seed)
    ob = (rng.random((ny, nx)) < 0.1).astype(np.int32)
    return lbm.make_dparams(nx, ny, steps, obstacles=ob), ob, random_state(rng, 0.1, ny, nx)


def run_all(lbm, p, ob, cells0, steps, multistep, chunks=(1, 5)):
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_option("multistep", multistep)
        assert sim.get_option("multistep") == multistep
        sim.upload(cells0)
        for n in chunks:                  # runs of several lengths: launches of every depth, a flush mid-record
            sim.run(n)
        sim.run(steps - sum(chunks))
        cells, av = sim.download()
        return cells, av, sim.final_state(), sim.reynolds()


@pytest.mark.parametrize("nx,ny", [(128, 128), (127, 129), (300, 1000)])
def test_kernel_forms_bit_identical(lbm, nx, ny):
    steps = 37
    p, ob, cells0 = random_case(lbm, nx, ny, nx * 7 + ny, steps)
    base = run_all(lbm, p, ob, cells0, steps, 0)
    assert np.all(np.isfinite(base[0])) and base[1].shape == (steps,)
    for ms in range(1, 9):
        other = run_all(lbm, p, ob, cells0, steps, ms)
        assert np.array_equal(other[0], base[0]), ms
        assert np.array_equal(other[1], base[1]), ms
        for a, b in zip(other[2], base[2]):
            assert np.array_equal(a, b), ms
        assert other[3] == base[3], ms


def test_identical_runs_are_bit_identical(lbm):
    p, ob, cells0 = random_case(lbm, 200, 150, 5, 50)
    for ms in (-1, 0):
        a = run_all(lbm, p, ob, cells0, 50, ms) if ms == 0 else None
        with lbm.LBMDouble(p, ob) as s1, lbm.LBMDouble(p, ob) as s2:
            outs = []
            for s in (s1, s2):
                s.set_option("multistep", ms)
                s.upload(cells0)
                s.run(50)
                outs.append(s.download() + (s.final_state(), s.reynolds()))
        (c1, av1, f1, r1), (c2, av2, f2, r2) = outs
        assert np.array_equal(c1, c2) and np.array_equal(av1, av2) and r1 == r2
        assert all(np.array_equal(x, y) for x, y in zip(f1, f2))
        if a is not None:
            assert np.array_equal(a[0], c1) and np.array_equal(a[1], av1)


def test_auto_form_and_option_errors(lbm):
    p, ob, _ = random_case(lbm, 128, 128, 3, 4)
    with lbm.LBMDouble(p, ob) as sim:
        assert sim.get_option("multistep") == 8          # auto: LDS tiles on a launch-bound grid
        for bad in (-2, 9):
            with pytest.raises(lbm.LBMError):
                sim.set_option("multistep", bad)
        with pytest.raises(lbm.LBMError):
            sim.set_option("fuse", 1)
        with pytest.raises(lbm.LBMError):
            sim.get_option("fuse")
        sim.upload(None)
        sim.run(4)
        with pytest.raises(lbm.LBMError):
            sim.run(1)                                     # beyond max_iters
        assert sim.steps_done == 4
    p, ob, _ = random_case(lbm, 1024, 1024, 3, 4)
    with lbm.LBMDouble(p, ob) as sim:
        assert sim.get_option("multistep") == 0          # auto: one step per launch above 300K cells


# ---- 5. mass -----------------------------------------------------------------------------------------------------------

def test_mass_is_conserved(lbm):
    p, ob = lbm.read_inputs_double(*input_files("256x256"))
    p.max_iters = 1000
    with lbm.LBMDouble(p, ob) as sim:
        sim.upload(None)
        sim.run(1000)
        cells, _ = sim.download(av_vels=False)
    total = math.fsum(cells.ravel().tolist())
    rel = abs(total / (p.nx * p.ny * p.density) - 1.0)
    print("256x256 after 1000 steps: total density relative error %.3e" % rel)
    assert rel <= MASS_REL


# ---- 6. large grid ---------------------------------------------------------------------------------------------------

def test_large_cavity_against_oracle(lbm, oracle_f64_omp, oracle_fma):
    nx = ny = 4096
    ob = np.zeros((ny, nx), dtype=np.int32)       # bench.py's cavity(): walls on all four edges
    ob[0, :] = ob[-1, :] = 1
    ob[:, 0] = ob[:, -1] = 1
    p = lbm.make_dparams(nx, ny, 4, obstacles=ob)
    start = oracle_f64_omp.init_cells(oracle_params(oracle_f64_omp, p))
    ref = oracle_track(oracle_f64_omp, p, ob, start, [4])[0]
    alt = oracle_track(oracle_fma, p, ob, start, [4])[0]
    gate = ORACLE_FORMS_FACTOR * max(max_abs(ref[0], alt[0]), max_abs(ref[1], alt[1]))
    with lbm.LBMDouble(p, ob) as sim:
        assert sim.get_option("multistep") == 0
        sim.upload(None)
        sim.run(4)
        cells, av = sim.download()
    err = max(max_abs(cells, ref[0]), max_abs(av, ref[1]))
    print("4096x4096 cavity, 4 steps: max|gpu - oracle| %.3e, gate %.3e" % (err, gate))
    assert err <= gate


# ---- 7. coexistence with an fp32 context -------------------------------------------------------------------------------

def test_fp32_context_unaffected_by_dp_context(lbm):
    p32, ob = lbm.read_inputs(*input_files("256x256"))
    p32.max_iters = 200
    with lbm.LBM(p32, ob) as sim:
        sim.upload(None)
        for _ in range(4):            # the same runs as below: an fp32 record depends on how a run is cut into launches
            sim.run(50)
        alone = sim.download() + (sim.reynolds(),)
    pdp, _ = lbm.read_inputs_double(*input_files("256x256"))
    pdp.max_iters = 200
    with lbm.LBM(p32, ob) as sim, lbm.LBMDouble(pdp, ob) as dp:
        sim.upload(None)
        dp.upload(None)
        for _ in range(4):
            dp.run(50)
            sim.run(50)
        dp.sync()
        beside = sim.download() + (sim.reynolds(),)
        dp_cells, _ = dp.download()
    assert np.array_equal(alone[0], beside[0]) and np.array_equal(alone[1], beside[1]) and alone[2] == beside[2]
    assert np.all(np.isfinite(dp_cells))

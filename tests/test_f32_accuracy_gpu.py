"""The fp32 kernels held to the fp64 oracle in units of rounding (tests/_f32_ref.py; the gates are proven on the CPU in
tests/test_f32_accuracy_cpu.py).

  1. One step of d2q9_step (fuse 0, multistep 0, run(1), accelerate_flow included) against the truth, beside the fp32 oracle on
     the same case: 33x19 (scalar path), 64x48 (float4 path) and 256x8 (wave-level load modes), the last two with every load
     variant, omega 0.6 / 1.0 / 1.7 / 1.99, density 0.1 / 1 / 100, near rest and driven.  Blocked cells exact; rms, max, class /
     mass / momentum means, the sensitivities a and b, and av_vels within av_bound.
  2. Every other family on the driven state, bit for bit against d2q9_step, where until now these identities were only tested
     near rest at density 0.1: the pair form (collide_pair) and the LDS-tile collision are separate spellings of the arithmetic.
  3. Sixteen steps once per family: rms, max and class means against the fp32 oracle's, av_vels of every step within 16 av_bound.

Every figure is printed (pytest -s); profiles/f32_accuracy.txt holds the worst of each."""
import numpy as np
import pytest

import _f32_ref as fr
from test_gpu_parity import SINGLE, oracle_params, run_gpu

pytestmark = pytest.mark.gpu

ACCEL = 0.005
_cases, _single = {}, {}


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def case(lbm, oracle_f32, oracle_f64, nx, ny, omega, density, state, nsteps):
    """inputs, truth and the fp32 oracle's run with its figures, computed once per case and left unchanged"""
    key = (nx, ny, omega, density, state, nsteps)
    if key not in _cases:
        ob, cells = fr.build_state(state, nx, ny, density)
        p = lbm.make_params(nx, ny, nsteps, density=density, accel=ACCEL, omega=omega, obstacles=ob)
        tr = fr.truth(oracle_f64, p, ob, cells, nsteps)
        ref = cells.copy()
        av = oracle_f32.run(oracle_params(oracle_f32, p, ob), ref, ob, nsteps)
        for a in (ob, cells, ref):
            a.setflags(write=False)
        _cases[key] = dict(p=p, ob=ob, cells=cells, tr=tr, ref=ref, av=av, orc=fr.measure(ref, tr, ob))
    return _cases[key]


# ---- 1. one step against the truth -----------------------------------------------------------------------------------------------

ANCHORS = [(33, 19, 0)] + [(64, 48, v) for v in (1, 2, 3, 4)] + [(256, 8, v) for v in (1, 2, 3, 4)]


@pytest.mark.parametrize("state", fr.STATES)
@pytest.mark.parametrize("density", fr.DENSITIES)
@pytest.mark.parametrize("omega", fr.OMEGAS)
@pytest.mark.parametrize("nx,ny,variant", ANCHORS)
def test_one_step_against_fp64(lbm, oracle_f32, oracle_f64, nx, ny, variant, omega, density, state):
    c = case(lbm, oracle_f32, oracle_f64, nx, ny, omega, density, state, 1)
    with lbm.LBM(c["p"], c["ob"]) as sim:
        for k, v in dict(SINGLE, variant=variant).items():
            sim.set_option(k, v)
        if nx % 256 == 0:
            assert sim.get_option("variant") == variant
        sim.upload(c["cells"])
        sim.run(1)
        got, av = sim.download()
    tr, ob = c["tr"], c["ob"]
    m = fr.measure(got, tr, ob)
    gates = fr.check_gates(m, c["orc"])
    bound = fr.av_bound(tr["u"][0], tr["inv64"])
    d_av = abs(float(av[0]) - tr["av"][0])
    what = "%dx%d v%d om %.2f rho %g %s" % (nx, ny, variant, omega, density, state)
    print(fr.line(what + " oracle", c["orc"]))
    print(fr.line(what + " gpu", m))
    print("   rms ratio %.3f max ratio %.3f  av_vels off by %.2e (oracle %.2e) bound %.2e  failed: %s" % (
        m["rms"] / c["orc"]["rms"], m["max"] / c["orc"]["max"], d_av, abs(float(c["av"][0]) - tr["av"][0]), bound, fr.failed(gates)))
    assert fr.blocked_equal(got, tr, ob)
    assert not fr.failed(gates), gates
    assert d_av <= bound


# ---- 2. every family on the driven state, bit for bit against d2q9_step ------------------------------------------------------

def deep(depth, pair, paths):
    opts = {"multistep": 0, "fuse": depth, "chunk_rows": 0, "obst_paths": paths, "pair": pair, "nt_stores": -1}
    if pair == 1:
        opts["twin_steps"] = depth
    return opts


# name -> (nx, ny, options, checks on the options in force)
FAMILIES = {
    "fuse1 256x8": (256, 8, {"multistep": 0, "fuse": 1, "chunk_rows": 0}, {"fuse": 1}),
    "fuse3 256x8": (256, 8, {"multistep": 0, "fuse": 3, "chunk_rows": 0}, {}),
    "fuse4 256x8": (256, 8, {"multistep": 0, "fuse": 4, "chunk_rows": 0}, {}),
    "fuse1 260x33": (260, 33, {"multistep": 0, "fuse": 1, "chunk_rows": 4}, {"fuse": 1}),
    "fuse3 260x33": (260, 33, {"multistep": 0, "fuse": 3, "chunk_rows": 4}, {"fuse": 3}),
    "fuse4 260x33": (260, 33, {"multistep": 0, "fuse": 4, "chunk_rows": 4}, {"fuse": 4}),
    "multi8 33x17": (33, 17, {"multistep": 8}, {"multistep": 8}),
    "multi8 5x4": (5, 4, {"multistep": 8}, {"multistep": 8}),
    "resident 128x6": (128, 6, {"resident": 1}, {"resident": 2}),
}
for _d in (6, 8):
    for _pair in (0, 1):
        for _paths in (0, 1):
            FAMILIES["deep%d pair%d paths%d 256x32" % (_d, _pair, _paths)] = (256, 32, deep(_d, _pair, _paths), {"fuse": _d, "pair": _pair})
SIXTEEN = ["fuse1 260x33", "fuse3 260x33", "fuse4 260x33", "multi8 33x17", "resident 128x6", "deep8 pair0 paths1 256x32",
           "deep8 pair1 paths1 256x32"]


def family_inputs(lbm, name, density, omega, nsteps):
    """the driven state of the family's shape; the resident kernel and the second collision path of the deep kernel get the rows
    without blocked cells that their own tests give them"""
    nx, ny, _, _ = FAMILIES[name]
    ob, cells = fr.build_state("driven", nx, ny, density)
    if name.startswith("resident"):
        ob[0, :] = ob[-1, :] = 0
    if "paths1" in name:
        ob[ny // 3: 2 * ny // 3, :] = 0
    p = lbm.make_params(nx, ny, nsteps, density=density, accel=ACCEL, omega=omega, obstacles=ob)
    return p, ob, cells


def single_steps(lbm, p, ob, cells, nsteps):
    key = (p.nx, p.ny, float(p.density), float(p.omega), float(p.accel), nsteps, ob.tobytes(), cells[:, 0].tobytes())
    if key not in _single:
        _single[key] = run_gpu(lbm, p, ob, cells, nsteps, SINGLE)
        assert np.all(np.isfinite(_single[key][0]))
    return _single[key]


def run_family(lbm, name, p, ob, cells, nsteps):
    _, _, opts, expect = FAMILIES[name]
    with lbm.LBM(p, ob) as sim:
        for k, v in opts.items():
            sim.set_option(k, v)
        for k, v in expect.items():
            assert sim.get_option(k) == v, (name, k)
        sim.upload(cells)
        sim.run(nsteps)
        return sim.download()


def av_close(av, av_ref):
    """two summation orders of the same terms (the bound of test_two_steps_per_launch_equals_single_steps)"""
    return float(np.max(np.abs(av - av_ref))) <= 2e-6 * float(np.max(np.abs(av_ref)))


@pytest.mark.parametrize("omega", [1.99, 0.6])
@pytest.mark.parametrize("density", [1.0, 100.0])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_equals_single_steps_on_the_driven_state(lbm, name, density, omega):
    p, ob, cells = family_inputs(lbm, name, density, omega, 8)
    one, av_one = single_steps(lbm, p, ob, cells, 8)
    got, av = run_family(lbm, name, p, ob, cells, 8)
    assert np.array_equal(got, one)
    assert av_close(av, av_one)


def members(lbm, density, omega, nsteps):
    """three members on 33x19: the driven state shifted by one column per member, omega / 1.0 / 1.7, their own accel"""
    nx, ny = 33, 19
    ob0, cells0 = fr.build_state("driven", nx, ny, density)
    obs = np.stack([np.roll(ob0, m, axis=1) for m in range(3)])
    cells = np.stack([np.roll(cells0, m, axis=2) for m in range(3)])
    params = [lbm.make_params(nx, ny, nsteps, density=density, accel=ACCEL * (1 + m), omega=om, obstacles=obs[m])
              for m, om in enumerate((omega, 1.0, 1.7))]
    return params, obs, cells


def run_ensemble(lbm, how, params, obs, cells, nsteps):
    with lbm.Ensemble(params, obs) as ens:
        ens.upload(cells)
        if how == "run":
            ens.run(nsteps)
        else:   # the gated kernel; rel_tol 0 stops no member: the record of a driven state never repeats
            steps, conv = ens.run_until(nsteps, window=nsteps // 2, rel_tol=0.0)
            assert steps.tolist() == [nsteps] * 3 and not conv.any()
        return ens.download()


@pytest.mark.parametrize("omega", [1.99, 0.6])
@pytest.mark.parametrize("density", [1.0, 100.0])
@pytest.mark.parametrize("how", ["run", "run_until"])
def test_ensemble_members_equal_single_steps_on_the_driven_state(lbm, how, density, omega):
    params, obs, cells = members(lbm, density, omega, 8)
    got, av = run_ensemble(lbm, how, params, obs, cells, 8)
    for m in range(3):
        one, av_one = single_steps(lbm, params[m], obs[m], cells[m], 8)
        assert np.array_equal(got[m], one), "member %d" % m
        assert av_close(av[m], av_one), "member %d" % m


# ---- 3. sixteen steps, once per family ----------------------------------------------------------------------------------

def sixteen_gates(what, got, av, tr, ref, av_ref, ob):
    m, orc = fr.measure(got, tr, ob), fr.measure(ref, tr, ob)
    gates = fr.check_gates(m, orc)
    bounds = np.array([16.0 * fr.av_bound(u, tr["inv64"]) for u in tr["u"]])
    d_av = np.abs(av.astype(np.float64) - tr["av"])
    print(fr.line(what + " oracle", orc))
    print(fr.line(what + " gpu", m))
    print("   rms ratio %.3f max ratio %.3f  av_vels off by at most %.4f of 16 av_bound (oracle %.4f)  failed: %s" % (
        m["rms"] / orc["rms"], m["max"] / orc["max"], float(np.max(d_av / bounds)),
        float(np.max(np.abs(av_ref.astype(np.float64) - tr["av"]) / bounds)), fr.failed(gates)))
    assert np.all(np.isfinite(got))
    assert not fr.failed(gates), gates
    assert np.all(d_av <= bounds)


@pytest.mark.parametrize("name", ["single 64x48"] + SIXTEEN)
def test_sixteen_steps_against_fp64(lbm, oracle_f32, oracle_f64, name):
    density, omega = 1.0, 1.7
    if name.startswith("single"):
        ob, cells = fr.build_state("driven", 64, 48, density)
        p = lbm.make_params(64, 48, 16, density=density, accel=ACCEL, omega=omega, obstacles=ob)
        got, av = single_steps(lbm, p, ob, cells, 16)
    else:
        p, ob, cells = family_inputs(lbm, name, density, omega, 16)
        got, av = run_family(lbm, name, p, ob, cells, 16)
    tr = fr.truth(oracle_f64, p, ob, cells, 16)
    ref = cells.copy()
    av_ref = oracle_f32.run(oracle_params(oracle_f32, p, ob), ref, ob, 16)
    sixteen_gates("16 steps " + name, got, av, tr, ref, av_ref, ob)


@pytest.mark.parametrize("how", ["run", "run_until"])
def test_sixteen_steps_of_an_ensemble_against_fp64(lbm, oracle_f32, oracle_f64, how):
    params, obs, cells = members(lbm, 1.0, 1.99, 16)
    got, av = run_ensemble(lbm, how, params, obs, cells, 16)
    for m in range(3):
        tr = fr.truth(oracle_f64, params[m], obs[m], cells[m], 16)
        ref = cells[m].copy()
        av_ref = oracle_f32.run(oracle_params(oracle_f32, params[m], obs[m]), ref, obs[m], 16)
        sixteen_gates("16 steps Ensemble.%s member %d" % (how, m), got[m], av[m], tr, ref, av_ref, obs[m])

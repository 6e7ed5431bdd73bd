"""The gates of tests/_f32_ref.py proven on the CPU: what tests/test_f32_accuracy_gpu.py asks of the HIP kernels is asked here of
a numpy stand-in, which must pass, and of the stand-in with seeded defects, each of which must fail the gate named for it
while it passes the suite's older gate RTOL_CELLS = 2e-5 (asserted, to document the gap).  Also the conditions on the inputs."""
import numpy as np
import pytest

import _f32_ref as fr

RTOL_CELLS = 2e-5   # tests/test_gpu_parity.py
f32, f64 = np.float32, np.float64
CASES = [(nx, ny, om, d, st) for (nx, ny) in fr.SHAPES for om in fr.OMEGAS for d in fr.DENSITIES for st in fr.STATES]
_cache = {}


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def fma(a, b, c):
    """a fused multiply-add: the float64 product and sum, rounded once to fp32"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def ulps(x, n):
    x = f32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf if n > 0 else -np.inf), dtype=f32)
    return x


def emulate_step(p, ob, cells, defect=None):
    """A STAND-IN KERNEL FOR PROVING THE GATES, NOT A REFERENCE: accelerate_flow, the gather and collide_cell
    (csrc/d2q9_kernels.h) restated on fp32 numpy arrays, every operation rounded to fp32 in collide_cell's order and grouping,
    its fused multiply-adds as fma() above, the reciprocal correctly rounded (the hardware's is good to 1 ulp).  `defect` seeds
    one fault: "w2+2", "w0-1" (a weight off by ulps), "omega+2", "h3" (h3 = 3.000001 h), "rcp+4" / "rcp+1" (the correctly rounded
    reciprocal moved up that many places on every cell: off by up to 4.5 / 1.5 ulp), "rcp_up" (the first fp32 above the exact
    reciprocal on every cell: off by up to 1 ulp, always high), "swap68" (equilibria 6 and 8 swapped), "nofma" (every product
    rounded)."""
    c = np.array(cells, dtype=f32)
    dens_, accel = f32(p.density), f32(p.accel)
    aw1, aw2 = dens_ * accel / f32(9.0), dens_ * accel / f32(36.0)
    row = p.ny - 2
    ok = (ob[row] == 0) & (c[3, row] - aw1 > 0) & (c[6, row] - aw2 > 0) & (c[7, row] - aw2 > 0)
    for k, a in ((1, aw1), (5, aw2), (8, aw2), (3, -aw1), (6, -aw2), (7, -aw2)):
        c[k, row] = np.where(ok, c[k, row] + a, c[k, row])
    g = fr.gather(c)
    w0, w1, w2 = f32(4.0) / f32(9.0), f32(1.0) / f32(9.0), f32(1.0) / f32(36.0)
    omega = f32(p.omega)
    three = f32(3.0)
    if defect == "w2+2":
        w2 = ulps(w2, 2)
    if defect == "w0-1":
        w0 = ulps(w0, -1)
    if defect == "omega+2":
        omega = ulps(omega, 2)
    mad = fma if defect != "nofma" else (lambda a, b, cc: (a * b) + cc)
    dens = g[0] + g[1]
    for k in range(2, 9):
        dens = dens + g[k]
    densinv = f32(1.0) / dens
    if defect in ("rcp+4", "rcp+1"):
        n = int(defect[-1])
        for _ in range(n):
            densinv = np.nextafter(densinv, f32(np.inf), dtype=f32)
    if defect == "rcp_up":
        low = densinv.astype(f64) * dens.astype(f64) < 1.0      # (the product of two fp32 values is exact in double)
        densinv = np.where(low, np.nextafter(densinv, f32(np.inf), dtype=f32), densinv)
    da, db = g[5] - g[7], g[8] - g[6]
    jx = (g[1] - g[3]) + (da + db)
    jy = (g[2] - g[4]) + (da - db)
    usq = mad(jx, jx, jy * jy)
    h = f32(1.5) * densinv
    cc = mad(-h, usq, dens)
    h3 = (f32(3.000001) if defect == "h3" else three) * h
    jp, jm = jx + jy, jx - jy
    ax, ay, ap, am = mad(h3 * jx, jx, cc), mad(h3 * jy, jy, cc), mad(h3 * jp, jp, cc), mad(h3 * jm, jm, cc)
    eq = [None] * 9
    eq[0] = w0 * cc
    eq[1], eq[3] = w1 * mad(three, jx, ax), w1 * mad(-three, jx, ax)
    eq[2], eq[4] = w1 * mad(three, jy, ay), w1 * mad(-three, jy, ay)
    eq[5], eq[7] = w2 * mad(three, jp, ap), w2 * mad(-three, jp, ap)
    eq[8], eq[6] = w2 * mad(three, jm, am), w2 * mad(-three, jm, am)
    if defect == "swap68":
        eq[6], eq[8] = eq[8], eq[6]
    blk = ob != 0
    out = np.empty_like(g)
    for k in range(9):
        out[k] = np.where(blk, g[fr.OPP[k]], mad(omega, eq[k] - g[k], g[k]))
    assert out.dtype == f32 and usq.dtype == f32
    u = np.where(blk, f32(0.0), np.sqrt(usq) * densinv).astype(f64)
    inv = f32(1.0) / f32(np.count_nonzero(~blk))
    return out, f32(u.sum() * f64(inv))


def case(oracle_f32, oracle_f64, nx, ny, omega, density, state):
    """one case, computed once: inputs, the truth, the fp32 oracle's step and its figures"""
    key = (nx, ny, omega, density, state)
    if key not in _cache:
        ob, cells = fr.build_state(state, nx, ny, density)
        p = oracle_f32.make_params(nx, ny, 1, 10, density, 0.005, omega)
        oracle_f32.set_obstacles(p, ob)
        tr = fr.truth(oracle_f64, p, ob, cells, 1)
        ref = cells.copy()
        av = oracle_f32.run(p, ref, ob, 1)
        for a in (ob, cells, ref):
            a.setflags(write=False)
        _cache[key] = dict(p=p, ob=ob, cells=cells, tr=tr, ref=ref, av=av, orc=fr.measure(ref, tr, ob))
    return _cache[key]


def max_rel(a, b):
    return float(np.max(np.abs(a.astype(f64) - b.astype(f64)) / np.maximum(np.abs(b.astype(f64)), 1e-30)))


@pytest.mark.parametrize("nx,ny,omega,density,state", CASES)
def test_emulation_passes_every_gate(oracle_f32, oracle_f64, nx, ny, omega, density, state):
    """the stand-in is a correct fp32 statement in another order than the oracle's: every gate of the GPU module holds, and the
    oracle and the stand-in stay within half of av_bound"""
    c = case(oracle_f32, oracle_f64, nx, ny, omega, density, state)
    out, av = emulate_step(c["p"], c["ob"], c["cells"])
    got = fr.measure(out, c["tr"], c["ob"])
    what = "%dx%d om %.2f rho %g %s" % (nx, ny, omega, density, state)
    print(fr.line(what + " oracle", c["orc"]))
    print(fr.line(what + " emulation", got))
    gates = fr.check_gates(got, c["orc"])
    print("   rms ratio %.3f max ratio %.3f" % (got["rms"] / c["orc"]["rms"], got["max"] / c["orc"]["max"]))
    assert fr.blocked_equal(out, c["tr"], c["ob"]) and fr.blocked_equal(c["ref"], c["tr"], c["ob"])
    assert not fr.failed(gates), gates
    bound = fr.av_bound(c["tr"]["u"][0], c["tr"]["inv64"])
    d_orc, d_emu = abs(float(c["av"][0]) - c["tr"]["av"][0]), abs(float(av) - c["tr"]["av"][0])
    print("   av_vels: oracle off by %.2e, emulation by %.2e, bound %.2e" % (d_orc, d_emu, bound))
    assert d_orc <= 0.5 * bound and d_emu <= 0.5 * bound


@pytest.mark.parametrize("nx,ny,omega,density,state", CASES)
def test_conditions_on_the_inputs(oracle_f32, oracle_f64, nx, ny, omega, density, state):
    c = case(oracle_f32, oracle_f64, nx, ny, omega, density, state)
    assert np.all(c["cells"] > 0) and np.all(np.isfinite(c["ref"]))
    assert 0 < np.count_nonzero(c["ob"]) < c["ob"].size
    if state == "driven":
        assert fr.max_mach(c["cells"], c["ob"]) >= 0.25
        # one ulp of omega or of the reciprocal is several sigma of the fit
        assert c["orc"]["sa"] <= 0.1 and c["orc"]["sb"] <= 0.5, (c["orc"]["sa"], c["orc"]["sb"])
    # the inputs are of the kind the gates were measured on (the oracle measured <= 14.7)
    assert c["orc"]["max"] <= 16.0, c["orc"]["max"]


def test_near_rest_is_random_case():
    from test_gpu_parity import random_case
    ob, cells = fr.near_rest(np.random.default_rng(7), 33, 19, 0.1)
    ob2, cells2 = random_case(np.random.default_rng(7), 33, 19)
    assert np.array_equal(ob, ob2) and np.array_equal(cells, cells2)


@pytest.mark.parametrize("omega", [1.7, 1.99])
@pytest.mark.parametrize("nx,ny", [(64, 48), (260, 33), (33, 17), (128, 6), (256, 32), (33, 19)])
def test_emulation_passes_the_sixteen_step_gates(oracle_f32, oracle_f64, nx, ny, omega):
    """the shapes of the GPU module's sixteen-step runs: rms, max and the means against the oracle's, av_vels of every step of
    the oracle and of the stand-in within half of 16 av_bound"""
    ob, cells = fr.build_state("driven", nx, ny, 1.0)
    p = oracle_f32.make_params(nx, ny, 16, 10, 1.0, 0.005, omega)
    oracle_f32.set_obstacles(p, ob)
    tr = fr.truth(oracle_f64, p, ob, cells, 16)
    ref = cells.copy()
    av_ref = oracle_f32.run(p, ref, ob, 16)
    cur, av = cells, np.zeros(16)
    for t in range(16):
        cur, av[t] = emulate_step(p, ob, cur)
    got, orc = fr.measure(cur, tr, ob), fr.measure(ref, tr, ob)
    bounds = np.array([16.0 * fr.av_bound(u, tr["inv64"]) for u in tr["u"]])
    what = "16 steps %dx%d om %.2f" % (nx, ny, omega)
    print(fr.line(what + " oracle", orc))
    print(fr.line(what + " emulation", got))
    r_orc, r_emu = np.abs(av_ref - tr["av"]) / bounds, np.abs(av - tr["av"]) / bounds
    print("   rms ratio %.3f max ratio %.3f  av_vels / (16 av_bound): oracle %.3f emulation %.3f" % (
        got["rms"] / orc["rms"], got["max"] / orc["max"], r_orc.max(), r_emu.max()))
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(cur))
    assert not fr.failed(fr.check_gates(got, orc))
    assert r_orc.max() <= 0.5 and r_emu.max() <= 0.5


# defect -> the gates that have to fail, all of them
DEFECTS = {"w2+2": ("diag",), "w0-1": ("rest",), "omega+2": ("a",), "h3": ("b",), "rcp+4": ("b",), "swap68": ("max", "rms")}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
@pytest.mark.parametrize("omega", [0.6, 1.0])
@pytest.mark.parametrize("nx,ny", [(33, 19), (64, 48)])
def test_seeded_defect_fails_its_gate_and_passes_the_old_one(oracle_f32, oracle_f64, nx, ny, omega, defect):
    """omega 0.6 and 1.0: up to omega = 1 a relaxed value is a convex combination of two positive ones, so RTOL_CELLS, which is
    relative to each value, is well conditioned; above it values of this state cross zero and RTOL_CELLS refuses a correct
    kernel too (the stand-in without a defect is 7e-5 from the oracle at omega 1.7).
    Equilibria 6 and 8 swapped: max and rms fail by orders of magnitude.  The gates on the MEAN momentum error do not see the swap on
    this state: the error is 6 omega w2 (jx - jy) along (1, -1), and jx - jy has zero mean over cells with random velocities.  What
    sees it is the spread: the standard error of the momentum error is asserted to be 100 times the oracle's."""
    c = case(oracle_f32, oracle_f64, nx, ny, omega, 1.0, "driven")
    out, _ = emulate_step(c["p"], c["ob"], c["cells"], defect)
    got = fr.measure(out, c["tr"], c["ob"])
    gates = fr.check_gates(got, c["orc"])
    print(fr.line("%dx%d om %.2f %s" % (nx, ny, omega, defect), got))
    print("   failed: %s; against the oracle max_rel %.2e" % (fr.failed(gates), max_rel(out, c["ref"])))
    assert all(not gates[k][2] for k in DEFECTS[defect]), gates
    if defect == "swap68":
        assert got["momx"][1] > 100 * c["orc"]["momx"][1] and got["momy"][1] > 100 * c["orc"]["momy"][1]
    else:
        assert max_rel(out, c["ref"]) < RTOL_CELLS


@pytest.mark.parametrize("omega", [0.6, 1.7])
@pytest.mark.parametrize("nx,ny", [(33, 19), (64, 48)])
def test_collision_without_fused_multiply_adds(oracle_f32, oracle_f64, nx, ny, omega):
    """Every product of the collision rounded on its own.  Recorded, not gated: the unfused form's rms is 1.04 to 1.05 times the
    oracle's (the fused stand-in's: 1.01 to 1.03) -- the oracle rounds every product itself, and the products are few among the
    roundings of a cell -- so the rms gate of 1.25 does NOT see this change.  No gate was tuned until it did.  What the unfused
    form must still do is pass every gate, being a correct statement."""
    c = case(oracle_f32, oracle_f64, nx, ny, omega, 1.0, "driven")
    out, _ = emulate_step(c["p"], c["ob"], c["cells"], "nofma")
    fused, _ = emulate_step(c["p"], c["ob"], c["cells"])
    got, base = fr.measure(out, c["tr"], c["ob"]), fr.measure(fused, c["tr"], c["ob"])
    print(fr.line("%dx%d om %.2f nofma" % (nx, ny, omega), got))
    print("   rms: unfused %.3f fused %.3f oracle %.3f; rms gate sees it: %s" % (got["rms"], base["rms"], c["orc"]["rms"],
                                                                                   got["rms"] > fr.RMS_RATIO * c["orc"]["rms"]))
    assert not fr.failed(fr.check_gates(got, c["orc"]))


@pytest.mark.parametrize("nx,ny,omega,density,state", [k for k in CASES if k[4] == "driven"])
def test_reciprocal_within_one_ulp_passes(oracle_f32, oracle_f64, nx, ny, omega, density, state):
    """The hardware's documented accuracy at its worst, all to one side: on every cell the first fp32 above the exact
    reciprocal ("rcp_up": high by up to 1 ulp, 0.5 ulp in the mean) passes every gate and av_bound.
    The correctly rounded reciprocal moved up one place on every cell ("rcp+1") is off by up to 1.5 ulp, which is outside that
    accuracy: it passes rms, max, a, b and av_bound on every case (b comes out 1.25 to 1.83 above the clean value, inside the
    slack of 2), and the gates on the means on all but one -- 64x48, omega 0.6, density 1.0: the diagonal class mean moves by
    0.071 where 5 pooled standard errors are 0.064, since c = rho - h usq carries the reciprocal's error into every value.  The
    means have no slack for the reciprocal, so a reciprocal with a one-sided error of a whole ulp would be reported."""
    c = case(oracle_f32, oracle_f64, nx, ny, omega, density, state)
    bound = fr.av_bound(c["tr"]["u"][0], c["tr"]["inv64"])
    out, av = emulate_step(c["p"], c["ob"], c["cells"], "rcp_up")
    got = fr.measure(out, c["tr"], c["ob"])
    print(fr.line("%dx%d om %.2f rho %g rcp_up" % (nx, ny, omega, density), got))
    assert not fr.failed(fr.check_gates(got, c["orc"]))
    assert abs(float(av) - c["tr"]["av"][0]) <= bound
    out, av = emulate_step(c["p"], c["ob"], c["cells"], "rcp+1")
    got = fr.measure(out, c["tr"], c["ob"])
    gates = fr.check_gates(got, c["orc"])
    print(fr.line("%dx%d om %.2f rho %g rcp+1" % (nx, ny, omega, density), got))
    print("   rcp+1 failed: %s" % fr.failed(gates))
    assert all(gates[k][2] for k in ("rms", "max", "a", "b"))
    assert abs(float(av) - c["tr"]["av"][0]) <= bound


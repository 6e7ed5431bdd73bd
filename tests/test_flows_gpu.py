"""The fp64 families on two flows whose answer is known from outside the project (tests/_flows_ref.py): the place of a
bounce-back wall under two relaxation times, and the drag and lift of Schaefer and Turek's cylinder 2D-1 at Re = 20.

The other fp64 modules hold every kernel instance to a numpy restatement of include/lbm.h's statements bit for bit; a wrong
statement (a Zou-He coefficient, the link set or a sign of the force, the relation between omega_minus and Lambda) passes
them, because restatement and kernel share it.  Here the library's own long runs are gated on what the flow must give.  The
gates are tests/_flows_ref.py's (channel_gates, cylinder_gates, mirror_gates, finer_gates), which
tests/test_flows_restatement_cpu.py applies to the restatement's recorded figures in tests/golden/flows.json; the stop rule is
tests/_steady_rule.py's; and kernel and restatement are compared:
cells after the first 200 steps with np.array_equal, final figures with the fixture's to 1e-9 relative, force records with
the fixture's within 8 L 2^-53 sum|link terms| (the gate of test_force_gpu between two summation orders, L links).

Channel (32x11, 12 000 steps): one EnsembleDouble of four members omega 0.6, 1.0, 1.7, 1.9 per Lambda (3/16, 1/4), and three
LBMDouble contexts with BGK at omega 0.6 ("multistep" 0), 1.0 (8) and 1.7 (3).
Cylinder D = 10 (220x43, 40 000 steps, "force" on, the body the disc alone): an LBMDouble at "multistep" 8, one at 0 over the
first 2 000 steps, and a two-member EnsembleDouble whose member 1 is the mirrored case.  D = 20 (440x84): the fixture's 68 000
steps, after which the restatement's C_d moves by 0.2 % over 6 000 steps.

The steady stop.  The drag rings with the pressure wave between the velocity inlet, which reflects it like a closed end, and
the pressure outlet, an open end: a quarter-wave resonance, period 4 nx / c_s = 1 524 steps at nx = 220, measured 1 580 on
the record.  |F(s) - F(s - window)| is the swing times a factor that depends on the phase of the check points; with a window
that is no multiple of half the period that phase walks, and the run stops at the first check point where the factor
happens to be near zero (window 760, rel_tol 1e-3: step 12 920, where C_d still swings by a tenth).  WINDOW = 790 is half the
measured period: every check point has the same phase, the difference falls with the swing alone (1.3e-2 at 19 750, 2.1e-3
at 30 020, 1.8e-3 at 30 810), and REL_TOL = 2e-3 stops both members at 30 810.

Measured on the MI355X (figure, gate):
  channel, shape over omega 0.6 / 1.0 / 1.7 / 1.9     Lambda 3/16: 2.1723e-5 2.1265e-5 2.0994e-5 2.0965e-5, max / min 1.0362
                                                      Lambda 1/4:  4.2017e-3 4.2015e-3 4.2014e-3 4.2014e-3, max / min 1.0001
                                                      (gate: max / min <= 1.1; at 3/16 every shape <= 1e-4)
  shape at 1/4 over shape at 3/16, per omega          193.4 197.6 200.1 200.4 (gate >= 100)
  BGK, shape at omega 0.6 / 1.0 / 1.7                 7.0768e-2 4.2015e-3 1.2323e-2, max / min 16.84 (gate >= 10)
  shape at 1/4 against BGK's at omega 1, relative     6.0e-5 0 3.3e-5 1.4e-5 (gate 1e-3)
  spread, omega <= 1.7, all eleven runs               1.4e-13 .. 5.4e-13 (gate 1e-9); at omega 1.9 2.4e-8 and 8.7e-8, not gated
  every figure against the fixture's                  equal to the last digit (gate 1e-9 relative)
  cells after 200 steps, all runs and forms           np.array_equal with 200 restated steps
  force records against the restatement's             at most 0.001 of 8 L 2^-53 sum|link terms|: every one of the first 200
                                                      steps, and every 250th to the end (D 10: 40 000, D 20: 68 000)
  D 10, last 6 000 steps, "multistep" 8 and ensemble  C_d 5.8786, +5.35 % of 5.58 (gate 7 %); max - min 0.091 % (gate 0.2 %)
                                                      C_l 0.01252, +17.0 % of 0.0107 (gate 25 %, and positive)
  mirrored member                                     |C_d - C_d'| 0 (gate 8.9e-14), |C_l + C_l'| 1.4e-16 (gate 1.2e-13); the
                                                      gates are 100 x the restatement's 8.9e-16 and 1.2e-15, far below 1e-6 C_d
  D 20, last 6 000 of 68 000 steps                    C_d 5.7799, +3.58 % (gate: below D 10's 5.35 %, and 5 %); max - min
                                                      0.169 % (gate 0.2 %); C_l 0.01046 (published 0.0104 - 0.0110, not gated)
  run_until(on="drag"), window 790, rel_tol 2e-3      both members stop at 30 810, converged, as the rule on the plain record
                                                      says; C_d there 5.8837, +5.44 % (gate 7 %), C_l +0.01255 and -0.01255
The whole module takes 2 s, its longest test 0.5 s.
"""
import numpy as np
import pytest

import _flows_ref as flows
import _open_ref
import _trt_ref
from _flows_ref import (BGK_OMEGAS, L14, L316, channel_gates, channel_table, cylinder_gates, finer_gates, fixture, mirror_gates,
                        tail_of)
from _steady_rule import rule

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EARLY = 200
WINDOW, REL_TOL = 790, 2e-3
BGK_MULTISTEP = {0.6: 0, 1.0: 8, 1.7: 3}
_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def close(a, b):
    return abs(a - b) <= 1e-9 * abs(b)


# ---- channel -------------------------------------------------------------------------------------------------------------

def channel_restated(omega, magic):
    """the state after EARLY restated steps from rest"""
    def make():
        ob, u_in = flows.channel_mask(), _open_ref.poiseuille(flows.CH_NY, flows.CH_U)
        om = None if magic is None else _trt_ref.omega_minus(omega, magic)
        f = _open_ref.rest_state(flows.DENSITY, flows.CH_NY, flows.CH_NX).copy()
        for _ in range(EARLY):
            f = _open_ref.step(f, ob, omega, om, u_in, flows.DENSITY)[0]
        return f
    return once(("channel restated", omega, magic), make)


def channel_runs(lbm, magic):
    """{omega: (cells after EARLY steps, cells after CH_STEPS)}: magic None = the three BGK contexts, else one ensemble"""
    def make():
        ob, u_in = flows.channel_mask(), _open_ref.poiseuille(flows.CH_NY, flows.CH_U)
        base = lbm.make_dparams(flows.CH_NX, flows.CH_NY, flows.CH_STEPS, density=flows.DENSITY, accel=0.005, omega=1.0, obstacles=ob)
        out = {}
        if magic is None:
            for omega, p in zip(BGK_OMEGAS, lbm.sweep_dparams(base, omega=list(BGK_OMEGAS))):
                with lbm.LBMDouble(p, ob) as sim:
                    sim.set_option("multistep", BGK_MULTISTEP[omega])
                    sim.set_open(u_in, flows.DENSITY)
                    assert sim.trt() == (0.0, omega)
                    sim.upload(None)
                    sim.run(EARLY)
                    early = sim.download(av_vels=False)[0]
                    sim.run(flows.CH_STEPS - EARLY)
                    out[omega] = (early, sim.download(av_vels=False)[0])
            return out
        with lbm.EnsembleDouble(lbm.sweep_dparams(base, omega=list(flows.CH_OMEGAS)), ob) as ens:
            ens.set_trt([magic] * 4)
            ens.set_open(u_in, flows.DENSITY)
            assert ens.trt()[1].tolist() == [_trt_ref.omega_minus(w, magic) for w in flows.CH_OMEGAS]
            ens.upload(None)
            ens.run(EARLY)
            early = ens.download(av_vels=False)[0]
            ens.run(flows.CH_STEPS - EARLY)
            assert ens.steps_done == flows.CH_STEPS
            last = ens.download(av_vels=False)[0]
        return {w: (early[m], last[m]) for m, w in enumerate(flows.CH_OMEGAS)}
    return once(("channel", magic), make)


@pytest.mark.parametrize("magic", [L316, L14, None], ids=["3/16", "1/4", "BGK"])
def test_channel_equals_the_restatement(lbm, magic):
    table = channel_table(fixture())
    for omega, (early, last) in channel_runs(lbm, magic).items():
        assert np.array_equal(early, channel_restated(omega, magic)), omega
        spread, shape = _open_ref.channel_figures(last, flows.CH_U)
        want_spread, want_shape = table[(magic, omega)]
        print("omega %.1f: shape %.17e (fixture %.17e) spread %.17e (fixture %.17e)" % (omega, shape, want_shape, spread, want_spread))
        assert close(shape, want_shape) and close(spread, want_spread), omega


def test_channel_wall_stays_with_two_relaxation_times_and_moves_with_one(lbm):
    fig = {}
    for magic in (L316, L14, None):
        for omega, (_, last) in channel_runs(lbm, magic).items():
            fig[(magic, omega)] = _open_ref.channel_figures(last, flows.CH_U)
    assert len(fig) == 11
    print("\n".join(channel_gates(fig)))


# ---- cylinder ------------------------------------------------------------------------------------------------------------

def cylinder_restated(mirror):
    """EARLY restated steps of the D = 10 case from rest: (state, F_x[EARLY], F_y[EARLY], sum|link terms|[EARLY], links)"""
    def make():
        case = flows.cylinder_channel(10)
        if mirror:
            case = flows.mirrored(case)
        f = flows.rest(case)
        rec = np.zeros((3, EARLY))
        for t in range(EARLY):
            rec[0, t], rec[1, t], links, rec[2, t] = flows.force(f, case)
            f = flows.step(f, case)
        return f, rec[0], rec[1], rec[2], links
    return once(("cylinder restated", mirror), make)


def params_of(lbm, case, steps):
    return lbm.make_dparams(case["nx"], case["ny"], steps, density=case["density"], accel=0.005, omega=case["omega"],
                            obstacles=case["ob"])


def context_run(lbm, D, multistep, steps):
    """an LBMDouble on the case: cells after EARLY steps, the record of `steps` steps and force() after them"""
    def make():
        case = flows.cylinder_channel(D)
        with lbm.LBMDouble(params_of(lbm, case, steps), case["ob"]) as sim:
            sim.set_option("multistep", multistep)
            sim.set_option("force", 1)
            sim.set_body(case["body"])
            sim.set_trt(case["magic"])
            sim.set_open(case["u_in"], case["rho_out"])
            assert sim.trt() == (case["magic"], case["omega_m"])
            sim.upload(None)
            sim.run(EARLY)
            early = sim.download(av_vels=False)[0]
            sim.run(steps - EARLY)
            fx, fy = sim.force_record()
            return {"early": early, "fx": fx, "fy": fy, "now": sim.force()}
    return once(("context", D, multistep, steps), make)


def pair_of(lbm, steps):
    """the two-member ensemble: member 0 the D = 10 case, member 1 its mirror image"""
    case = flows.cylinder_channel(10)
    mirror = flows.mirrored(case)
    ens = lbm.EnsembleDouble(lbm.sweep_dparams(params_of(lbm, case, steps), omega=[case["omega"]] * 2),
                             np.stack([case["ob"], mirror["ob"]]))
    ens.set_option("force", 1)
    ens.set_body(np.stack([case["body"], mirror["body"]]))
    ens.set_trt(case["magic"])
    ens.set_open(np.stack([case["u_in"], mirror["u_in"]]), case["rho_out"])
    ens.upload(None)
    return ens


def pair_run(lbm):
    def make():
        steps = fixture()["cylinder"]["10"]["steps"]
        with pair_of(lbm, steps) as ens:
            ens.run(EARLY)
            early = ens.download(av_vels=False)[0]
            ens.run(steps - EARLY)
            fx, fy = ens.force_record()
            return {"early": early, "fx": fx, "fy": fy, "now": ens.force()}
    return once("pair", make)


def d10_run(lbm, form):
    """early cells, record and force() of member 0 in the three forms, and the steps the form runs"""
    steps = fixture()["cylinder"]["10"]["steps"]
    if form == "ensemble":
        r = pair_run(lbm)
        return {"early": r["early"][0], "fx": r["fx"][0], "fy": r["fy"][0], "now": (r["now"][0][0], r["now"][1][0])}, steps
    if form == "multistep 0":
        return context_run(lbm, 10, 0, 2000), 2000
    return context_run(lbm, 10, 8, steps), steps


FORMS = ["multistep 8", "multistep 0", "ensemble"]


def assert_record_meets_the_fixture(run, fix, steps):
    """every sampled entry of the record, and force() after the run, within the sibling gate of the fixture's"""
    every, links = fix["every"], fix["links"]
    assert run["fx"].shape == run["fy"].shape == (steps,) and steps % every == 0 and steps <= fix["steps"]
    worst = 0.0
    for i in range(steps // every + 1):
        t = i * every
        gx, gy = (run["fx"][t], run["fy"][t]) if t < steps else run["now"]
        tol = 8.0 * links * U * fix["mag"][i]
        worst = max(worst, abs(gx - fix["fx"][i]) / tol, abs(gy - fix["fy"][i]) / tol)
        assert abs(gx - fix["fx"][i]) <= tol and abs(gy - fix["fy"][i]) <= tol, (t, gx, fix["fx"][i], gy, fix["fy"][i], tol)
    return worst


@pytest.mark.parametrize("form", FORMS)
def test_cylinder_equals_the_restatement(lbm, form):
    fix = fixture()["cylinder"]["10"]
    run, steps = d10_run(lbm, form)
    state, rx, ry, mag, links = cylinder_restated(False)
    assert links == fix["links"] == 94
    assert np.array_equal(run["early"], state)
    worst = 0.0
    for t in range(EARLY):
        tol = 8.0 * links * U * mag[t]
        worst = max(worst, abs(run["fx"][t] - rx[t]) / tol, abs(run["fy"][t] - ry[t]) / tol)
        assert abs(run["fx"][t] - rx[t]) <= tol and abs(run["fy"][t] - ry[t]) <= tol, (t, run["fx"][t], rx[t], run["fy"][t], ry[t], tol)
    sampled = assert_record_meets_the_fixture(run, fix, steps)
    assert steps >= 2000
    print("%s: cells after %d steps equal; record against the restatement's, largest share of the gate: %.3f over the first %d "
          "steps, %.3f over the fixture's samples to step %d" % (form, EARLY, worst, EARLY, sampled, steps))
    if form != "multistep 8":
        ref = context_run(lbm, 10, 8, fix["steps"])                      # one record whatever the form
        assert np.array_equal(run["fx"], ref["fx"][:steps]) and np.array_equal(run["fy"], ref["fy"][:steps])


def test_mirrored_member_equals_the_restatement(lbm):
    r = pair_run(lbm)
    state, rx, ry, mag, links = cylinder_restated(True)
    assert links == 94 and np.array_equal(r["early"][1], state)
    for t in range(EARLY):
        tol = 8.0 * links * U * mag[t]
        assert abs(r["fx"][1][t] - rx[t]) <= tol and abs(r["fy"][1][t] - ry[t]) <= tol, t
    assert not np.array_equal(r["early"][1], r["early"][0])


@pytest.mark.parametrize("form", ["multistep 8", "ensemble"])
def test_cylinder_drag_and_lift_are_the_benchmarks(lbm, form):
    run, steps = d10_run(lbm, form)
    assert steps == 40000
    print("%s: %s" % (form, cylinder_gates(tail_of(run["fx"], run["fy"], 10))))


def test_mirrored_member_has_the_same_drag_and_the_opposite_lift(lbm):
    r = pair_run(lbm)
    t0, t1 = tail_of(r["fx"][0], r["fy"][0], 10), tail_of(r["fx"][1], r["fy"][1], 10)
    assert t1["cl_mean"] < 0.0 < t0["cl_mean"]
    print(mirror_gates(t0, t1, fixture()["cylinder"]["10"]["mirrored"]))


def test_finer_cylinder_comes_closer(lbm):
    fix = fixture()["cylinder"]["20"]
    steps = fix["steps"]
    run = context_run(lbm, 20, 8, steps)
    worst = assert_record_meets_the_fixture(run, fix, steps)
    t20 = tail_of(run["fx"], run["fy"], 20)
    swing = (t20["cd_max"] - t20["cd_min"]) / t20["cd_mean"]
    print("D 20 after %d steps: max - min of C_d %.3f %% (gate 0.2 %%); record against the fixture, largest share of the gate %.3f"
          % (steps, 100.0 * swing, worst))
    assert swing <= 2e-3
    t10 = tail_of(*[context_run(lbm, 10, 8, 40000)[k] for k in ("fx", "fy")], 10)
    print(finer_gates(t20, t10))


def test_steady_stop_on_drag(lbm):
    plain = pair_run(lbm)
    cap = plain["fx"].shape[1]
    want_steps, want_conv = rule(plain["fx"], 0, cap, WINDOW, REL_TOL)
    print("window %d rel_tol %g: stops %s converged %s" % (WINDOW, REL_TOL, want_steps.tolist(), want_conv.tolist()))
    assert np.all(want_steps > 20000) and np.all(want_steps < cap) and want_conv.all()     # conditions on the plain record
    with pair_of(lbm, cap) as ens:
        steps, conv = ens.run_until(cap, window=WINDOW, rel_tol=REL_TOL, on="drag")
        fx, fy = ens.force_record()
    assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
    for m in range(2):
        c = int(steps[m])
        assert np.array_equal(fx[m, :c], plain["fx"][m, :c]) and np.array_equal(fy[m, :c], plain["fy"][m, :c]), m
        cd, cl = flows.coefficients(fx[m, c - 1], fy[m, c - 1], 10)
        print("member %d stopped at %d: C_d %.4f (%+.2f %% of 5.58, gate 7 %%), C_l %+.5f" % (m, c, cd, 100.0 * (cd / flows.CD_PUBLISHED - 1.0), cl))
        assert abs(cd - flows.CD_PUBLISHED) <= 0.07 * flows.CD_PUBLISHED

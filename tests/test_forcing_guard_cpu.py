"""Conditions on the inputs of tests/test_forcing_guard_gpu.py, checked on the CPU oracle alone.

The forcing guard is discontinuous: a kernel may only be compared with the oracle on a state whose guard margins are wide,
and only while the state stays finite.  For every case the GPU file uses (tests/_guard_case.py: CASES, run for the longest
step count any test runs on it) this file asserts, on the oracle:
  * every value is finite, and below 10 x density, after every step;
  * at every step at least 8 free cells of the forcing row are refused and at least 8 accepted;
  * each of the three clauses is the only one to refuse in some cell at step 0 and again at one of steps 1..7 (one launch of the
    deep kernel sees all three);
  * the smallest relative guard margin |f - aw| / aw is at least 1e-4 at every step, in every oracle form;
  * the fp32 oracle in both forms (pairwise momenta without FMA contraction, the Makefile's; left-to-right momenta with
    contraction) and the fp64 oracle decide the same cells at every step;
  * refused and accepted cells share a lane pair (2i, 2i+1), and both occur on either side of x = 0, at step 0 and again at one
    of steps 1..7; where nx is no multiple of 256 both occur in the partly filled last wave.
  * after the last step the fp32 oracle's two forms are within SPREAD_MAX of the fp64 oracle: the state does not amplify rounding.
These are conditions, not measurements: a case that misses one gets another seed or another state, never another bound."""
import numpy as np
import pytest

import _guard_case as G


@pytest.fixture(scope="module")
def oracles(oracle_f32_omp, oracle_f64_omp, tmp_path_factory):
    return {"fp32 oracle": oracle_f32_omp,
            "fp32 oracle, left-to-right momenta and FMA contraction": G.oracle_form(tmp_path_factory.mktemp("oracle_forms"), "f32", 0, "fast"),
            "fp64 oracle": oracle_f64_omp}


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_meets_the_conditions(oracles, name):
    nx, ny, nsteps, _ = G.CASES[name]
    density, accel, omega, ob, cells0 = G.case(name, real=np.float64 if name in G.DOUBLE_CASES else np.float32)
    runs = {label: G.guard_audit(orc, density, accel, omega, ob, cells0, nsteps, keep=(nsteps,)) for label, orc in oracles.items()}
    audits = {label: r[0] for label, r in runs.items()}
    ref = runs["fp64 oracle"]
    spread = max(max(G.plane_norm(r[1][nsteps], ref[1][nsteps]), G.plane_norm(r[2], ref[2])) for r in runs.values())
    first = audits["fp32 oracle"]
    print("%s, %d steps: refused per step %s; refusing alone f3 / f6 / f7 %s; smallest margin %.2e" %
          (name, nsteps, [int(s["refused"].sum()) for s in first], [[s["sole"][k] for s in first] for k in G.CLAUSES],
           min(s["margin"] for a in audits.values() for s in a)))
    print("fp32 forms against the fp64 oracle after %d steps: %.2e of a plane's mean" % (nsteps, spread))
    assert G.conditions(nx, audits, density, nsteps) == []
    assert spread <= G.SPREAD_MAX


def test_thresholds_are_off_the_defaults_and_the_plain_cases_never_refuse():
    """what the case is for: on the perturbed rest state of the other tests the guard accepts every free cell"""
    from oracle.oracle import Oracle
    orc = Oracle("f32")
    rng = np.random.default_rng(1)
    nx, ny = 260, 33
    ob = (rng.random((ny, nx)) < 0.08).astype(np.int32)
    cells = (G.W * 0.1 * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5))).astype(np.float32)
    steps, _, _ = G.guard_audit(orc, 0.1, 0.01, 1.85, ob, cells, 11)
    assert all(not s["refused"].any() for s in steps)
    assert (G.DENSITY, G.ACCEL, G.OMEGA) != (0.1, 0.005, 1.85)


def test_gated_ensemble_tolerance_stops_some_members_early(oracle_f32_omp):
    """the window and tolerance of test_gated_ensemble_members, on the oracle's records: at the first check point some guard
    member has settled and another has not, each at least 5 % away from the tolerance"""
    GATE_MAX_STEPS, GATE_TOL, GATE_WINDOW = G.GATE_MAX_STEPS, G.GATE_TOL, G.GATE_WINDOW
    s = 2 * GATE_WINDOW
    change = []
    for name in G.MEMBERS:
        density, accel, omega, ob, cells0 = G.case(name)
        av = G.guard_audit(oracle_f32_omp, density, accel, omega, ob, cells0, GATE_MAX_STEPS)[2].astype(np.float64)
        change.append(abs(av[s - 1] - av[s - GATE_WINDOW - 1]) / abs(av[s - 1]))
    print("change over %d steps at step %d: %s" % (GATE_WINDOW, s, ["%.3f" % c for c in change]))
    assert any(c < 0.95 * GATE_TOL for c in change) and any(c > 1.05 * GATE_TOL for c in change)
    assert all(abs(c / GATE_TOL - 1.0) > 0.05 for c in change)

"""tests/_scalar_ref.py, the numpy restatement of the passive scalar (include/lbm.h, "Scalar transport"), held to what the GPU
tests hold the device to, as far as that is cheap on a CPU, and tests/golden/scalar.json held to the restatement and to the gates.

  - the restatement's pieces: the rest state sums to c0, a uniform field under any velocity stays uniform (an insulating wall and a
    wall held at that value included), a blocked cell is copied through, accelerate() is the oracle's accelerate_flow bit for bit;
  - the cheap runs (conservation, the three diffusion runs) recomputed in full meet their gates and equal the fixture's figures;
  - the first 200 steps of every fixture run, recomputed, give the fixture's probe to 1e-12;
  - every gate, applied to the fixture's figures."""
import json
import os

import numpy as np
import pytest

import _scalar_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fix():
    with open(os.path.join(GOLDEN, "scalar.json")) as f:
        return json.load(f)


def entry_of(fix, kind, D):
    (e,) = [e for e in fix["entries"] if e["kind"] == kind and (D is None or e["D"] == D)]
    return e


def test_the_fixture_holds_the_runs_and_their_settings(fix):
    assert [(e["kind"], e["D"]) for e in fix["entries"]] == [(k, ref.case(k, D).D) for k, D in ref.RUNS]
    assert fix["start_steps"] == ref.START
    settings = json.loads(json.dumps({"conservation": ref.CONSERVATION, "diffusion": ref.DIFFUSION, "walls": ref.WALLS,
                                      "open": ref.OPEN, "taylor": ref.TAYLOR}))
    assert fix["settings"] == settings
    assert [e["steps"] for e in fix["entries"] if e["kind"] == "walls"] == [102400, 20480, 12288, 6827]


def test_the_pieces():
    rng = np.random.default_rng(5)
    ny, nx = 9, 11
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    ob[4, 3:6] = 1
    c0 = 0.5 + rng.random((ny, nx))
    g = ref.init(c0)
    assert np.allclose(ref.field(g, np.zeros_like(ob)), c0, rtol=4e-16, atol=0.0)
    assert not np.any(ref.field(g, ob)[ob != 0])
    u_x, u_y = 0.1 * (rng.random((ny, nx)) - 0.5), 0.1 * (rng.random((ny, nx)) - 0.5)
    # a uniform field stays uniform under any velocity: beside insulating walls, and beside walls held at its own value
    for wall in (None, np.where(rng.random((ny, nx)) < 0.5, np.nan, 0.7)):
        out = ref.step(ref.init(np.full((ny, nx), 0.7)), ob, u_x * 0, u_y * 0, ref.omega_s(0.05), wall)
        assert np.max(np.abs(ref.field(out, ob)[ob == 0] - 0.7)) <= 4e-16
    # blocked cells are copied through; insulating walls conserve the sum over the fluid cells
    out = ref.step(g, ob, u_x, u_y, ref.omega_s(0.05))
    assert np.array_equal(out[:, ob != 0], g[:, ob != 0])
    assert abs(ref.total(ref.field(out, ob), ob) / ref.total(c0, ob) - 1.0) <= 1e-15
    # open ends: the inlet cell carries c_in, the outlet gathers its own g[3]
    free = np.zeros_like(ob)
    c_in = 0.5 + rng.random(ny)
    out = ref.step(g, free, u_x * 0, u_y * 0, ref.omega_s(1.0 / 6.0), None, c_in)        # omega_s = 1: the result is the equilibrium
    assert np.allclose(ref.field(out, free)[:, 0], c_in, rtol=1e-15, atol=0.0)


def test_accelerate_is_the_oracles():
    from oracle.oracle import Oracle
    from _dp_states import random_state
    from _force_ref import accelerated
    from types import SimpleNamespace
    orc = Oracle("f64")
    ny, nx = 12, 13
    f = random_state(np.random.default_rng(3), 0.1, ny, nx)
    f[3, ny - 2, 4] = 1e-6                                      # a cell the guard refuses
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[ny - 2, 6:8] = 1
    p = SimpleNamespace(nx=nx, ny=ny, max_iters=1, reynolds_dim=10, density=0.1, accel=0.005, omega=1.0, free_cells_inv=1.0)
    want = accelerated(orc, p, ob, f)
    got = ref.accelerate(f, ob, 0.1, 0.005)
    assert np.array_equal(got, want) and not np.array_equal(got, f)
    assert np.array_equal(got[:, ny - 2, 4], f[:, ny - 2, 4])


@pytest.mark.parametrize("kind,D", [r for r in ref.RUNS if r[0] in ("conservation", "diffusion")])
def test_cheap_runs_meet_their_gates_and_the_fixture(fix, kind, D):
    cs = ref.case(kind, D)
    _, seen, _ = ref.run(cs)
    fig = ref.figures(kind, cs, seen)
    stored = entry_of(fix, kind, D)
    ref.gates(kind, fig, stored)
    for key, value in fig.items():
        assert value == stored[key], (key, value, stored[key])


@pytest.mark.parametrize("kind,D", ref.RUNS)
def test_first_steps_of_every_fixture_run(fix, kind, D):
    cs = ref.case(kind, D)
    got = ref.probe(ref.run(cs, steps=ref.START, spin_up=0)[2])
    want = entry_of(fix, kind, D)["start"]
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-12 * max(abs(b), 1.0), (kind, D, got, want)


def test_every_gate_on_the_fixture(fix):
    for e in fix["entries"]:
        ref.gates(e["kind"], e, e)
    t = entry_of(fix, "taylor", None)
    assert t["parabola_deviation"] <= ref.TAYLOR["parabola_gate"]
    # the prototype of the issue gave 0.985 of theory and a centre speed of 0.0501
    assert 0.95 <= t["d_eff_ratio"] <= 1.05 and 0.99 <= t["speed_ratio"] <= 1.01

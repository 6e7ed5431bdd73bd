"""The reference of the output-stage tests, held to the fp64 oracle, and the spreads their GPU gates are built from.

1. fields() of tests/_fields_ref.py (numpy float64, written from the formulas) agrees with the fp64 oracle's final_fields,
   reynolds and total_density to 1e-13 relative on three states advanced 40 steps by the fp64 oracle.
2. For every case of tests/test_output_stage_gpu.py: how far the fp32 oracle's own output arithmetic lands from fields() on the
   state the fp32 oracle has advanced as far as the GPU test runs it (u_x, u_y, u as max absolute error over the case's largest
   speed; Reynolds number and av_vels relative).  The GPU gates are GATE_FACTOR = 4 times these, so every spread must be a
   usable gate: positive, far below the 1e-4 the suite held av_vels to before, and — for av_vels — small enough that one lost
   or doubled average cell is at least two gates (ncells * gate < 0.5).

Measured here (pytest -s prints every case): u_x, u_y, u 5.5e-7 .. 2.2e-6 after 9 steps (the ragged ensemble after 208 .. 400
steps: up to 4.2e-6); Reynolds number 3e-9 .. 8.5e-6; av_vels 2.3e-8 (256x37, 4 steps) .. 2.7e-6 (3x3); the ragged channel sweep
stops at 208 / 304 / 400 / 400 steps on the fp32 oracle.  The largest ncells * gate is 0.012 (1024x50)."""
import numpy as np
import pytest

import _fields_ref as F
from _guard_case import oracle_form
from conftest import input_files


@pytest.fixture(scope="module")
def f32_forms(oracle_f32_omp, tmp_path_factory):
    """the fp32 oracle of the Makefile and its other honest form (momenta left to right, FMA contraction on)"""
    return oracle_f32_omp, oracle_form(tmp_path_factory.mktemp("oracle_forms"), "f32", 0, "fast")


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))


@pytest.mark.parametrize("name", ["30x17", "132x40", "128x128 shipped"])
def test_fields_ref_agrees_with_the_fp64_oracle(oracle_f64_omp, name):
    orc = oracle_f64_omp
    if name.endswith("shipped"):
        p, ob = orc.load(*input_files("128x128"))
        cells = orc.init_cells(p)
    else:
        nx, ny = (int(v) for v in name.split("x"))
        ob, cells = F.state(nx, ny, nx + ny, real=np.float64)
        ob[ny // 2, :] = (np.random.default_rng(nx).random(nx) < 0.08)      # random obstacles only: flow through every row
        p = orc.make_params(nx, ny, 40, F.REYNOLDS_DIM, F.DENSITY, F.ACCEL, F.OMEGA)
        orc.set_obstacles(p, ob)
    orc.run(p, cells, ob, 40)
    ref = F.fields(cells, ob, p.density, p.omega, p.reynolds_dim)
    ux, uy, u, pr = orc.final_fields(p, cells, ob)
    free = ob == 0
    top = F.max_speed(ref)
    # velocities: absolute over the largest speed (a relative error means nothing next to a zero crossing)
    for got, k in ((ux, "u_x"), (uy, "u_y"), (u, "u")):
        assert np.max(np.abs(got - ref[k])) <= 1e-13 * top, k
        assert np.all(got[~free] == 0.0)
    assert rel(pr, ref["pressure"]) <= 1e-13
    assert np.all(pr[~free] == p.density / 3.0) or rel(pr[~free], p.density / 3.0) <= 1e-15
    assert abs(orc.reynolds(p, cells, ob) / ref["reynolds"] - 1.0) <= 1e-13
    assert abs(orc.av_velocity(p, cells, ob) / ref["mean_u"] - 1.0) <= 1e-13
    # total density: the oracle adds 9 nx ny terms one after the other, which alone costs up to n 2^-53 (7.7e-13 on the
    # shipped input, where the exact sum is known: 128 * 128 * 0.1); the 1e-13 holds against the same sum in the same order,
    # and fields()' pairwise sum lies within that bound of both
    serial = float(np.cumsum(cells.ravel())[-1])
    assert abs(orc.total_density(p, cells) / serial - 1.0) <= 1e-13
    assert abs(serial / ref["total_density"] - 1.0) <= cells.size * 2.0 ** -53
    assert top > 1e-3 and np.count_nonzero(~free) > 0


def show(what, s):
    print("spread %-28s u_x %.3e  u_y %.3e  u %.3e  Re %.3e  av_vels %.3e" %
          (what, s["u_x"], s["u_y"], s["u"], s["reynolds"], s["av"]))


def usable(s, ncells=None):
    for k in ("u_x", "u_y", "u"):
        assert 0.0 < s[k] < 2e-5, k          # a few fp32 roundings of a momentum over the case's largest speed
    assert 0.0 <= s["reynolds"] < 1e-3        # the oracle sums the speeds serially in fp32
    assert 0.0 < s["av"] < 1e-5
    if ncells is not None:
        assert ncells * F.gates(s)["av"] < 0.5


FIELD_CASES = dict(F.ONE_SLAB, **F.SLABS)


@pytest.mark.parametrize("name", list(FIELD_CASES))
def test_spreads_of_the_field_cases(f32_forms, name):
    s = F.oracle_spreads(f32_forms, FIELD_CASES[name], F.FIELD_STEPS)
    show(name, s)
    usable(s)


@pytest.mark.parametrize("name", list(F.ENSEMBLES))
def test_spreads_of_the_ensemble_members(f32_forms, name):
    for m, c in enumerate(F.ENSEMBLES[name]):
        s = F.oracle_spreads(f32_forms, c, F.FIELD_STEPS)
        show("%s member %d" % (name, m), s)
        usable(s, c["nx"] * c["ny"])


def test_spreads_of_the_ragged_ensemble(f32_forms):
    """the channel sweep from rest, every member at the count the steady-run rule stops it at on the fp32 oracle's own record"""
    from test_steady_gpu import rule
    r = F.RAGGED
    ob = F.ragged_channel(r["nx"], r["ny"])
    stops = []
    for omega in r["omegas"]:
        c = F.case(r["nx"], r["ny"], 0, density=r["density"], omega=omega, reynolds_dim=r["reynolds_dim"], accel=r["accel"])
        cells0 = np.ascontiguousarray(np.broadcast_to(F.W * r["density"], (9, r["ny"], r["nx"])).astype(np.float32))
        record = np.array([av for _, av, _ in F.oracle_steps(f32_forms[0], c, ob, cells0, r["max_steps"])], dtype=np.float32)
        steps, _ = rule(record[None], 0, r["max_steps"], r["window"], r["rel_tol"])
        stops.append(int(steps[0]))
        s = F.oracle_spreads(f32_forms, c, stops[-1], ob, cells0, av_window=r["window"])
        show("ragged omega %.1f, %d steps" % (omega, stops[-1]), s)
        usable(s, r["nx"] * r["ny"])
    print("ragged ensemble stops on the fp32 oracle:", stops)
    assert len(set(stops)) > 1


@pytest.mark.parametrize("name", list(F.AV_SINGLE) + list(F.AV_CASES))
def test_spreads_of_the_av_vels_cases(f32_forms, name):
    c, nsteps = (F.AV_SINGLE.get(name) or F.AV_CASES[name])
    for n in sorted({nsteps, 4, 6} if name in ("256x37", "256x67 / 4") else {nsteps}):
        s = F.oracle_spreads(f32_forms, c, n)
        show("%s, %d steps" % (name, n), s)
        usable(s, c["nx"] * c["ny"])

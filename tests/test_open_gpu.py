"""Open boundaries on the GPU (lbm_dopen_*, LBMDouble / EnsembleDouble .set_open() and .open()): a velocity inlet on column
0 and a pressure outlet on column nx - 1.

The reference is tests/_open_ref.py: include/lbm.h's statements in numpy float64 on top of tests/_trt_ref.py, held to what is
known without a GPU by tests/test_open_restatement_cpu.py.  Gates:
  1. cells after a step against the restatement of the state before it (downloaded; no accelerate_flow): np.array_equal.
     av_vels against the restatement's sum|u| * free_cells_inv within N 2^-53 sum|u|, the bound between two summation orders
     of N terms.  The force record against _open_ref.force (the column rule of lbm.h) within test_force_gpu's gate,
     8 L 2^-53 sum|link terms|;
  2. - 6. bit identity (np.array_equal), stop counts and error codes: no tolerance;
  7. the channel check of tests/test_open_restatement_cpu.py at "multistep" 8, the same gates.
Shapes: 16x16 (one tile, nx even), 33x19 (nx odd, ragged tiles), 48x35 (3x3 tiles: the end tiles hold the opposite column in
their halo), 5x4 (the region of every tile form is wider than nx and holds column 0 more than once; no walls)."""
import ctypes

import numpy as np
import pytest

import _open_ref
import _trt_ref
from _dp_states import RUNS, random_state
from _force_ref import accelerated, block_body
from _steady_rule import CAP, OMEGAS, TOL, rule, sweep

pytestmark = pytest.mark.gpu

LBM_ERR_ARG, LBM_ERR_STATE = 1, 3
U = 2.0 ** -53
MAGIC = 3.0 / 16.0
SHAPES = [(16, 16), (33, 19), (48, 35), (5, 4)]
SINGLE_STEPS = 6
RHO_OUT = 0.102
SPLITS = RUNS[:11] + [400 - sum(RUNS[:11])]      # 1, 1, 9, 2..8, 20 and the tail: 400 steps


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def open_mask(nx, ny):
    """(obstacles, body or None).  16x16: walls and a body.  33x19: walls, a body and a blocked cell inside column 0.  48x35:
    walls, a body and a blocked cell inside column nx - 1.  5x4: nothing blocked, no walls."""
    ob = np.zeros((ny, nx), dtype=np.int32)
    if (nx, ny) == (5, 4):
        return ob, None
    ob[0] = ob[ny - 1] = 1
    body = np.zeros_like(ob)
    body[ny // 2 - 2:ny // 2 + 2, nx // 4:nx // 4 + 5] = 1
    ob |= body
    if (nx, ny) == (33, 19):
        ob[5, 0] = 1
        assert not ob[4, 0] and not ob[6, 0] and not ob[5, 1] and not ob[5, nx - 1]
    if (nx, ny) == (48, 35):
        ob[7, nx - 1] = 1
        assert not ob[6, nx - 1] and not ob[8, nx - 1] and not ob[7, nx - 2] and not ob[7, 0]
    return ob, body


def profile(nx, ny, seed=0, scale=1.0):
    """an inlet profile that differs from row to row: the parabola between the walls (5x4: a flat one) times 1 +- 5 %"""
    rng = np.random.default_rng(1000 * nx + ny + seed)
    base = np.full(ny, 0.03) if (nx, ny) == (5, 4) else _open_ref.poiseuille(ny, 0.04)
    return scale * base * (1.0 + 0.1 * (rng.random(ny) - 0.5))


def open_case(lbm, nx, ny, max_iters, omega=1.7):
    ob, body = open_mask(nx, ny)
    p = lbm.make_dparams(nx, ny, max_iters, density=0.1, accel=0.005, omega=omega, obstacles=ob)
    return p, ob, body, random_state(np.random.default_rng(11 + nx), 0.1, ny, nx), profile(nx, ny)


# ---- 1. single steps against the restatement ---------------------------------------------------------------------------

_single = {}


def trt_of(nx, ny, multistep):
    """BGK and TRT alternate over the twelve cases: every shape and every form sees both"""
    return (SHAPES.index((nx, ny)) + [0, 3, 8].index(multistep)) % 2 == 1


def single_steps(lbm, nx, ny, multistep):
    key = (nx, ny, multistep)
    if key not in _single:
        p, ob, body, cells0, u_in = open_case(lbm, nx, ny, SINGLE_STEPS)
        states = []
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("multistep", multistep)
            sim.set_option("force", 1)
            if body is not None and multistep != 3:          # multistep 3: every blocked cell, the walls included
                sim.set_body(body)
            if trt_of(nx, ny, multistep):
                sim.set_trt(MAGIC)
            sim.set_open(u_in, RHO_OUT)
            sim.upload(cells0)
            for _ in range(SINGLE_STEPS):
                states.append(sim.download(av_vels=False)[0])
                now = sim.force()
                sim.run(1)
                assert now == tuple(v[-1] for v in sim.force_record())     # the output stage: the entry the step writes
            cells, av = sim.download()
            states.append(cells)
            fx, fy = sim.force_record()
        _single[key] = (p, ob, body if multistep != 3 else None, u_in, states, av, fx, fy)
    return _single[key]


@pytest.mark.parametrize("multistep", [0, 3, 8])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_single_steps_equal_the_restatement_bit_for_bit(lbm, oracle_f64, nx, ny, multistep):
    p, ob, body, u_in, states, av, fx, fy = single_steps(lbm, nx, ny, multistep)
    om = _trt_ref.omega_minus(p.omega, MAGIC) if trt_of(nx, ny, multistep) else None
    assert av.shape == (SINGLE_STEPS,)
    for t in range(SINGLE_STEPS):
        want, u = _open_ref.step(states[t], ob, p.omega, om, u_in, RHO_OUT)
        differs = int(np.count_nonzero(want != states[t + 1]))
        total = float(np.sum(u))
        err, tol = abs(av[t] - total * p.free_cells_inv), nx * ny * U * total
        rx, ry, links, mag = _open_ref.force(states[t], ob, body)
        ftol = 8.0 * links * U * mag
        print("%dx%d multistep %d %s step %d: %d values differ; av_vels %.17e |d| %.2e tol %.2e; F (%.6e, %.6e) |d| %.2e %.2e tol %.2e" %
              (nx, ny, multistep, "TRT" if om else "BGK", t, differs, av[t], err, tol, fx[t], fy[t], abs(fx[t] - rx),
               abs(fy[t] - ry), ftol))
        assert np.array_equal(states[t + 1], want), (t, differs)
        assert total > 0.0 and err <= tol, (t, av[t], total * p.free_cells_inv, tol)
        assert abs(fx[t] - rx) <= ftol and abs(fy[t] - ry) <= ftol, (t, fx[t], rx, fy[t], ry, ftol)
        if links:
            assert mag > 0.0 and max(abs(fx[t]), abs(fy[t])) > 1e-5
        else:
            assert (nx, ny) == (5, 4) and fx[t] == 0.0 and fy[t] == 0.0
        # another flow: not the periodic, accelerated step of the same state
        periodic, _ = _trt_ref.step(accelerated(oracle_f64, p, ob, states[t]), ob, p.omega, om)
        assert not np.array_equal(states[t + 1], periodic)
        assert not np.array_equal(states[t + 1][:, :, 0], periodic[:, :, 0])
        assert not np.array_equal(states[t + 1][:, :, nx - 1], periodic[:, :, nx - 1])


def test_the_column_rule_keeps_links_across_the_wrap_out_of_the_force(lbm):
    """33x19: the blocked cell (5, 0) has fluid neighbours on both sides of the wrap.  With open boundaries it is outside every
    body; the caller's body map is returned unchanged"""
    p, ob, body, cells0, u_in = open_case(lbm, 33, 19, 4)
    with lbm.LBMDouble(p, ob) as sim:
        whole = sim.body()
        assert whole[5, 0] == 1
        sim.upload(cells0)
        periodic = sim.force()
        sim.set_open(u_in, RHO_OUT)
        assert np.array_equal(sim.body(), whole)
        got = sim.force()
        rx, ry, links, mag = _open_ref.force(cells0, ob, None)
        tol = 8.0 * links * U * mag
        assert abs(got[0] - rx) <= tol and abs(got[1] - ry) <= tol
        assert got[0] != periodic[0] and got[1] != periodic[1]       # the cell's links, and accelerate_flow, are gone
        only = np.zeros_like(ob)
        only[5, 0] = 1
        sim.set_body(only)
        assert np.array_equal(sim.body(), only)
        assert sim.force() == (0.0, 0.0)
        sim.set_open(None)
        assert sim.force() != (0.0, 0.0)


# ---- 2. forms, launch splits, runs -------------------------------------------------------------------------------------

def run_of(lbm, p, ob, body, cells0, u_in, multistep, runs, on=True):
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_option("multistep", multistep)
        sim.set_option("force", 1)
        sim.set_body(body)
        sim.set_trt(MAGIC)
        if on:
            sim.set_open(u_in, RHO_OUT)
        sim.upload(cells0)
        for r in runs:
            sim.run(r)
        return sim.download() + sim.force_record()


@pytest.mark.parametrize("nx,ny", [(33, 19), (48, 35)])
def test_bit_identical_between_forms_splits_and_runs(lbm, nx, ny):
    steps = sum(SPLITS)
    assert steps == 400
    p, ob, body, cells0, u_in = open_case(lbm, nx, ny, steps)
    ref = run_of(lbm, p, ob, body, cells0, u_in, 0, [steps])
    assert ref[1].shape == (steps,) and all(np.all(np.isfinite(v)) for v in ref) and np.all(ref[0] > 0.0)
    for multistep in (0, 3, 8):
        for runs in ([steps], SPLITS):
            if (multistep, len(runs)) == (0, 1):
                continue
            got = run_of(lbm, p, ob, body, cells0, u_in, multistep, runs)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)), (multistep, len(runs))
    again = run_of(lbm, p, ob, body, cells0, u_in, 8, [150, 250])                    # two runs against one
    assert all(np.array_equal(a, b) for a, b in zip(again, ref))
    periodic = run_of(lbm, p, ob, body, cells0, u_in, 8, SPLITS, on=False)
    assert not np.array_equal(periodic[0], ref[0]) and not np.array_equal(periodic[1], ref[1])


# ---- 3. ensemble members -----------------------------------------------------------------------------------------------

ENS_OMEGAS = [float(v) for v in np.linspace(1.0, 1.85, 5)]
ENS_MAGICS = [3.0 / 16.0, 1.0 / 4.0, 1.0 / 12.0, 1.0 / 6.0, 3.0 / 16.0]
ENS_RHO = [0.1, 0.102, 0.098, 0.101, 0.1005]
ENS_RUNS = RUNS[:10] + [20]      # 1, 1, 9, 2..8, 20: launches of every depth, two-launch splits and a tail, 66 steps


def snapshot(sim):
    cells, av = sim.download()
    return [cells, av] + list(sim.final_state()) + [sim.reynolds()] + list(sim.force_record()) + list(sim.force())


@pytest.mark.parametrize("nx,ny,trt", [(33, 19, True), (48, 35, False)])
def test_members_equal_dp_contexts_bit_for_bit(lbm, nx, ny, trt):
    n, steps = len(ENS_OMEGAS), sum(ENS_RUNS)
    ob, body = open_mask(nx, ny)
    base = lbm.make_dparams(nx, ny, steps, density=0.1, accel=0.005, omega=1.7, obstacles=ob)
    params = lbm.sweep_dparams(base, omega=ENS_OMEGAS)
    rng = np.random.default_rng(100 * nx + ny)
    cells0 = np.stack([random_state(rng, 0.1, ny, nx) for _ in range(n)])
    u_in = np.stack([profile(nx, ny, seed=k, scale=0.6 + 0.2 * k) for k in range(n)])
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.set_option("force", 1)
        ens.set_body(body)
        if trt:
            ens.set_trt(ENS_MAGICS)
        assert ens.open() is None
        ens.set_open(u_in, ENS_RHO)
        back = ens.open()
        assert np.array_equal(back[0], u_in) and back[1].tolist() == ENS_RHO
        ens.upload(cells0)
        for r in ENS_RUNS:
            ens.run(r)
        got = snapshot(ens)
    assert np.all(np.isfinite(got[0])) and got[1].shape == (n, steps) and np.any(got[7] != 0.0)
    for k in range(n):
        with lbm.LBMDouble(params[k], ob) as sim:
            sim.set_option("force", 1)
            sim.set_body(body)
            if trt:
                sim.set_trt(ENS_MAGICS[k])
            sim.set_open(u_in[k], ENS_RHO[k])
            sim.upload(cells0[k])
            sim.run(steps)
            ref = snapshot(sim)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert np.array_equal(a[k], b), (k, i)
    assert len({got[0][k].tobytes() for k in range(n)}) == n


# ---- 4. steady runs ----------------------------------------------------------------------------------------------------

def steady_profiles(ny):
    return np.stack([_open_ref.poiseuille(ny, 0.02 * (1.0 + 0.5 * m)) for m in range(4)])


def steady_ensemble(lbm, nx, ny):
    params, ob = sweep(lbm, nx, ny, OMEGAS[4], max_iters=CAP)
    ens = lbm.EnsembleDouble(params, ob)
    ens.set_option("force", 1)
    ens.set_body(block_body(nx, ny))
    ens.set_trt(MAGIC)
    ens.set_open(steady_profiles(ny), 0.1)
    ens.upload(None)
    return ens, params, ob


@pytest.mark.parametrize("on", ["av_vels", "drag"])
def test_run_until_stops_every_member_where_the_rule_says(lbm, on):
    nx, ny, window = 48, 32, 7
    ens, params, ob = steady_ensemble(lbm, nx, ny)
    with ens:
        ens.run(CAP)
        whole = {"av": ens.download(cells=False)[1], "fx": ens.force_record()[0]}
        assert whole["av"].shape == (4, CAP) and np.all(np.isfinite(whole["av"])) and np.all(np.isfinite(whole["fx"]))
        # the stop decisions, on the host from the downloaded record
        want_steps, want_conv = rule(whole["av" if on == "av_vels" else "fx"], 0, CAP, window, TOL)
        print("open %dx%d window %d on %s: stops %s converged %s" % (nx, ny, window, on, want_steps.tolist(), want_conv.tolist()))
        assert np.any(want_conv) and len(set(want_steps.tolist())) >= 2
        ens.upload(None)
        assert ens.open() is not None                                  # the upload keeps the setting
        steps, conv = ens.run_until(CAP, window=window, rel_tol=TOL, on=on)
        assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
        cells, av = ens.download()
        fx, fy = ens.force_record()
        fields, re, now = ens.final_state(), ens.reynolds(), ens.force()
    profiles = steady_profiles(ny)
    for m in range(4):
        c = int(steps[m])
        with lbm.LBMDouble(params[m], ob) as sim:
            sim.set_option("force", 1)
            sim.set_body(block_body(nx, ny))
            sim.set_trt(MAGIC)
            sim.set_open(profiles[m], 0.1)
            sim.upload(None)
            sim.run(c)
            rc, rav = sim.download()
            rfx, rfy = sim.force_record()
            assert np.array_equal(cells[m], rc), m
            assert np.array_equal(av[m, :c], rav) and np.array_equal(av[m, :c], whole["av"][m, :c]), m
            assert np.array_equal(fx[m, :c], rfx) and np.array_equal(fy[m, :c], rfy), m
            assert all(np.array_equal(a[m], b) for a, b in zip(fields, sim.final_state())), m
            assert re[m] == sim.reynolds() and (now[0][m], now[1][m]) == sim.force(), m


# ---- 5. the channel check ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("omega", [1.0, 1.7])
def test_channel_check_at_multistep_8(lbm, omega):
    nx, ny, u_max, steps = 32, 11, 0.01, 8000
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    p = lbm.make_dparams(nx, ny, steps, density=0.1, accel=0.005, omega=omega, obstacles=ob)
    figures = {}
    for trt in (True, False):
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("multistep", 8)
            if trt:
                sim.set_trt(MAGIC)
            sim.set_open(_open_ref.poiseuille(ny, u_max), 0.1)
            sim.upload(None)
            sim.run(steps)
            figures[trt] = _open_ref.channel_figures(sim.download(av_vels=False)[0], u_max)
    print("32x11 omega %.1f after %d steps at multistep 8: flux spread TRT %.2e BGK %.2e; shape error TRT %.2e BGK %.2e" %
          (omega, steps, figures[True][0], figures[False][0], figures[True][1], figures[False][1]))
    assert 0.0 <= figures[True][0] < 1e-7 and 0.0 <= figures[False][0] < 1e-7
    assert figures[True][1] < 1e-4
    assert figures[False][1] > 1e-3


# ---- 6. set, unset, errors ---------------------------------------------------------------------------------------------

def plain_run(lbm, p, ob, cells0, multistep, touch=None):
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_option("multistep", multistep)
        sim.set_option("force", 1)
        if touch:
            touch(sim)
        sim.upload(cells0)
        for r in (1, 9, 30):
            sim.run(r)
        return list(sim.download()) + list(sim.force_record()) + list(sim.final_state()) + [sim.reynolds()]


@pytest.mark.parametrize("multistep", [0, 8])
def test_off_and_set_then_unset_leave_the_periodic_bits(lbm, multistep):
    p, ob, body, cells0, u_in = open_case(lbm, 33, 19, 40)
    never = plain_run(lbm, p, ob, cells0, multistep)

    def off(sim):
        assert sim.open() is None
        sim.set_open(None)
        assert sim.open() is None

    def on_off(sim):
        sim.set_open(u_in, RHO_OUT)
        got = sim.open()
        assert np.array_equal(got[0], u_in) and got[1] == RHO_OUT
        sim.set_open(None)
        assert sim.open() is None

    for touch in (off, on_off):
        assert all(np.array_equal(a, b) for a, b in zip(plain_run(lbm, p, ob, cells0, multistep, touch), never)), touch.__name__
    params = lbm.sweep_dparams(p, omega=[1.2, 1.7])
    snaps = []
    for touch in (False, True):
        with lbm.EnsembleDouble(params, ob) as ens:
            ens.set_option("force", 1)
            if touch:
                ens.set_open(u_in, RHO_OUT)
                assert ens.open()[1].tolist() == [RHO_OUT, RHO_OUT]
                ens.set_open(None)
            assert ens.open() is None
            ens.upload(np.stack([cells0, cells0]))
            ens.run(40)
            snaps.append(ens.download() + ens.force_record())
    assert all(np.array_equal(a, b) for a, b in zip(*snaps))


def test_a_second_setting_after_off_replaces_the_first(lbm):
    """Set, unset, set again with another profile and outlet density, then one step against the restatement on the second
    setting: the device copy of the profile is rewritten in place and nothing of the first setting stays.  17x16: nx odd, one
    whole tile and a ragged one; the form with one step a launch and the LDS-tile form."""
    nx, ny = 17, 16
    p, ob, body, cells0, u_in = open_case(lbm, nx, ny, 2)
    other, rho = profile(nx, ny, seed=1, scale=0.5), 0.0985
    want, _ = _open_ref.step(cells0, ob, p.omega, None, other, rho)
    first, _ = _open_ref.step(cells0, ob, p.omega, None, u_in, RHO_OUT)
    assert not np.array_equal(want, first)
    for multistep in (0, 8):
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("multistep", multistep)
            sim.set_open(u_in, RHO_OUT)
            sim.set_open(None)
            sim.set_open(other, rho)
            got = sim.open()
            assert np.array_equal(got[0], other) and got[1] == rho
            sim.upload(cells0)
            sim.run(1)
            assert np.array_equal(sim.download(av_vels=False)[0], want), multistep


def test_errors_and_what_keeps_the_setting(lbm):
    lib = lbm.load_library()
    p, ob, body, cells0, u_in = open_case(lbm, 33, 19, 8)
    ny = 19
    on = ctypes.c_int()

    def ptr(a):
        return a.ctypes.data

    with lbm.LBMDouble(p, ob) as sim:
        sim.upload(cells0)
        sim.run(1)
        periodic = sim.download(av_vels=False)[0]
        assert lib.lbm_dopen_set(sim.ctx, ptr(u_in), RHO_OUT) == LBM_ERR_STATE         # after a step
        assert sim.open() is None
        sim.upload(cells0)                                                            # accepted again
        sim.set_open(u_in, RHO_OUT)
        for row, bad in ((3, float("nan")), (0, float("inf")), (18, 1.0), (7, 1.5), (5, -float("inf"))):
            u = u_in.copy()
            u[row] = bad                                                              # row 5: column 0 is blocked there
            assert lib.lbm_dopen_set(sim.ctx, ptr(u), RHO_OUT) == LBM_ERR_ARG
            assert ("row %d" % row).encode() in lib.lbm_last_error(), lib.lbm_last_error()
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            assert lib.lbm_dopen_set(sim.ctx, ptr(u_in), bad) == LBM_ERR_ARG
            assert b"rho_out" in lib.lbm_last_error()
        assert lib.lbm_dopen_get(sim.ctx, None, None, None) == LBM_ERR_ARG
        assert lib.lbm_dopen_get(sim.ctx, ctypes.byref(on), None, None) == 0 and on.value == 1
        got = sim.open()
        assert np.array_equal(got[0], u_in) and got[1] == RHO_OUT                     # nothing changed on the host
        sim.run(1)
        opened = sim.download(av_vels=False)[0]
        want, _ = _open_ref.step(cells0, ob, p.omega, None, u_in, RHO_OUT)
        assert np.array_equal(opened, want) and not np.array_equal(opened, periodic)  # ... nor on the device
        assert lib.lbm_dopen_set(sim.ctx, None, 0.0) == LBM_ERR_STATE
        sim.upload(cells0)                                                            # uploads keep the setting
        sim.upload_obstacles(ob)
        assert sim.open() is not None
        only = np.zeros_like(ob)
        only[5, 0] = 1
        sim.set_body(only)                                                            # the obstacle upload wrote the column rule
        assert sim.force() == (0.0, 0.0)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], opened)

    params = lbm.sweep_dparams(p, omega=[1.2, 1.7, 1.0])
    profiles = np.stack([u_in, 0.5 * u_in, 1.5 * u_in])
    rhos = np.array([0.1, 0.102, 0.099])
    with lbm.EnsembleDouble(params, ob) as ens:
        ens.set_open(profiles, rhos)
        for member, row, bad in ((1, 4, float("nan")), (2, 0, 1.0), (0, 18, float("inf"))):
            u = profiles.copy()
            u[member, row] = bad
            assert lib.lbm_dopen_ens_set(ens.ens, ptr(u), ptr(rhos)) == LBM_ERR_ARG
            msg = lib.lbm_last_error()
            assert ("member %d" % member).encode() in msg and ("row %d" % row).encode() in msg, msg
        quarter = 0.25 * profiles
        for member, bad in ((1, 0.0), (2, float("nan")), (0, -1.0)):
            r = rhos.copy()
            r[member] = bad
            assert lib.lbm_dopen_ens_set(ens.ens, ptr(quarter), ptr(r)) == LBM_ERR_ARG
            msg = lib.lbm_last_error()
            assert ("member %d" % member).encode() in msg and b"rho_out" in msg, msg
        assert lib.lbm_dopen_ens_set(ens.ens, ptr(profiles), None) == LBM_ERR_ARG
        assert lib.lbm_dopen_ens_get(ens.ens, None, None, None) == LBM_ERR_ARG
        back = ens.open()
        assert np.array_equal(back[0], profiles) and np.array_equal(back[1], rhos)
        ens.upload(np.stack([cells0] * 3))
        ens.run(2)
        cells = ens.download(av_vels=False)[0]
        assert lib.lbm_dopen_ens_set(ens.ens, None, None) == LBM_ERR_STATE
        assert lib.lbm_dopen_ens_set(ens.ens, ptr(profiles), ptr(rhos)) == LBM_ERR_STATE
        ens.upload(np.stack([cells0] * 3))                                            # keeps the setting
        assert ens.open() is not None
        ens.run(2)
        assert np.array_equal(ens.download(av_vels=False)[0], cells)
    # nothing on the device changed after the refusals: the members ran as contexts with the accepted setting
    for k in range(3):
        with lbm.LBMDouble(params[k], ob) as sim:
            sim.set_open(profiles[k], rhos[k])
            sim.upload(cells0)
            sim.run(2)
            assert np.array_equal(sim.download(av_vels=False)[0], cells[k]), k
        assert ny == profiles.shape[1]

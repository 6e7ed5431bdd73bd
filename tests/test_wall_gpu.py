"""Moving walls (include/lbm.h, "Moving walls"; lbm_dwall_*) on the GPU: every WALL instance of the four double-precision
kernel families against tests/_wall_ref.py, bit for bit.

WALL is a fourth template flag beside FORCE, TRT and OPEN of d2q9_dp_step, d2q9_dp_multi (LBMDouble at "multistep" 0 and 8),
d2q9_dp_ensemble (EnsembleDouble.run) and d2q9_dp_ensemble_gated (EnsembleDouble.run_until): 32 more separately compiled
kernels.  The cases, the drivers and the gates are those of tests/_dp_matrix.py and tests/test_dp_matrix_gpu.py, imported and
not edited; `walled` hands the drivers an LBMDouble / EnsembleDouble that has had set_wall called on it.

  1. the matrix: the 8 FORCE x TRT x OPEN combinations x the 4 families x 33x19 and 17x16, three members, runs of 1, 1, 1 and 7
     steps.  Per member a velocity with |component| <= 0.05 on every blocked cell, but one wall row and part of the body, which
     stay at exactly 0.0: both branches of the obstacle run beside each other.  rho_wall differs per member.  Compared: cells
     after each run, av_vels, the force record and force() before each run; ensemble members also against the contexts;
  2. a region wider than the grid: 6x5, rows 0 and 4 moving with a velocity per column and member, in d2q9_dp_multi and both
     ensemble kernels, six single steps.  A copy of a wall cell that takes another cell's velocity fails here;
  3. off is off: set_wall and then off, and a map of +-0.0, equal a handle that never heard of walls in cells, av_vels, the force
     record and force(), on both shapes in all families;
  4. identities: "multistep" 0 against 8 and context against member (in 1), one run of 10 against 3 + 7, a member stopped by
     run_until against a plain run to its count (37x29, four members, a moving lid);
  5. end to end: Couette flow, 16x16, 6000 steps through LBMDouble with "multistep" 8 and "force", to the profile bound and the
     two wall forces of tests/test_wall_restatement_cpu.py, the downloaded state equal to _wall_ref run alongside on the CPU."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import _dp_matrix as dm
import _wall_ref
from test_dp_matrix_gpu import assert_equals_the_reference, assert_same_bits
from test_dp_steady_gpu import TOL, channel, rule
from test_wall_restatement_cpu import couette_run

pytestmark = pytest.mark.gpu

SHAPES = [(33, 19), (17, 16)]
RUNS = [1, 1, 1, 7]
FLAGS = list(itertools.product((0, 1), repeat=3))
RHO_WALLS = [0.0985, 0.1, 0.103]
_refs, _runs = {}, {}


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def walled(lbm, case):
    """`lbm` as the drivers of _dp_matrix use it: LBMDouble and EnsembleDouble that call set_wall with the members' `wall`
    (None: never called; "off": set, then turned off) before anything else happens to the handle"""
    def set_on(handle, members):
        mode = members[0].wall
        if mode is None:
            return handle
        on = [m.wall_on if mode == "off" else m.wall for m in members]
        if len(on) == 1:
            handle.set_wall(*on[0])
        else:
            handle.set_wall(np.stack([w[0] for w in on]), np.stack([w[1] for w in on]), [w[2] for w in on])
        assert handle.wall() is not None
        if mode == "off":
            handle.set_wall(None, None)
            assert handle.wall() is None
        return handle

    def context(p, ob):
        return set_on(lbm.LBMDouble(p, ob), [next(m for m in case.members if m.p is p)])

    def ensemble(params, obs):
        assert all(p is m.p for p, m in zip(params, case.members))
        return set_on(lbm.EnsembleDouble(params, obs), case.members)

    return SimpleNamespace(LBMDouble=context, EnsembleDouble=ensemble)


def member_wall(m, k, nx, ny):
    """member k's velocities: |component| <= 0.05 on every blocked cell, exactly 0.0 on wall row 0, on the first row of the
    body's block and on one lip cell"""
    rng = np.random.default_rng(4000 + 100 * nx + 10 * ny + k)
    blocked = m.ob != 0
    u_x = np.where(blocked, 0.1 * (rng.random((ny, nx)) - 0.5), 0.0)
    u_y = np.where(blocked, 0.1 * (rng.random((ny, nx)) - 0.5), 0.0)
    r = dm.matrix_rows(nx, ny, k)
    for u in (u_x, u_y):
        u[0] = 0.0
        u[ny // 2 - 2] = 0.0
        u[r.lip_west, 1] = 0.0
    return u_x, u_y, RHO_WALLS[k]


def with_walls(case, mode="on"):
    """the case with a `wall` per member: mode "on" = member_wall, None = never set, "off" = set and turned off, "zeros" = a
    map of +0.0 and -0.0"""
    for k, m in enumerate(case.members):
        m.wall_on = member_wall(m, k, case.nx, case.ny)
        if mode == "on":
            m.wall = m.wall_on
        elif mode == "zeros":
            signed = np.where((np.arange(case.nx)[None, :] + np.arange(case.ny)[:, None]) % 2 == 0, 0.0, -0.0)
            m.wall = (signed, -signed, RHO_WALLS[k])
        else:
            m.wall = mode
    return case


def reference_run(oracle_f64, m, steps):
    """_dp_matrix.reference_run through _wall_ref.reference_step"""
    wall = m.wall if isinstance(m.wall, tuple) else None
    states, totals, forces = [m.cells0], [], []
    for _ in range(steps):
        cells, u, force = _wall_ref.reference_step(oracle_f64, m.p, m.ob, m.body, states[-1], m.magic, m.open, wall)
        states.append(cells)
        totals.append(float(np.sum(u)))
        forces.append(force)
    return SimpleNamespace(states=states, totals=totals, forces=forces)


def reference_of(oracle_f64, key, case, steps):
    if key not in _refs:
        _refs[key] = [reference_run(oracle_f64, m, steps) for m in case.members]
    return _refs[key]


def run_of(lbm, key, family, case, runs):
    if (family,) + key not in _runs:
        _runs[(family,) + key] = dm.drive(walled(lbm, case), family, case, runs)
    return _runs[(family,) + key]


# ---- 1. the instance matrix --------------------------------------------------------------------------------------------

def matrix_case(lbm, nx, ny, force, trt, opened, mode="on"):
    return with_walls(dm.make_case(lbm, nx, ny, 3, sum(RUNS), force, trt, opened), mode)


def test_the_velocities_hold_what_they_promise(lbm):
    for nx, ny in SHAPES:
        case = matrix_case(lbm, nx, ny, 1, 0, 0)
        for m in case.members:
            u_x, u_y, rho = m.wall
            blocked = m.ob != 0
            mv = _wall_ref.moving(m.ob, u_x, u_y)
            assert np.all(u_x[~blocked] == 0.0) and np.all(u_y[~blocked] == 0.0)
            assert max(np.abs(u_x).max(), np.abs(u_y).max()) <= 0.05
            assert not mv[0].any() and mv[ny - 1].all()                           # one wall row rests, the other moves
            body = m.body != 0
            assert np.count_nonzero(body & mv) >= 8 and np.count_nonzero(body & ~mv) >= 4
            assert np.count_nonzero(blocked & ~body & mv) >= nx                   # moving cells outside the body too
        assert len({m.wall[2] for m in case.members}) == 3 and len({m.wall[0].tobytes() for m in case.members}) == 3


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", dm.FAMILIES)
@pytest.mark.parametrize("force,trt,opened", FLAGS)
def test_every_wall_instance_equals_the_reference(lbm, oracle_f64, force, trt, opened, family, nx, ny):
    what = "%s<%d,%d,%d,1> %dx%d" % (family, force, trt, opened, nx, ny)
    case = matrix_case(lbm, nx, ny, force, trt, opened)
    refs = reference_of(oracle_f64, ("matrix", nx, ny, trt, opened), case, sum(RUNS))
    got = run_of(lbm, ("matrix", nx, ny, force, trt, opened), family, case, RUNS)
    assert_equals_the_reference(case, refs, got, RUNS, what)
    assert len({r.states[-1].tobytes() for r in got}) == case.n                   # the members are different flows
    # the walls change the flow: the reference without them differs from the first step on
    still = reference_of(oracle_f64, ("still", nx, ny, trt, opened), matrix_case(lbm, nx, ny, force, trt, opened, None), 1)
    assert all(not np.array_equal(a.states[1], b.states[1]) for a, b in zip(refs, still))
    if not force:
        # the option computes the same flow, and force() needs no option
        on = run_of(lbm, ("matrix", nx, ny, 1, trt, opened), family, matrix_case(lbm, nx, ny, 1, trt, opened), RUNS)
        assert_same_bits(got, on, what)
    if family in ("ensemble", "gated"):
        # a member is the LBMDouble with its velocities and rho_wall, at "multistep" 0 and 8, bit for bit
        for other in ("dp_step", "dp_multi"):
            assert_same_bits(got, run_of(lbm, ("matrix", nx, ny, force, trt, opened), other, case, RUNS), what)


# ---- 2. a region wider than the grid -------------------------------------------------------------------------------------

def narrow_case(lbm):
    """6x5, rows 0 and 4 blocked and moving, another velocity per column and member; nothing else blocked, every blocked
    cell counts"""
    nx, ny, n, steps = 6, 5, 3, 6
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    members = []
    for k in range(n):
        rng = np.random.default_rng(600 + k)
        p = lbm.make_dparams(nx, ny, steps, density=0.1, accel=0.005, omega=dm.OMEGAS[k], obstacles=ob)
        u_x, u_y = np.zeros((ny, nx)), np.zeros((ny, nx))
        for row in (0, ny - 1):
            u_x[row] = 0.01 * (1 + np.arange(nx)) * (1.0 + 0.25 * k) * (1 if row else -1)
            u_y[row] = 0.004 * (nx - np.arange(nx)) * (1 if row else -1) * (-1) ** k
        members.append(SimpleNamespace(p=p, ob=ob, body=None, cells0=dm.member_state(nx, ny, k), magic=None, open=None,
                                       wall=(u_x, u_y, RHO_WALLS[k])))
    return SimpleNamespace(nx=nx, ny=ny, n=n, steps=steps, force=True, trt=False, opened=False, members=members)


@pytest.mark.parametrize("family", ["dp_multi", "ensemble", "gated"])
def test_region_wider_than_the_grid(lbm, oracle_f64, family):
    runs = [1] * 6
    case = narrow_case(lbm)
    for m in case.members:
        u_x, u_y, _ = m.wall
        assert len(set(u_x[0])) == case.nx and len(set(u_x[-1])) == case.nx and len(set(u_y[0])) == case.nx
        assert max(np.abs(u_x).max(), np.abs(u_y).max()) <= 0.1
    refs = reference_of(oracle_f64, ("narrow",), case, len(runs))
    got = run_of(lbm, ("narrow",), family, case, runs)
    assert_equals_the_reference(case, refs, got, runs, "%s 6x5" % family)
    assert len({r.states[-1].tobytes() for r in got}) == case.n


# ---- 3. off is off -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", dm.FAMILIES)
@pytest.mark.parametrize("force,trt,opened", [(1, 0, 0), (1, 1, 1)])
def test_off_is_off(lbm, force, trt, opened, family, nx, ny):
    what = "%s<%d,%d,%d> %dx%d" % (family, force, trt, opened, nx, ny)
    never = run_of(lbm, ("never", nx, ny, force, trt, opened), family, matrix_case(lbm, nx, ny, force, trt, opened, None), RUNS)
    for mode in ("off", "zeros"):
        case = matrix_case(lbm, nx, ny, force, trt, opened, mode)
        got = run_of(lbm, (mode, nx, ny, force, trt, opened), family, case, RUNS)
        assert_same_bits(got, never, what + " " + mode)
    # and that flow is not the one with the walls moving
    on = run_of(lbm, ("matrix", nx, ny, force, trt, opened), family, matrix_case(lbm, nx, ny, force, trt, opened), RUNS)
    assert all(not np.array_equal(a.states[0], b.states[0]) for a, b in zip(on, never))


# ---- 4. identities -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", dm.FAMILIES)
def test_one_run_of_ten_against_three_and_seven(lbm, family):
    nx, ny = SHAPES[0]
    whole = run_of(lbm, ("ten", 10), family, matrix_case(lbm, nx, ny, 1, 1, 0), [10])
    split = run_of(lbm, ("ten", 3, 7), family, matrix_case(lbm, nx, ny, 1, 1, 0), [3, 7])
    for k, (a, b) in enumerate(zip(whole, split)):
        assert np.array_equal(a.states[-1], b.states[-1]), (family, k)
        assert np.array_equal(a.av, b.av) and np.array_equal(a.fx, b.fx) and np.array_equal(a.fy, b.fy), (family, k)
        assert b.now[1] == (b.fx[3], b.fy[3])


def test_a_member_stopped_by_run_until_is_a_plain_run_to_its_count(lbm):
    nx, ny, window, cap = 37, 29, 7, 200
    omegas = (0.6, 1.0, 1.4, 1.7)
    ob = channel(nx, ny)
    base = lbm.make_dparams(nx, ny, cap, density=0.1, accel=0.005, omega=omegas[0], obstacles=ob)
    params = lbm.sweep_dparams(base, omega=list(omegas))
    u_x, u_y = np.zeros((ny, nx)), np.zeros((ny, nx))
    u_x[ny - 1] = 0.04                                                            # the lid
    rhos = np.array([0.1, 0.0985, 0.102, 0.1])

    def ensemble():
        ens = lbm.EnsembleDouble(params, ob)
        ens.set_option("force", 1)
        ens.set_wall(u_x, u_y, rhos)
        ens.upload(None)
        return ens

    with ensemble() as ens:
        ens.run(cap)
        whole = ens.download(cells=False)[1]
    want_steps, want_conv = rule(whole, 0, cap, window, TOL)
    print("moving lid %dx%d window %d: stops %s converged %s" % (nx, ny, window, want_steps.tolist(), want_conv.tolist()))
    assert np.any(want_conv) and len(set(want_steps.tolist())) >= 2
    with ensemble() as ens:
        steps, conv = ens.run_until(cap, window=window, rel_tol=TOL)
        assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
        cells, av = ens.download()
        fx, fy = ens.force_record()
        now = ens.force()
    for k, p in enumerate(params):
        c = int(steps[k])
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("force", 1)
            sim.set_wall(u_x, u_y, rhos[k])
            sim.upload(None)
            sim.run(c)
            rc, rav = sim.download()
            rfx, rfy = sim.force_record()
            assert np.array_equal(cells[k], rc), k
            assert np.array_equal(av[k, :c], rav) and np.array_equal(av[k, :c], whole[k, :c]), k
            assert np.array_equal(fx[k, :c], rfx) and np.array_equal(fy[k, :c], rfy), k
            assert (now[0][k], now[1][k]) == sim.force(), k
        # the lid drives it: without the setting the member is another flow
    with lbm.LBMDouble(params[0], ob) as sim:
        sim.upload(None)
        sim.run(int(steps[0]))
        assert not np.array_equal(sim.download(av_vels=False)[0], cells[0])


# ---- 5. end to end: Couette flow -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("trt", [False, True])
def test_couette_flow_end_to_end(lbm, trt):
    c = _wall_ref.COUETTE
    nx, ny, steps = c["nx"], c["ny"], c["steps"]
    ob, u_x, u_y = _wall_ref.couette_maps()
    p = lbm.make_dparams(nx, ny, steps, density=c["rho"], accel=0.0, omega=c["omega"], obstacles=ob)
    top, bottom = np.zeros_like(ob), np.zeros_like(ob)
    top[ny - 1], bottom[0] = 1, 1

    def context(force):
        sim = lbm.LBMDouble(p, ob)
        sim.set_option("multistep", 8)
        sim.set_option("force", force)
        if trt:
            sim.set_trt(c["magic"])
        sim.set_wall(u_x, u_y, c["rho"])
        sim.upload(None)
        return sim

    with context(1) as sim:
        sim.set_body(top)
        sim.run(steps)
        cells = sim.download(av_vels=False)[0]
        f_top = sim.force()
        record = sim.force_record()
    with context(0) as sim:                                                       # a body map may change between runs here
        sim.run(steps)
        assert np.array_equal(sim.download(av_vels=False)[0], cells)
        sim.set_body(top)
        assert sim.force() == f_top
        sim.set_body(bottom)
        f_bottom = sim.force()
    _, want, _ = couette_run(trt)
    assert np.array_equal(cells, want)                                            # _wall_ref alongside, bit for bit
    err = float(np.max(np.abs(_wall_ref.column_velocity(cells, nx // 2) - _wall_ref.couette_profile(ny, c["U"])))) / c["U"]
    shear = _wall_ref.couette_force(nx, ny, c["U"], c["rho"], c["omega"])
    rel_top, rel_bottom = abs(f_top[0] + shear) / shear, abs(f_bottom[0] - shear) / shear
    print("Couette %s on the GPU: profile within %.2e U, F_x top %+.13e (%.1e relative) bottom %+.13e (%.1e relative)" %
          ("TRT" if trt else "BGK", err, f_top[0], rel_top, f_bottom[0], rel_bottom))
    assert err <= 1e-10
    assert rel_top <= 1e-9 and rel_bottom <= 1e-9
    assert abs(record[0][-1] + shear) <= 1e-9 * shear                             # the record's last entry is the settled force too

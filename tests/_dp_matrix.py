"""The instance matrix of the double-precision kernel families: one case that carries the settings of every option (FORCE, TRT,
OPEN, moving walls, the subgrid viscosity, the body force, the scalar), the routed reference, one driver per family, the gates,
and one body for each test that every option's GPU module repeats.  Shared by tests/test_dp_matrix_cpu.py (the conditions on the
inputs), tests/test_dp_matrix_gpu.py, tests/test_wall_gpu.py, tests/test_les_gpu.py, tests/test_drive_gpu.py and
tests/test_scalar_gpu.py.

Nothing is restated here.  reference_step routes a state to what the suite already trusts: _drive_ref.step, which falls through
_les_ref.step, _wall_ref.step and _open_ref.step to _trt_ref.step as each option is off, and for the force _open_ref.force with
open boundaries on, _force_ref.restatement or _force_ref.body_restatement on _force_ref.accelerated(...) without.  column_links
names the links of _open_ref.force whose fluid end lies in column 0 or nx - 1, by that function's own index arithmetic, for the
CPU module's condition that a force pass which loses them is seen.

The masks put counted cells beside the two open columns.  With open boundaries on, the LDS-tile kernels mark the fluid cells
of those columns in their mask byte, and the force pass has to read a marked neighbour as fluid: a body away from the columns,
as every ensemble test before this one had, never asks that of it.

A member names each option by one field: None = never set, "off" = set to the member's `<option>_on` and then unset, anything
else = the setting (`wall` "zeros" of make_case: a map of +0.0 and -0.0).  open_context and open_ensemble call set_wall, set_les
and set_drive in that order before anything else happens to the handle, and read each setting back."""
import itertools
from types import SimpleNamespace

import numpy as np

import _drive_ref
import _open_ref
import _scalar_ref
import _trt_ref
from _dp_states import random_state
from _force_ref import accelerated, body_restatement, restatement
from _steady_rule import TOL, channel, rule

U = 2.0 ** -53
FAMILIES = ("dp_step", "dp_multi", "ensemble", "gated")
MULTISTEP = {"dp_step": 0, "dp_multi": 8}
SHAPES = [(33, 19), (17, 16)]
RUNS = [1, 1, 1, 7]
# per member; four of each for the steady run
OMEGAS = [1.7, 1.2, 1.0, 1.45]
MAGICS = [3.0 / 16.0, 1.0 / 4.0, 1.0 / 12.0, 1.0 / 6.0]
RHOS = [0.102, 0.1, 0.0985, 0.101]
RHO_WALLS = [0.0985, 0.1, 0.103]                                              # moving walls: rho_wall
CS = [0.1, 0.17, 0.3, 0.17]                                                   # the subgrid viscosity: c
FORCES = [(1e-6, -3e-5), (-1e-4, 2e-6), (4e-5, 1e-5), (-2e-5, -6e-6)]         # the body force: (F_x, F_y)
DS = [0.01, 1.0 / 6.0, 0.4]                                                   # the scalar: D
# a gated run is one leg shorter than this window: it is run and not checked (lbm_dsteady_run), so no member stops
GATED_WINDOW = 16
GATED_TOL = 2e-2


def flags(n):
    """every combination of n template flags"""
    return list(itertools.product((0, 1), repeat=n))


def matrix_rows(nx, ny, member=0):
    """where matrix_mask puts what moves with the member: the first rows of the two three-cell lips and the rows of the two
    column cells"""
    return SimpleNamespace(lip_west=ny // 2 - 3 + member, lip_east=ny // 2 - 2 + member, cell_west=3 + member,
                           cell_east=2 + member)


def matrix_mask(nx, ny, member=0, beside=False):
    """(obstacles, body).  Walls on rows 0 and ny - 1.  The body: the 4x5 block of test_open_gpu.open_mask, a lip of three
    cells in column 1 and one in column nx - 2 (matrix_rows: both shift with the member).  Outside the body: the walls, one
    blocked cell inside column 0 and one inside column nx - 1, whose rows shift with the member too.  beside: one more body
    cell, in column 1 beside the blocked cell of column 0.  5x4: nothing blocked, body None."""
    ob = np.zeros((ny, nx), dtype=np.int32)
    if (nx, ny) == (5, 4):
        return ob, None
    r = matrix_rows(nx, ny, member)
    ob[0] = ob[ny - 1] = 1
    body = np.zeros_like(ob)
    body[ny // 2 - 2:ny // 2 + 2, nx // 4:nx // 4 + 5] = 1
    body[r.lip_west:r.lip_west + 3, 1] = 1
    body[r.lip_east:r.lip_east + 3, nx - 2] = 1
    if beside:
        body[r.cell_west, 1] = 1
    ob |= body
    ob[r.cell_west, 0] = 1
    ob[r.cell_east, nx - 1] = 1
    return ob, body


def inlet_profile(nx, ny, member):
    """the parabola between the walls (5x4: a flat profile) times 1 +- 5 % from row to row, another amplitude per member"""
    rng = np.random.default_rng(1000 * nx + ny + member)
    base = np.full(ny, 0.03) if (nx, ny) == (5, 4) else _open_ref.poiseuille(ny, 0.04)
    return (0.6 + 0.2 * member) * base * (1.0 + 0.1 * (rng.random(ny) - 0.5))


def member_state(nx, ny, member):
    """the state a member starts from: the rest weights x 0.1 x (1 +- 10 %)"""
    return random_state(np.random.default_rng(7000 + 100 * nx + 10 * ny + member), 0.1, ny, nx)


def member_wall(m, k, nx, ny):
    """member k's velocities: |component| <= 0.05 on every blocked cell, exactly 0.0 on wall row 0, on the first row of the
    body's block and on one lip cell"""
    rng = np.random.default_rng(4000 + 100 * nx + 10 * ny + k)
    blocked = m.ob != 0
    u_x = np.where(blocked, 0.1 * (rng.random((ny, nx)) - 0.5), 0.0)
    u_y = np.where(blocked, 0.1 * (rng.random((ny, nx)) - 0.5), 0.0)
    r = matrix_rows(nx, ny, k)
    for u in (u_x, u_y):
        u[0] = 0.0
        u[ny // 2 - 2] = 0.0
        u[r.lip_west, 1] = 0.0
    return u_x, u_y, RHO_WALLS[k]


def member_scalar(m, k, nx, ny):
    """member k's scalar: D, c0 in 0.5 .. 1.5, c_wall NaN on half the cells and 0 .. 2 on the others, c_in per row"""
    rng = np.random.default_rng(9000 + 100 * nx + 10 * ny + k)
    wall = 2.0 * rng.random((ny, nx))
    wall[rng.random((ny, nx)) < 0.5] = np.nan
    scalar = SimpleNamespace(D=DS[k], c0=0.5 + rng.random((ny, nx)), wall=wall, inlet=0.5 + rng.random(ny))
    blocked = m.ob != 0
    assert np.any(np.isnan(wall[blocked])) and np.any(np.isfinite(wall[blocked]))
    return scalar


def set_options(m, k, nx, ny, wall=None, les=None, drive=None, scalar=False):
    """fills member k's option fields.  wall: None = never set, "on" = member_wall, "off" = set and turned off, "zeros" = a map
    of +0.0 and -0.0.  les, drive: None, "on" (CS[k], FORCES[k]) or "off".  scalar: member_scalar, else None."""
    m.wall_on = None if wall is None else member_wall(m, k, nx, ny)
    if wall == "on":
        m.wall = m.wall_on
    elif wall == "zeros":
        signed = np.where((np.arange(nx)[None, :] + np.arange(ny)[:, None]) % 2 == 0, 0.0, -0.0)
        m.wall = (signed, -signed, RHO_WALLS[k])
    else:
        m.wall = wall
    m.les_on, m.les = CS[k], (CS[k] if les == "on" else les)
    m.drive_on, m.drive = FORCES[k], (FORCES[k] if drive == "on" else drive)
    m.scalar = member_scalar(m, k, nx, ny) if scalar else None
    return m


def make_case(lbm, nx, ny, n, steps, force, trt, opened, counted="body", beside=None, omegas=OMEGAS, profiles=None, rhos=RHOS,
              rest=False, wall=None, les=None, drive=None, scalar=False):
    """n members on matrix_mask(nx, ny, member), each with its own omega, magic parameter, inlet profile, rho_out and state.
    counted: "body" = the body of matrix_mask, "all" = every blocked cell (body None).  beside: the member whose map gets
    matrix_mask's cell beside the blocked cell of column 0.  profiles: other inlet profiles than inlet_profile's.  rest: every
    member starts from the library's rest state (cells0 None).  wall, les, drive, scalar: set_options."""
    members = []
    for k in range(n):
        ob, body = matrix_mask(nx, ny, k, beside=(k == beside))
        p = lbm.make_dparams(nx, ny, steps, density=0.1, accel=0.005, omega=omegas[k], obstacles=ob)
        u_in = inlet_profile(nx, ny, k) if profiles is None else profiles[k]
        m = SimpleNamespace(p=p, ob=ob, body=body if counted == "body" else None,
                            cells0=None if rest else member_state(nx, ny, k), magic=MAGICS[k] if trt else None,
                            open=(u_in, rhos[k]) if opened else None)
        members.append(set_options(m, k, nx, ny, wall, les, drive, scalar))
    return SimpleNamespace(nx=nx, ny=ny, n=n, steps=steps, force=bool(force), trt=bool(trt), opened=bool(opened), members=members)


def narrow_case(lbm, les=None, drive=None, scalar=False):
    """6x5, rows 0 and 4 blocked and moving, another velocity per column and member; nothing else blocked, every blocked
    cell counts.  les, drive, scalar: set_options."""
    nx, ny, n, steps = 6, 5, 3, 6
    ob = np.zeros((ny, nx), dtype=np.int32)
    ob[0] = ob[ny - 1] = 1
    members = []
    for k in range(n):
        p = lbm.make_dparams(nx, ny, steps, density=0.1, accel=0.005, omega=OMEGAS[k], obstacles=ob)
        u_x, u_y = np.zeros((ny, nx)), np.zeros((ny, nx))
        for row in (0, ny - 1):
            u_x[row] = 0.01 * (1 + np.arange(nx)) * (1.0 + 0.25 * k) * (1 if row else -1)
            u_y[row] = 0.004 * (nx - np.arange(nx)) * (1 if row else -1) * (-1) ** k
        m = set_options(SimpleNamespace(p=p, ob=ob, body=None, cells0=member_state(nx, ny, k), magic=None, open=None), k, nx, ny,
                        None, les, drive, scalar)
        m.wall = (u_x, u_y, RHO_WALLS[k])
        members.append(m)
    return SimpleNamespace(nx=nx, ny=ny, n=n, steps=steps, force=True, trt=False, opened=False, members=members)


def reference_step(oracle_f64, p, ob, body, f, trt_magic, open_setting, wall=None, c=None, drive=None):
    """One restated step of the stored state f under any combination of options: (cells, |u| with 0 on blocked cells, (F_x, F_y,
    links, sum|link terms|) of that step, or None where nothing is blocked).  trt_magic: None or 0 = BGK.  open_setting: None, or
    (u_in, rho_out).  wall: None, or (u_x, u_y, rho_wall).  c: None, or the Smagorinsky constant.  drive: None, or (F_x, F_y)."""
    if open_setting is not None:
        u_in, rho_out = open_setting
        cells, u = _drive_ref.step(f, ob, p.omega, trt_magic, u_in, rho_out, wall, c, drive)
        force = _open_ref.force(f, ob, body)
    else:
        fa = accelerated(oracle_f64, p, ob, f)
        cells, u = _drive_ref.step(fa, ob, p.omega, trt_magic, wall=wall, c=c, drive=drive)
        force = restatement(fa, ob) if body is None else body_restatement(fa, ob, body)
    return cells, u, (force if np.any(ob) else None)


def reference_run(oracle_f64, m, steps):
    """`steps` chained reference steps of member m from its first state: the state after every step (index 0: before the
    first), sum|u| and the force tuple per step"""
    wall = m.wall if isinstance(m.wall, tuple) else None
    c = m.les if isinstance(m.les, float) else None
    drive = m.drive if isinstance(m.drive, tuple) else None
    states, totals, forces = [m.cells0], [], []
    for _ in range(steps):
        cells, u, force = reference_step(oracle_f64, m.p, m.ob, m.body, states[-1], m.magic, m.open, wall, c, drive)
        states.append(cells)
        totals.append(float(np.sum(u)))
        forces.append(force)
    return SimpleNamespace(states=states, totals=totals, forces=forces)


def column_links(f, ob, body=None):
    """The links _open_ref.force counts whose fluid end lies in column 0 and in column nx - 1: (links west, links east, their
    share of F_x, their share of F_y).  _open_ref.force's masks and shifts; a force pass that reads a marked fluid cell of
    those columns as blocked loses exactly these."""
    ny, nx = ob.shape
    blocked = ob != 0
    outer = _open_ref.counted_cells(ob, body)
    column = np.arange(nx)[None, :] + np.zeros((ny, 1), dtype=np.int64)
    west = east = 0
    fx = fy = 0.0
    for k in range(1, 9):
        shift = (_trt_ref.CY[k], _trt_ref.CX[k])
        counted = outer & np.roll(~blocked, shift, axis=(0, 1))
        at = np.roll(column, shift, axis=(0, 1))                 # the column of the fluid end
        term = np.roll(f[k], shift, axis=(0, 1)) + f[_trt_ref.OPP[k]]
        w, e = counted & (at == 0), counted & (at == nx - 1)
        west += int(np.count_nonzero(w))
        east += int(np.count_nonzero(e))
        fx += _trt_ref.CX[k] * float(np.sum(term[w | e]))
        fy += _trt_ref.CY[k] * float(np.sum(term[w | e]))
    return west, east, fx, fy


# ---- drivers: one per kernel family -------------------------------------------------------------------------------------

def _result(states, av, record, now):
    return SimpleNamespace(states=states, av=av, fx=None if record is None else record[0], fy=None if record is None else record[1],
                           now=now)


def set_first(handle, members, one):
    """set_wall, set_les and set_drive as the members name them, each read back, before anything else happens to the handle.
    one: an LBMDouble of members[0]; else an EnsembleDouble of all of them"""
    mode = members[0].wall
    if mode is not None:
        on = [m.wall_on if mode == "off" else m.wall for m in members]
        if one:
            handle.set_wall(*on[0])
        else:
            handle.set_wall(np.stack([w[0] for w in on]), np.stack([w[1] for w in on]), [w[2] for w in on])
        assert handle.wall() is not None
        if mode == "off":
            handle.set_wall(None, None)
            assert handle.wall() is None
    mode = members[0].les
    if mode is not None:
        cs = [m.les_on if mode == "off" else m.les for m in members]
        handle.set_les(cs[0] if one else cs)
        assert np.array_equal(np.atleast_1d(handle.les()[0]), cs)
        if mode == "off":
            handle.set_les(0.0)
            assert not np.any(handle.les()[0]) and not np.any(handle.les()[1])
    mode = members[0].drive
    if mode is not None:
        fs = [m.drive_on if mode == "off" else m.drive for m in members]
        handle.set_drive(fs[0] if one else fs)
        assert np.array_equal(np.atleast_2d(handle.drive()), fs)
        if mode == "off":
            handle.set_drive((0.0, 0.0) if one else None)
            assert not np.any(handle.drive())
    return handle


def set_scalars(handle, members):
    """set_scalar with the members' scalars, read back"""
    s = [m.scalar for m in members]
    if len(s) == 1:
        handle.set_scalar(s[0].D, s[0].c0, s[0].wall, s[0].inlet)
    else:
        handle.set_scalar([x.D for x in s], np.stack([x.c0 for x in s]), np.stack([x.wall for x in s]), np.stack([x.inlet for x in s]))
    D, om = handle.scalar()
    assert np.array_equal(np.atleast_1d(D), [x.D for x in s])
    assert np.array_equal(np.atleast_1d(om), [_scalar_ref.omega_s(x.D) for x in s])


def open_context(lbm, case, m, multistep, scalar=False):
    """member m as an uploaded LBMDouble of its own with the case's settings; scalar: and the member's scalar, set last"""
    sim = set_first(lbm.LBMDouble(m.p, m.ob), [m], True)
    sim.set_option("multistep", multistep)
    sim.set_option("force", int(case.force))
    sim.set_body(m.body)
    if m.magic:
        sim.set_trt(m.magic)
    if m.open:
        sim.set_open(*m.open)
    sim.upload(m.cells0)
    if scalar:
        set_scalars(sim, [m])
    return sim


def open_ensemble(lbm, case, scalar=False):
    """all members as one uploaded EnsembleDouble with the case's settings, each member on its own map; scalar: and the
    members' scalars, set last"""
    ms = case.members
    ens = set_first(lbm.EnsembleDouble([m.p for m in ms], np.stack([m.ob for m in ms])), ms, False)
    ens.set_option("force", int(case.force))
    if case.opened:
        ens.set_open(np.stack([m.open[0] for m in ms]), [m.open[1] for m in ms])
    ens.set_body(None if ms[0].body is None else np.stack([m.body for m in ms]))
    if case.trt:
        ens.set_trt([m.magic for m in ms])
    ens.upload(None if ms[0].cells0 is None else np.stack([m.cells0 for m in ms]))
    if scalar:
        set_scalars(ens, ms)
    return ens


def drive_context(lbm, case, runs, multistep):
    """every member as an LBMDouble of its own: d2q9_dp_step (multistep 0) or d2q9_dp_multi (8)"""
    out = []
    for m in case.members:
        with open_context(lbm, case, m, multistep) as sim:
            states, now = [], []
            for r in runs:
                now.append(sim.force())
                sim.run(r)
                states.append(sim.download(av_vels=False)[0])
            av = sim.download(cells=False)[1]
            out.append(_result(states, av, sim.force_record() if case.force else None, now))
    return out


def drive_ensemble(lbm, case, runs, gated):
    """all members in one EnsembleDouble: run() is d2q9_dp_ensemble; gated, run_until() in legs shorter than its window is
    d2q9_dp_ensemble_gated with every member active, on the drag criterion where the record is on, else on av_vels"""
    with open_ensemble(lbm, case) as ens:
        states, now, done = [], [], 0
        for r in runs:
            now.append(ens.force())
            done += r
            if gated:
                assert r < GATED_WINDOW
                steps, conv = ens.run_until(r, window=GATED_WINDOW, rel_tol=GATED_TOL, on="drag" if case.force else "av_vels")
                assert steps.tolist() == [done] * case.n and not conv.any(), (steps, conv)   # every member advanced, none stopped
            else:
                ens.run(r)
            assert ens.steps_done == done
            states.append(ens.download(av_vels=False)[0])
        av = ens.download(cells=False)[1]
        record = ens.force_record() if case.force else None
    return [_result([s[k] for s in states], av[k], None if record is None else (record[0][k], record[1][k]),
                    [(float(fx[k]), float(fy[k])) for fx, fy in now]) for k in range(case.n)]


def drive(lbm, family, case, runs):
    """per member: the downloaded state after each run, av_vels, the force record (force on) and force() before each run"""
    assert sum(runs) <= case.steps
    if family in MULTISTEP:
        return drive_context(lbm, case, runs, MULTISTEP[family])
    return drive_ensemble(lbm, case, runs, gated={"ensemble": False, "gated": True}[family])


class Once:
    """what a test module computes once per key: the chained reference of a case's members, and their runs on the device"""

    def __init__(self):
        self.refs, self.runs = {}, {}

    def reference_of(self, oracle_f64, key, case, steps):
        """the chained reference of every member; the force tuples are those of the case's bodies"""
        if key not in self.refs:
            self.refs[key] = [reference_run(oracle_f64, m, steps) for m in case.members]
        return self.refs[key]

    def run_of(self, lbm, key, family, case, runs):
        """family: one of FAMILIES, or an int: LBMDouble at that "multistep" """
        if (family,) + key not in self.runs:
            if isinstance(family, int):
                self.runs[(family,) + key] = drive_context(lbm, case, runs, family)
            else:
                self.runs[(family,) + key] = drive(lbm, family, case, runs)
        return self.runs[(family,) + key]


# ---- the gates -------------------------------------------------------------------------------------------------------------

def plus_zero(v):
    v = np.asarray(v)
    return bool(np.all(v == 0.0) and not np.any(np.signbit(v)))


def assert_equals_the_reference(case, refs, results, runs, what):
    nx, ny = case.nx, case.ny
    for k, (m, ref, got) in enumerate(zip(case.members, refs, results)):
        steps = sum(runs)
        assert got.av.shape == (steps,) and len(got.states) == len(runs)
        done, worst_av, worst_f = 0, 0.0, 0.0
        for i, r in enumerate(runs):
            done += r
            differs = int(np.count_nonzero(got.states[i] != ref.states[done]))
            assert np.array_equal(got.states[i], ref.states[done]), (what, k, done, differs)
        for t in range(steps):
            total = ref.totals[t]
            err, tol = abs(got.av[t] - total * m.p.free_cells_inv), nx * ny * U * total
            worst_av = max(worst_av, err / tol)
            assert total > 0.0 and err <= tol, (what, k, t, got.av[t], total * m.p.free_cells_inv, tol)
            if not case.force:
                continue
            if ref.forces[t] is None:
                assert plus_zero(got.fx[t]) and plus_zero(got.fy[t]), (what, k, t)
                continue
            rx, ry, links, mag = ref.forces[t]
            ftol = 8.0 * links * U * mag
            worst_f = max(worst_f, abs(got.fx[t] - rx) / ftol, abs(got.fy[t] - ry) / ftol)
            assert abs(got.fx[t] - rx) <= ftol and abs(got.fy[t] - ry) <= ftol, (what, k, t, got.fx[t], rx, got.fy[t], ry, ftol)
            assert links > 0 and mag > 0.0 and max(abs(got.fx[t]), abs(got.fy[t])) > 1e-5
        for i, r in enumerate(runs):
            if case.force:
                # the output stage: force() of the state before a run equals the entry the run's first step writes
                first = sum(runs[:i])
                assert got.now[i] == (got.fx[first], got.fy[first]), (what, k, first)
        print("%s member %d: cells equal after runs of %s steps; av_vels within %.1e of its gate, force within %.1e of its gate" %
              (what, k, runs, worst_av, worst_f))


def assert_same_bits(a, b, what):
    """two results of one case, member by member: states, av_vels, force() and, where both have it, the record"""
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert all(np.array_equal(s, t) for s, t in zip(x.states, y.states)), (what, k)
        assert np.array_equal(x.av, y.av), (what, k)
        assert x.now == y.now, (what, k)
        assert all(np.signbit(u) == np.signbit(v) for p, q in zip(x.now, y.now) for u, v in zip(p, q)), (what, k)
        if x.fx is not None and y.fx is not None:
            assert np.array_equal(x.fx, y.fx) and np.array_equal(x.fy, y.fy), (what, k)
            assert np.array_equal(np.signbit(x.fx), np.signbit(y.fx)) and np.array_equal(np.signbit(x.fy), np.signbit(y.fy)), (what, k)


# ---- the tests every option repeats: one body each ---------------------------------------------------------------------------
# once: the module's Once.  matrix_case(lbm, nx, ny, *flags, mode): the module's case with its option "on", None or "off";
# flags: (force, trt, opened, ...) as the module parametrises them.

def check_every_instance(once, matrix_case, lbm, oracle_f64, case, flags, family, nx, ny, what, fluid_alone=False,
                         force_off_against_on=False):
    """`case` (matrix_case with the option on) in `family` against the reference under the gates above; the members are
    different flows; the option changes the flow (fluid_alone: and leaves the blocked cells of the first step alone);
    force_off_against_on: FORCE off computes the bits of FORCE on; an ensemble member is its LBMDouble at "multistep" 0 and 8"""
    force, rest = flags[0], tuple(flags[1:])
    refs = once.reference_of(oracle_f64, ("matrix", nx, ny) + rest, case, sum(RUNS))
    got = once.run_of(lbm, ("matrix", nx, ny) + tuple(flags), family, case, RUNS)
    assert_equals_the_reference(case, refs, got, RUNS, what)
    assert len({r.states[-1].tobytes() for r in got}) == case.n                   # the members are different flows
    # the option changes the flow: the reference without it differs from the first step on
    plain = once.reference_of(oracle_f64, ("plain", nx, ny) + rest, matrix_case(lbm, nx, ny, *flags, None), 1)
    for m, a, b in zip(case.members, refs, plain):
        assert not np.array_equal(a.states[1], b.states[1])
        if fluid_alone:
            assert np.array_equal(a.states[1][:, m.ob != 0], b.states[1][:, m.ob != 0])
    if force_off_against_on and not force:
        # the option computes the same flow, and force() needs no option
        on = once.run_of(lbm, ("matrix", nx, ny, 1) + rest, family, matrix_case(lbm, nx, ny, 1, *rest), RUNS)
        assert_same_bits(got, on, what)
    if family in ("ensemble", "gated"):
        # a member is the LBMDouble with its setting, at "multistep" 0 and 8, bit for bit
        for other in ("dp_step", "dp_multi"):
            assert_same_bits(got, once.run_of(lbm, ("matrix", nx, ny) + tuple(flags), other, case, RUNS), what)


def check_region_wider_than_the_grid(once, lbm, oracle_f64, family, case):
    """the 6x5 case in `family`, six single steps, against the reference"""
    runs = [1] * 6
    assert (case.nx, case.ny) == (6, 5)
    refs = once.reference_of(oracle_f64, ("narrow",), case, len(runs))
    got = once.run_of(lbm, ("narrow",), family, case, runs)
    assert_equals_the_reference(case, refs, got, runs, "%s 6x5" % family)
    assert len({r.states[-1].tobytes() for r in got}) == case.n


def check_off_is_off(once, matrix_case, lbm, flags, family, nx, ny, what, off_modes, on_key, on_case, finite):
    """every mode of off_modes equals a handle that never heard of the option, bit for bit; on_case (cached under on_key) is
    another flow from the first run on, and (finite) still finite after the last"""
    flags = tuple(flags)
    never = once.run_of(lbm, ("never", nx, ny) + flags, family, matrix_case(lbm, nx, ny, *flags, None), RUNS)
    for mode in off_modes:
        got = once.run_of(lbm, (mode, nx, ny) + flags, family, matrix_case(lbm, nx, ny, *flags, mode), RUNS)
        assert_same_bits(got, never, what + " " + mode)
    on = once.run_of(lbm, (on_key, nx, ny) + flags, family, on_case, RUNS)
    assert all(not np.array_equal(a.states[0], b.states[0]) for a, b in zip(on, never))
    if finite:
        assert all(np.all(np.isfinite(a.states[-1])) for a in on)


def check_multistep_0_3_and_8_agree(once, lbm, key, make):
    """make(): the case.  LBMDouble at "multistep" 0, 3 and 8 and the ensemble's members: the same bits"""
    results = [once.run_of(lbm, key, ms, make(), RUNS) for ms in (0, 3, 8)]
    assert_same_bits(results[0], results[1], "multistep 0 against 3")
    assert_same_bits(results[0], results[2], "multistep 0 against 8")
    members = once.run_of(lbm, key, "ensemble", make(), RUNS)
    assert_same_bits(members, results[1], "member against context")


def check_one_run_of_ten_against_three_and_seven(once, lbm, family, make):
    whole = once.run_of(lbm, ("ten", 10), family, make(), [10])
    split = once.run_of(lbm, ("ten", 3, 7), family, make(), [3, 7])
    for k, (a, b) in enumerate(zip(whole, split)):
        assert np.array_equal(a.states[-1], b.states[-1]), (family, k)
        assert np.array_equal(a.av, b.av) and np.array_equal(a.fx, b.fx) and np.array_equal(a.fy, b.fy), (family, k)
        assert b.now[1] == (b.fx[3], b.fy[3])


def check_a_member_stopped_by_run_until(lbm, on, set_ensemble, set_member, title, other, final_state=False):
    """37x29, four members of the channel sweep with "force" on and the option set by set_ensemble(ens) / set_member(sim, k): a
    member that run_until stops equals an LBMDouble run to its count in cells, av_vels, the force record and force()
    (final_state: and in the four fields).  on: the criterion; None = run_until's default, av_vels, and then av_vels also equals
    the plain record.  other = (k, set_other): an LBMDouble of member k with set_other(sim) in place of its setting is another
    flow."""
    nx, ny, window, cap = 37, 29, 7, 200
    omegas = (0.6, 1.0, 1.4, 1.7)
    ob = channel(nx, ny)
    base = lbm.make_dparams(nx, ny, cap, density=0.1, accel=0.005, omega=omegas[0], obstacles=ob)
    params = lbm.sweep_dparams(base, omega=list(omegas))

    def ensemble():
        ens = lbm.EnsembleDouble(params, ob)
        ens.set_option("force", 1)
        set_ensemble(ens)
        ens.upload(None)
        return ens

    with ensemble() as ens:
        ens.run(cap)
        whole = ens.force_record()[0] if on == "drag" else ens.download(cells=False)[1]
    want_steps, want_conv = rule(whole, 0, cap, window, TOL)
    print("%s, window %d%s: stops %s converged %s" % (title % (nx, ny), window, "" if on is None else " on " + on,
                                                     want_steps.tolist(), want_conv.tolist()))
    assert np.any(want_conv) and len(set(want_steps.tolist())) >= 2
    with ensemble() as ens:
        steps, conv = ens.run_until(cap, window=window, rel_tol=TOL, **({} if on is None else {"on": on}))
        assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist()
        cells, av = ens.download()
        fx, fy = ens.force_record()
        now = ens.force()
        fields = ens.final_state() if final_state else None
    for k, p in enumerate(params):
        c = int(steps[k])
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("force", 1)
            set_member(sim, k)
            sim.upload(None)
            sim.run(c)
            rc, rav = sim.download()
            rfx, rfy = sim.force_record()
            assert np.array_equal(cells[k], rc), k
            assert np.array_equal(av[k, :c], rav), k
            if on is None:
                assert np.array_equal(av[k, :c], whole[k, :c]), k
            assert np.array_equal(fx[k, :c], rfx) and np.array_equal(fy[k, :c], rfy), k
            assert (now[0][k], now[1][k]) == sim.force(), k
            if final_state:
                assert all(np.array_equal(a[k], b) for a, b in zip(fields, sim.final_state())), k
    # the setting makes it: with the other one the member is another flow
    k, set_other = other
    with lbm.LBMDouble(params[k], ob) as sim:
        set_other(sim)
        sim.upload(None)
        sim.run(int(steps[k]))
        assert not np.array_equal(sim.download(av_vels=False)[0], cells[k])

"""The FORCE x TRT x OPEN matrix of the double-precision kernel families: masks, inputs, the routed reference and one driver
per family, shared by tests/test_dp_matrix_cpu.py (the conditions on the inputs) and tests/test_dp_matrix_gpu.py.

Nothing is restated here.  reference_step routes a state to what the suite already trusts: _open_ref.step and _open_ref.force
with open boundaries on, _trt_ref.step on test_force_gpu.accelerated(...) with test_force_gpu.restatement or
test_body_gpu.body_restatement without.  column_links names the links of _open_ref.force whose fluid end lies in column 0 or
nx - 1, by that function's own index arithmetic, for the CPU module's condition that a force pass which loses them is seen.

The masks put counted cells beside the two open columns.  With open boundaries on, the LDS-tile kernels mark the fluid cells
of those columns in their mask byte, and the force pass has to read a marked neighbour as fluid: a body away from the columns,
as every ensemble test before this one had, never asks that of it."""
from types import SimpleNamespace

import numpy as np

import _open_ref
import _trt_ref
from test_body_gpu import body_restatement
from test_dp_gpu import random_state
from test_force_gpu import accelerated, restatement

U = 2.0 ** -53
FAMILIES = ("dp_step", "dp_multi", "ensemble", "gated")
MULTISTEP = {"dp_step": 0, "dp_multi": 8}
# per member; four of each for the steady run
OMEGAS = [1.7, 1.2, 1.0, 1.45]
MAGICS = [3.0 / 16.0, 1.0 / 4.0, 1.0 / 12.0, 1.0 / 6.0]
RHOS = [0.102, 0.1, 0.0985, 0.101]
# a gated run is one leg shorter than this window: it is run and not checked (lbm_dsteady_run), so no member stops
GATED_WINDOW = 16
GATED_TOL = 2e-2


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


def make_case(lbm, nx, ny, n, steps, force, trt, opened, counted="body", beside=None, omegas=OMEGAS, profiles=None, rhos=RHOS,
              rest=False):
    """n members on matrix_mask(nx, ny, member), each with its own omega, magic parameter, inlet profile, rho_out and state.
    counted: "body" = the body of matrix_mask, "all" = every blocked cell (body None).  beside: the member whose map gets
    matrix_mask's cell beside the blocked cell of column 0.  profiles: other inlet profiles than inlet_profile's.  rest: every
    member starts from the library's rest state (cells0 None)."""
    members = []
    for k in range(n):
        ob, body = matrix_mask(nx, ny, k, beside=(k == beside))
        p = lbm.make_dparams(nx, ny, steps, density=0.1, accel=0.005, omega=omegas[k], obstacles=ob)
        u_in = inlet_profile(nx, ny, k) if profiles is None else profiles[k]
        members.append(SimpleNamespace(p=p, ob=ob, body=body if counted == "body" else None,
                                       cells0=None if rest else member_state(nx, ny, k), magic=MAGICS[k] if trt else None,
                                       open=(u_in, rhos[k]) if opened else None))
    return SimpleNamespace(nx=nx, ny=ny, n=n, steps=steps, force=bool(force), trt=bool(trt), opened=bool(opened), members=members)


def reference_step(oracle_f64, p, ob, body, f, trt_magic, open_setting):
    """One restated step of the stored state f under any flag combination: (cells, |u| with 0 on blocked cells, (F_x, F_y,
    links, sum|link terms|) of that step, or None where nothing is blocked).  trt_magic: None or 0 = BGK.  open_setting: None, or
    (u_in, rho_out)."""
    om = _trt_ref.omega_minus(p.omega, trt_magic) if trt_magic else None
    if open_setting is not None:
        u_in, rho_out = open_setting
        cells, u = _open_ref.step(f, ob, p.omega, om, u_in, rho_out)
        force = _open_ref.force(f, ob, body)
    else:
        fa = accelerated(oracle_f64, p, ob, f)
        cells, u = _trt_ref.step(fa, ob, p.omega, om)
        force = restatement(fa, ob) if body is None else body_restatement(fa, ob, body)
    return cells, u, (force if np.any(ob) else None)


def reference_run(oracle_f64, m, steps):
    """`steps` chained reference steps of member m from its first state: the state after every step (index 0: before the
    first), sum|u| and the force tuple per step"""
    states, totals, forces = [m.cells0], [], []
    for _ in range(steps):
        cells, u, force = reference_step(oracle_f64, m.p, m.ob, m.body, states[-1], m.magic, m.open)
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


def open_context(lbm, case, m, multistep):
    """member m as an uploaded LBMDouble of its own with the case's settings"""
    sim = lbm.LBMDouble(m.p, m.ob)
    sim.set_option("multistep", multistep)
    sim.set_option("force", int(case.force))
    sim.set_body(m.body)
    if m.magic:
        sim.set_trt(m.magic)
    if m.open:
        sim.set_open(*m.open)
    sim.upload(m.cells0)
    return sim


def open_ensemble(lbm, case):
    """all members as one uploaded EnsembleDouble with the case's settings, each member on its own map"""
    ms = case.members
    ens = lbm.EnsembleDouble([m.p for m in ms], np.stack([m.ob for m in ms]))
    ens.set_option("force", int(case.force))
    if case.opened:
        ens.set_open(np.stack([m.open[0] for m in ms]), [m.open[1] for m in ms])
    ens.set_body(None if ms[0].body is None else np.stack([m.body for m in ms]))
    if case.trt:
        ens.set_trt([m.magic for m in ms])
    ens.upload(None if ms[0].cells0 is None else np.stack([m.cells0 for m in ms]))
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

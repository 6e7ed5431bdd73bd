"""The scalar side of the instance matrix: every (FORCE, TRT, OPEN, WALL, LES) row of d2q9_dp_buoyant and d2q9_dp_buoyant_gated, the
steady runs with flow options on, the scalar one array off the flow, and runs across the ring of segment sums.  Shared by
tests/test_scalar_options_cpu.py (the conditions on the inputs and on the constants below) and tests/test_scalar_options_gpu.py.

Nothing is restated here.  The cases, masks, members and drivers are tests/_dp_matrix.py's; the per-member b and c_ref are those of
tests/test_buoy_gpu.py (a helper imports no test module, so they are repeated, and the CPU module holds them equal), and the
gates of a run against its reference ask what that module's and tests/test_scalar_record_gpu.py's ask.  reference() chains what
the suite already trusts: _scalar_record_ref.buoyant_advance with _buoy_ref.record for a buoyant member, tests/_dp_matrix.py's
routed reference of the flow with _scalar_record_ref.passive_entry for a passive one.  The wanted stops of a steady run are
_steady_rule.rule on that reference's record.

A row is (force, trt, open, wall, les); the body force of set_drive is on in the 16 rows with an odd number of flags set, so
F0 = 0 and F0 != 0 both meet every flag both ways.  options_of(row) appends that sixth flag."""
import itertools
from types import SimpleNamespace

import numpy as np

import _buoy_ref as bref
import _dp_matrix as dm
import _drive_ref
import _scalar_record_ref as rr
import _scalar_ref as sref
import _steady_rule

ROWS = list(itertools.product((0, 1), repeat=5))
SHAPES = [(17, 16), (33, 19)]
RUNS = [1, 2, 10]
FAMILIES = [0, 8, "ensemble", "gated"]
BS = [(3e-5, -2e-5), (-1e-5, 4e-5), (2e-5, 1e-5)]                              # per member, tests/test_buoy_gpu.py's
C_REFS = [1.0, 0.8, 1.2]
FLIPPED = (1, 2, 3, 4)                                   # trt, open, wall, les: the flags that choose another flow
# a gated run is one leg shorter than this window, so no check takes place and no member stops
GATED_WINDOW, GATED_TOL = 16, dm.GATED_TOL
assert max(RUNS) < GATED_WINDOW
STABLE = 96                                              # steps every row stays finite for in the restatement, at both shapes

# ---- the steady runs: 17x16, three members --------------------------------------------------------------------------------------
# (row, drive, buoyant) -> the criterion, the window, the tolerance and the cap.  tests/test_scalar_options_cpu.py holds every
# entry to the conditions of check_stops on the restatement alone and prints the stops.
STEADY_SHAPE = (17, 16)
STEADY = {
    ((1, 1, 1, 1, 1), 1, True): dict(on="scalar", window=7, rel_tol=3e-3, cap=63),
    ((1, 1, 0, 1, 1), 1, True): dict(on="scalar", window=7, rel_tol=3e-3, cap=70),
    ((0, 0, 1, 0, 0), 0, True): dict(on="scalar_flux_x", window=7, rel_tol=3e-2, cap=84),
    ((1, 1, 1, 1, 1), 1, False): dict(on="scalar_flux_y", window=11, rel_tol=1e-1, cap=77),
    ((1, 1, 0, 1, 1), 1, False): dict(on="scalar_flux_x", window=9, rel_tol=3e-2, cap=72),
    ((0, 0, 1, 0, 0), 0, False): dict(on="scalar", window=9, rel_tol=3e-3, cap=54),
}
# the scalar one array off the flow: run(FIRST), set_scalar again with again_c0, then run_until from s0 = FIRST.  FIRST is odd, so
# the flow is on array 1 and the scalar, set again, on array 0.
FIRST = 3
AGAIN = {
    ((1, 1, 0, 1, 1), 1, True): dict(on="scalar_flux_x", window=7, rel_tol=1e-2, cap=42),
    ((0, 0, 1, 0, 0), 0, False): dict(on="scalar_flux_y", window=7, rel_tol=1e-1, cap=21),
}
# across the ring: one call of RING_STEPS steps against RING_CALLS of RING_STEPS / RING_CALLS.  The ring holds at most kRingMax = 256
# steps (csrc/dp_host.h), so the long call flushes mid-run and a short one only at its end.
RING_STEPS, RING_CALLS, RING_MAX = 300, 3, 256
RING_BUOYANT = ((1, 1, 0, 1, 1), 1)
RING_PLAIN = ((1, 0, 0, 0, 0), 0)
RING_FAMILIES = [0, 3, 8, "ensemble"]
assert RING_STEPS // RING_CALLS < RING_MAX < RING_STEPS


def options_of(row, drive=None):
    """(force, trt, open, wall, les, drive): the body force on where the row has an odd number of flags set"""
    return tuple(row) + (sum(row) % 2 if drive is None else drive,)


def make_case(lbm, nx, ny, row, steps=sum(RUNS), drive=None, scalar=True):
    """three members of tests/_dp_matrix.py's make_case under options_of(row, drive), each with its scalar; scalar False: the flow
    alone"""
    force, trt, opened, wall, les, drive = options_of(row, drive)
    return dm.make_case(lbm, nx, ny, 3, steps, force, trt, opened, wall="on" if wall else None, les="on" if les else None,
                        drive="on" if drive else None, scalar=scalar)


def setting_of(m, k):
    """what _buoy_ref.advance needs of member k"""
    return bref.setting(m.ob, m.p.density, m.p.accel, m.p.omega, BS[k], C_REFS[k], m.scalar.D, magic=m.magic, opened=m.open,
                        wall=m.wall if isinstance(m.wall, tuple) else None, les=m.les if isinstance(m.les, float) else None,
                        drive=drive_of(m), c_wall=m.scalar.wall, c_in=m.scalar.inlet)


def again_c0(m, k):
    """the c0 of the second set_scalar: another field in 0.5 .. 1.5"""
    ny, nx = m.ob.shape
    return 0.5 + np.random.default_rng(9500 + 100 * nx + 10 * ny + k).random((ny, nx))


def drive_of(m):
    return m.drive if isinstance(m.drive, tuple) else None


# ---- the routed reference ------------------------------------------------------------------------------------------------------

def reference(oracle_f64, case, steps, buoyant=True, again=None):
    """per member: both states after every step (index 0: before the first), the three records float64[3, steps], and for a
    buoyant member av_vels and the force record as the device adds them (fx, fy None with FORCE off); for a passive one `flow`,
    tests/_dp_matrix.py's reference_run.  again: None, or the step count at which the scalar starts anew from again_c0 (g[again] is
    that new state); the flow and the records go on."""
    out = []
    for k, m in enumerate(case.members):
        g, rec = [sref.init(m.scalar.c0)], []
        av, fx, fy, s, flow = [], [], [], None, None
        if buoyant:
            s = setting_of(m, k)
            counted = bref.counted_cells(m.ob, m.body, m.open is not None) if case.force else None
            f = [m.cells0]
            for n in range(steps):
                if n == again:
                    g[-1] = sref.init(again_c0(m, k))
                f1, g1, r, u, fa = rr.buoyant_advance(f[-1], g[-1], s)
                a, x, y = bref.record(u, fa, m.ob, m.p.free_cells_inv, counted)
                f.append(f1), g.append(g1), rec.append(r), av.append(a), fx.append(x), fy.append(y)
        else:
            # the flow by the routed reference of tests/_dp_matrix.py, the scalar on the state each flow step streams
            flow = dm.reference_run(oracle_f64, m, steps)
            f = flow.states
            for n in range(steps):
                if n == again:
                    g[-1] = sref.init(again_c0(m, k))
                fa = f[n] if m.open is not None else sref.accelerate(f[n], m.ob, m.p.density, m.p.accel)
                g1, r = rr.passive_entry(fa, g[-1], m.ob, sref.omega_s(m.scalar.D), drive_of(m), m.scalar.wall,
                                         m.scalar.inlet if m.open is not None else None)
                g.append(g1), rec.append(r)
        out.append(SimpleNamespace(s=s, f=f, g=g, rec=np.array(rec).T, av=np.array(av) if buoyant else None,
                                   fx=np.array(fx) if buoyant and case.force else None,
                                   fy=np.array(fy) if buoyant and case.force else None, flow=flow))
    return out


class Once:
    """what a module computes once per key: the reference of a case, and its runs on the device.  The matrix has 64 keys of four
    families, and a key's arrays are of no use once it has gone by: the runs, and the references asked for with passing=True,
    are kept for one key at a time."""

    def __init__(self):
        self.refs, self.runs, self.key, self.passing = {}, {}, None, (None, None)

    def reference_of(self, oracle_f64, key, case, steps, buoyant=True, again=None, passing=False):
        if passing:
            if self.passing[0] != key:
                self.passing = (key, reference(oracle_f64, case, steps, buoyant, again))
            return self.passing[1]
        if key not in self.refs:
            self.refs[key] = reference(oracle_f64, case, steps, buoyant, again)
        return self.refs[key]

    def run_of(self, lbm, key, family, case, runs):
        if key != self.key:
            self.runs, self.key = {}, key
        if family not in self.runs:
            self.runs[family] = drive(lbm, family, case, runs)
        return self.runs[family]


def finite(refs):
    return all(np.all(np.isfinite(r.f[-1])) and np.all(np.isfinite(r.g[-1])) and np.all(np.isfinite(r.rec)) for r in refs)


# ---- the steady rule on the reference ------------------------------------------------------------------------------------------

def which_of(const):
    return rr.NAMES.index({v: k for k, v in rr.CRITERIA.items()}[const["on"]])


def wanted_stops(records, const, s0=0):
    """_steady_rule.rule on the members' records [3, >= s0 + cap] of a plain run to the cap: (steps, converged)"""
    chosen = np.ascontiguousarray(np.stack([np.asarray(r)[which_of(const)] for r in records]))
    return _steady_rule.rule(chosen, s0, const["cap"], const["window"], const["rel_tol"])


def check_stops(steps, conv, const, s0=0):
    """the conditions a steady case must meet for its run to leave members on both arrays; returns how many members reach the cap
    unconverged"""
    steps, conv = [int(v) for v in steps], [bool(v) for v in conv]
    stopped = [s for s, c in zip(steps, conv) if c]
    assert len(set(stopped)) >= 2, (steps, conv)                                  # two different counts among those that converge
    assert {s % 2 for s in stopped} == {0, 1}, (steps, conv)                       # one odd, one even: both arrays hold states
    if s0 == 0:
        assert min(steps) > const["window"], steps                                # no stop at the first check point
    else:
        # the first check point reads an entry from before the second set_scalar: it exists, so that branch is taken
        first = s0 + const["window"]
        assert first - const["window"] >= 1
    assert all(s == s0 + const["cap"] for s, c in zip(steps, conv) if not c)
    return sum(1 for c in conv if not c)


# ---- drivers --------------------------------------------------------------------------------------------------------------------

def set_on(handle, ks, buoyant=True):
    """behind the upload and the scalars: the members' buoyancy, read back, and the record"""
    assert handle.buoyancy() is None and not handle.scalar_record_on()
    if buoyant and len(ks) == 1:
        handle.set_buoyancy(BS[ks[0]], C_REFS[ks[0]])
        assert handle.buoyancy() == (BS[ks[0]], C_REFS[ks[0]])
    elif buoyant:
        handle.set_buoyancy([BS[k] for k in ks], [C_REFS[k] for k in ks])
        assert np.array_equal(handle.buoyancy(), [BS[k] + (C_REFS[k],) for k in ks])
    handle.set_scalar_record(True)
    assert handle.scalar_record_on()
    return handle


def open_ensemble(lbm, case, buoyant=True):
    return set_on(dm.open_ensemble(lbm, case, scalar=True), list(range(case.n)), buoyant)


def open_member(lbm, case, k, multistep, buoyant=True):
    return set_on(dm.open_context(lbm, case, case.members[k], multistep, scalar=True), [k], buoyant)


def set_scalar_again(handle, members, ks):
    """set_scalar once more, after steps: the members' D, walls and inlets with again_c0"""
    s = [members[k].scalar for k in ks]
    c0 = [again_c0(members[k], k) for k in ks]
    if len(ks) == 1:
        handle.set_scalar(s[0].D, c0[0], s[0].wall, s[0].inlet)
    else:
        handle.set_scalar([x.D for x in s], np.stack(c0), np.stack([x.wall for x in s]), np.stack([x.inlet for x in s]))


def drive(lbm, family, case, runs):
    """A buoyant case with the record on in one family, tests/test_scalar_record_gpu.py's result per member: the flow's state, the
    scalar's populations, final_state and the three records after each run, av_vels and the force record.  family: LBMDouble at
    that "multistep", "ensemble" (EnsembleDouble.run) or "gated" (run_until on "scalar" in legs shorter than its window:
    d2q9_dp_buoyant_gated and dp_scalar_step_rec<true> with every member active)."""
    def loop(handle, gated=False):
        states, g, fin, rec, done = [], [], [], [], 0
        for r in runs:
            done += r
            if gated:
                assert r < GATED_WINDOW
                steps, conv = handle.run_until(r, window=GATED_WINDOW, rel_tol=GATED_TOL, on="scalar")
                assert steps.tolist() == [done] * case.n and not conv.any(), (steps, conv)   # every member advanced, none stopped
            else:
                handle.run(r)
            assert handle.steps_done == done
            states.append(handle.download(av_vels=False)[0])
            g.append(handle.scalar_cells())
            fin.append(handle.final_state())
            rec.append(handle.scalar_record())
        return states, g, fin, rec, handle.download(cells=False)[1], (handle.force_record() if case.force else None)

    results = []
    if family in ("ensemble", "gated"):
        with open_ensemble(lbm, case) as ens:
            states, g, fin, rec, av, force = loop(ens, family == "gated")
        for k in range(case.n):
            results.append(SimpleNamespace(states=[s[k] for s in states], g=[x[k] for x in g], fin=[[a[k] for a in x] for x in fin],
                                           rec=[np.stack([v[k] for v in r]) for r in rec], av=av[k],
                                           fx=None if force is None else force[0][k], fy=None if force is None else force[1][k]))
    else:
        for k in range(case.n):
            with open_member(lbm, case, k, family) as sim:
                states, g, fin, rec, av, force = loop(sim)
            results.append(SimpleNamespace(states=states, g=g, fin=fin, rec=[np.stack(r) for r in rec], av=av,
                                           fx=None if force is None else force[0], fy=None if force is None else force[1]))
    return results


def assert_equals_the_reference(case, refs, got, runs, what):
    """after each run cells, scalar populations, the four fields and the three records, and at the end av_vels and the force record
    (FORCE on): np.array_equal throughout"""
    for k, (ref, res) in enumerate(zip(refs, got)):
        done = 0
        for i, r in enumerate(runs):
            done += r
            assert np.array_equal(res.g[i], ref.g[done]), (what, k, done, int(np.count_nonzero(res.g[i] != ref.g[done])))
            assert np.array_equal(res.states[i], ref.f[done]), (what, k, done, int(np.count_nonzero(res.states[i] != ref.f[done])))
            for name, a, b in zip(("u_x", "u_y", "u", "pressure"), res.fin[i], bref.final_state(ref.f[done], ref.g[done], ref.s)):
                assert np.array_equal(a, b), (what, k, done, name)
            assert res.rec[i].shape == (3, done)
            for v, name in enumerate(rr.NAMES):
                assert np.array_equal(res.rec[i][v], ref.rec[v, :done]), (what, k, done, name, res.rec[i][v], ref.rec[v, :done])
        assert res.av.shape == (done,) and np.array_equal(res.av, ref.av[:done]), (what, k, res.av, ref.av)
        if case.force:
            assert np.array_equal(res.fx, ref.fx[:done]) and np.array_equal(res.fy, ref.fy[:done]), (what, k, res.fx, ref.fx, res.fy, ref.fy)
            assert np.any(res.fx != 0.0)
        else:
            assert res.fx is None and res.fy is None
        assert np.all(np.isfinite(res.g[-1])) and np.all(np.isfinite(res.states[-1])), (what, k)
        assert np.all(np.isfinite(res.rec[-1])) and np.all(res.rec[-1][0] > 0.0) and np.all(res.rec[-1][1:] != 0.0), (what, k)


def assert_same_bits(a, b, what):
    """two results of one case, member by member, in everything drive() reads"""
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert len(x.states) == len(y.states)
        assert all(np.array_equal(s, t) for s, t in zip(x.states, y.states)), (what, k)
        assert all(np.array_equal(s, t) for s, t in zip(x.g, y.g)), (what, k)
        assert all(np.array_equal(s, t) for p, q in zip(x.fin, y.fin) for s, t in zip(p, q)), (what, k)
        assert all(np.array_equal(s, t) for s, t in zip(x.rec, y.rec)), (what, k)
        assert np.array_equal(x.av, y.av), (what, k)
        assert (x.fx is None) == (y.fx is None)
        if x.fx is not None:
            assert np.array_equal(x.fx, y.fx) and np.array_equal(x.fy, y.fy), (what, k)


# what a handle is read in, in everything()'s order; SERIES: the entries with one value per step
NAMES = ("cells", "scalar cells", "av_vels") + rr.NAMES + ("u_x", "u_y", "u", "pressure", "scalar field", "F_x record", "F_y record",
                                                           "force() x", "force() y")
SERIES = (2, 3, 4, 5, 11, 12)


def everything(h, force, k=None):
    """what a member is compared in (NAMES; the last four with FORCE on); k: member k of an ensemble's arrays"""
    cells, av = h.download()
    out = [cells, h.scalar_cells(), av] + list(h.scalar_record()) + list(h.final_state()) + [h.scalar_field()]
    if force:
        out += list(h.force_record()) + [np.asarray(v) for v in h.force()]
    return out if k is None else [a[k] for a in out]


def cut(values, c):
    """a member's values with every series cut to its first c entries"""
    return [a[:c] if i in SERIES else a for i, a in enumerate(values)]


def assert_same_values(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.shape(x) == np.shape(y) and np.array_equal(x, y), (what, NAMES[i])


def assert_member_is_the_reference(case, k, ref, mine, c, now0, buoyant, what):
    """a member's values (everything, cut to its count c) against the reference's state c.  Buoyant: all of it by np.array_equal.
    Passive: both states, the records, the fields (_drive_ref.fields) and the scalar field by np.array_equal, av_vels and the force
    under tests/_dp_matrix.py's gates.  now0: force() before the first step, for that gate.  The reference has c + 1 steps where
    FORCE is on: force() of state c is the entry step c + 1 writes."""
    m = case.members[k]
    assert np.array_equal(mine[0], ref.f[c]), (what, k, c, "cells")
    assert np.array_equal(mine[1], ref.g[c]), (what, k, c, "scalar cells")
    for v, name in enumerate(rr.NAMES):
        assert np.array_equal(mine[3 + v], ref.rec[v, :c]), (what, k, c, name, mine[3 + v], ref.rec[v, :c])
    assert np.array_equal(mine[10], sref.field(ref.g[c], m.ob)), (what, k, c, "scalar field")
    if buoyant:
        want = bref.final_state(ref.f[c], ref.g[c], ref.s)
        assert np.array_equal(mine[2], ref.av[:c]), (what, k, c, "av_vels")
        if case.force:
            assert np.array_equal(mine[11], ref.fx[:c]) and np.array_equal(mine[12], ref.fy[:c]), (what, k, c, "force record")
            assert (mine[13], mine[14]) == (ref.fx[c], ref.fy[c]), (what, k, c, "force()")
            assert np.any(mine[11] != 0.0)
    else:
        want = _drive_ref.fields(ref.f[c], m.ob, m.p.density, drive_of(m))
        one = SimpleNamespace(nx=case.nx, ny=case.ny, force=case.force, members=[m])
        res = SimpleNamespace(states=[mine[0]], av=mine[2], fx=mine[11] if case.force else None, fy=mine[12] if case.force else None,
                              now=[now0])
        dm.assert_equals_the_reference(one, [ref.flow], [res], [c], "%s member %d" % (what, k))
    for name, a, b in zip(("u_x", "u_y", "u", "pressure"), mine[6:10], want):
        assert np.array_equal(a, b), (what, k, c, name)

"""The buoyant and scalar kernels with flow options on, on the GPU: every instance of d2q9_dp_buoyant and d2q9_dp_buoyant_gated,
steady runs that stop members of flows with options on, the scalar one array off the flow, and runs across the ring of segment
sums, against tests/_scalar_options.py's routed reference by np.array_equal.

Where the 32 instances <FORCE, TRT, OPEN, WALL, LES> of each kernel are launched:
  d2q9_dp_buoyant        32 of 32: test_every_instance, in LBMDouble at "multistep" 0 and 8 and in EnsembleDouble.run
  d2q9_dp_buoyant_gated  32 of 32: test_every_instance in the family "gated" (every member active); <1,1,1,1,1>, <1,1,0,1,1> and
                         <0,0,1,0,0> with members that stop: test_a_steady_run_stops_members_with_options_on
dp_scalar_step_rec<true> runs under `active` beside each of them, with OPEN on in 16 rows; dp_scalar_step_rec<false> and
d2q9_dp_ensemble_gated at T = 1 beside a scalar in the passive steady cases.

  A. every instance: 17x16 and 33x19, all 32 rows, the body force on in the 16 rows with an odd number of flags set, three buoyant
     members with the record on, runs of 1, 2 and 10 steps, in four families: cells, scalar populations, the three records,
     av_vels, the force record (FORCE on) and the four fields equal the reference after each run; a member equals its context,
     gated equals ensemble, the members are different flows;
  B. steady runs, 17x16: three rows, each buoyant and passive, the constants of _scalar_options.STEADY (held to their conditions
     by tests/test_scalar_options_cpu.py).  The wanted stops are _steady_rule.rule on the reference's record; a plain run to the
     cap equals the reference in every entry, run_until returns the wanted stops, every member equals an LBMDouble run to its
     count in one call and the reference's state there, in everything() of _scalar_options; +0.0 beyond a member's count; the
     upload that ends raggedness;
  C. the scalar one array off the flow: run(3), set_scalar again, run_until from s0 = 3, buoyant and passive; the ragged reads,
     the upload; and with rel_tol 0.0 the run that is not ragged, then upload_scalar(scalar_cells()) and run(2);
  D. across the ring: one call of 300 steps against three of 100, LBMDouble at "multistep" 0, 3 and 8 and EnsembleDouble.run,
     a buoyant case with the record on and a case without a scalar: equal by bits, and every entry equals the reference.

The comparisons with numpy rest on the device's double-precision division and square root being correctly rounded, as those of
tests/test_scalar_gpu.py do.  Bits are asked for, and bits hold: on an MI355X all 274 cases pass in 8.2 s, the longest the first
case across the ring (0.8 s, with the reference of its 300 steps), a steady case 0.2 s, a case of the matrix 0.05 s and less.
With the scalar's offset read as 0 in csrc/lbm_dens.cpp (scalar_place, final_fields_dens, the gather of lbm_dens_upload and the
line behind a run that is not ragged), the four cases of C fail and every other case of B and C passes."""
import numpy as np
import pytest

import _dp_matrix as dm
import _scalar_options as so
import _scalar_record_ref as rr
import _steady_rule

pytestmark = pytest.mark.gpu

once = so.Once()
flows = dm.Once()


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def name_of(row, drive=None):
    return ",".join(map(str, so.options_of(row, drive)))


# ---- A. every instance, plain and gated ----------------------------------------------------------------------------------------
# the family varies fastest, so a (shape, row)'s reference and runs are computed once and dropped when the next key comes

@pytest.mark.parametrize("family", so.FAMILIES)
@pytest.mark.parametrize("row", so.ROWS, ids=lambda r: "".join(map(str, r)))
@pytest.mark.parametrize("nx,ny", so.SHAPES)
def test_every_instance(lbm, oracle_f64, nx, ny, row, family):
    what = "%s<%s> %dx%d" % (family, name_of(row), nx, ny)
    key = (nx, ny) + row
    case = so.make_case(lbm, nx, ny, row)
    refs = once.reference_of(oracle_f64, key, case, sum(so.RUNS), passing=True)
    got = once.run_of(lbm, key, family, case, so.RUNS)
    so.assert_equals_the_reference(case, refs, got, so.RUNS, what)
    assert len({r.states[-1].tobytes() for r in got}) == case.n                     # the members are different flows
    assert len({r.rec[-1].tobytes() for r in got}) == case.n
    if family == "ensemble":
        for other in (0, 8):                                                        # a member is its context, bit for bit
            so.assert_same_bits(got, once.run_of(lbm, key, other, case, so.RUNS), what)
    if family == "gated":
        so.assert_same_bits(got, once.run_of(lbm, key, "ensemble", case, so.RUNS), what)


# ---- B and C. steady runs with options on; the scalar one array off the flow ---------------------------------------------------

def steady_case(lbm, oracle_f64, key, const, again):
    """the case, its reference (one step beyond the cap: force() of the state at the cap) and the wanted stops"""
    row, drive, buoyant = key
    nx, ny = so.STEADY_SHAPE
    s0 = again or 0
    steps = s0 + const["cap"] + 1
    case = so.make_case(lbm, nx, ny, row, steps + 2, drive)
    refs = once.reference_of(oracle_f64, ("steady", again) + key, case, steps, buoyant, again)
    want_steps, want_conv = so.wanted_stops([r.rec for r in refs], const, s0)
    return case, refs, s0, want_steps, want_conv


def start(h, case, ks, again):
    """the calls before the steady run: force() of the first state, and with `again` run(FIRST) and set_scalar once more"""
    now0 = h.force() if case.force else None
    if again:
        h.run(again)
        so.set_scalar_again(h, case.members, ks)
    return now0


def check_the_upload_that_ends_raggedness(lbm, case, ens, got, buoyant):
    """upload() of the downloaded flow: the scalar populations are unchanged, and one more step is a context's from those two
    states"""
    flow, before = got[0], got[1]
    ens.upload(flow)
    assert np.array_equal(ens.scalar_cells(), before) and ens.steps_done == 0
    ens.run(1)
    after = so.everything(ens, case.force)
    for k in range(case.n):
        with so.open_member(lbm, case, k, 0, buoyant) as sim:
            sim.upload(flow[k])
            sim.upload_scalar(before[k])
            sim.run(1)
            so.assert_same_values([a[k] for a in after], so.everything(sim, case.force), ("after the upload", k))


def check_a_steady_run(lbm, oracle_f64, key, const, again=None):
    row, drive, buoyant = key
    what = "%s <%s>%s" % ("buoyant" if buoyant else "passive", name_of(row, drive), " set again" if again else "")
    case, refs, s0, want_steps, want_conv = steady_case(lbm, oracle_f64, key, const, again)
    n, cap, window, tol, which = case.n, const["cap"], const["window"], const["rel_tol"], so.which_of(const)
    everyone = list(range(n))
    print("%s on %s, window %d, rel_tol %g, from %d for up to %d: wanted stops %s converged %s" %
          (what, const["on"], window, tol, s0, cap, want_steps.tolist(), want_conv.tolist()))
    so.check_stops(want_steps, want_conv, const, s0)
    # the wanted stops never come from run_until: a plain run to the cap equals the reference in every entry of the three records,
    # and the rule on the device's own record gives the same stops
    with so.open_ensemble(lbm, case, buoyant) as ens:
        start(ens, case, everyone, again)
        ens.run(cap)
        whole = ens.scalar_record()
    for k in range(n):
        for v, name in enumerate(rr.NAMES):
            assert np.array_equal(whole[v][k], refs[k].rec[v, :s0 + cap]), (what, k, name)
    dev_steps, dev_conv = _steady_rule.rule(np.ascontiguousarray(whole[which]), s0, cap, window, tol)
    assert dev_steps.tolist() == want_steps.tolist() and dev_conv.tolist() == want_conv.tolist()
    with so.open_ensemble(lbm, case, buoyant) as ens:
        now0 = start(ens, case, everyone, again)
        steps, conv = ens.run_until(cap, window=window, rel_tol=tol, on=const["on"])
        assert steps.tolist() == want_steps.tolist() and conv.tolist() == want_conv.tolist(), (steps, conv)
        ms, mc = ens.member_steps()
        T = ens.steps_done
        assert ms.tolist() == want_steps.tolist() and mc.tolist() == want_conv.tolist() and T == max(want_steps)
        assert len(set(steps.tolist())) > 1                                         # ragged: every read below is a ragged read
        got = so.everything(ens, case.force)
        for k in range(n):
            c = int(steps[k])
            for i in so.SERIES:
                if i < len(got):
                    assert got[i].shape == (n, T) and dm.plus_zero(got[i][k, c:]), (what, k, so.NAMES[i])   # +0.0 beyond its count
            mine = so.cut([a[k] for a in got], c)
            # an LBMDouble of that member, the same calls, run to the count in one call
            with so.open_member(lbm, case, k, (0, 8, 0)[k], buoyant) as sim:
                start(sim, case, [k], again)
                sim.run(c - s0)
                so.assert_same_values(mine, so.everything(sim, case.force), (what, "member against context", k))
            so.assert_member_is_the_reference(case, k, refs[k], mine, c, None if now0 is None else (float(now0[0][k]), float(now0[1][k])),
                                              buoyant, what)
        check_the_upload_that_ends_raggedness(lbm, case, ens, got, buoyant)


def steady_ids(table):
    return ["%s-%s" % ("".join(map(str, k[0] + (k[1],))), "buoyant" if k[2] else "passive") for k in table]


@pytest.mark.parametrize("key", list(so.STEADY), ids=steady_ids(so.STEADY))
def test_a_steady_run_stops_members_with_options_on(lbm, oracle_f64, key):
    check_a_steady_run(lbm, oracle_f64, key, so.STEADY[key])


@pytest.mark.parametrize("key", list(so.AGAIN), ids=steady_ids(so.AGAIN))
def test_a_steady_run_with_the_scalar_one_array_off_the_flow(lbm, oracle_f64, key):
    check_a_steady_run(lbm, oracle_f64, key, so.AGAIN[key], so.FIRST)


@pytest.mark.parametrize("key", list(so.AGAIN), ids=steady_ids(so.AGAIN))
def test_one_array_off_and_not_ragged(lbm, oracle_f64, key):
    """rel_tol 0.0 stops nobody: the run ends with every member at the cap, and the scalar's current array is the flow's less the
    offset.  upload_scalar(scalar_cells()) followed by run(2) equals the context."""
    row, drive, buoyant = key
    const = dict(so.AGAIN[key], rel_tol=0.0, cap=2 * so.AGAIN[key]["window"])
    case, refs, s0, _, _ = steady_case(lbm, oracle_f64, key, so.AGAIN[key], so.FIRST)
    cap = const["cap"]
    assert s0 + cap + 2 <= case.steps and s0 + cap + 2 <= len(refs[0].g) - 1
    with so.open_ensemble(lbm, case, buoyant) as ens:
        now0 = start(ens, case, list(range(case.n)), so.FIRST)
        steps, conv = ens.run_until(cap, window=const["window"], rel_tol=0.0, on=const["on"])
        assert steps.tolist() == [s0 + cap] * case.n and not conv.any() and ens.steps_done == s0 + cap
        first = so.everything(ens, case.force)
        ens.upload_scalar(ens.scalar_cells())
        ens.run(2)
        second = so.everything(ens, case.force)
    for k in range(case.n):
        with so.open_member(lbm, case, k, (8, 0, 8)[k], buoyant) as sim:
            start(sim, case, [k], so.FIRST)
            sim.run(cap)
            so.assert_same_values([a[k] for a in first], so.everything(sim, case.force), ("not ragged", k))
            sim.upload_scalar(sim.scalar_cells())
            sim.run(2)
            so.assert_same_values([a[k] for a in second], so.everything(sim, case.force), ("not ragged, two more steps", k))
        at = None if now0 is None else (float(now0[0][k]), float(now0[1][k]))
        so.assert_member_is_the_reference(case, k, refs[k], [a[k] for a in first], s0 + cap, at, buoyant, "not ragged")
        so.assert_member_is_the_reference(case, k, refs[k], [a[k] for a in second], s0 + cap + 2, at, buoyant, "not ragged + 2")


# ---- D. across the ring --------------------------------------------------------------------------------------------------------

RING_RUNS = [[so.RING_STEPS], [so.RING_STEPS // so.RING_CALLS] * so.RING_CALLS]


@pytest.mark.parametrize("family", so.RING_FAMILIES)
def test_across_the_ring_buoyant_with_the_record(lbm, oracle_f64, family):
    nx, ny = so.STEADY_SHAPE
    row, drive = so.RING_BUOYANT
    case = so.make_case(lbm, nx, ny, row, so.RING_STEPS, drive)
    refs = once.reference_of(oracle_f64, "ring", case, so.RING_STEPS)
    whole, split = (so.drive(lbm, family, case, runs) for runs in RING_RUNS)
    for k, (a, b) in enumerate(zip(whole, split)):
        assert np.array_equal(a.states[-1], b.states[-1]) and np.array_equal(a.g[-1], b.g[-1]), (family, k)
        assert np.array_equal(a.av, b.av) and np.array_equal(a.fx, b.fx) and np.array_equal(a.fy, b.fy), (family, k)
        assert np.array_equal(a.rec[-1], b.rec[-1]) and a.rec[-1].shape == (3, so.RING_STEPS), (family, k)
    # every entry of every record equals the reference
    so.assert_equals_the_reference(case, refs, whole, RING_RUNS[0], "%s, one call" % family)
    so.assert_equals_the_reference(case, refs, split, RING_RUNS[1], "%s, three calls" % family)


@pytest.mark.parametrize("family", so.RING_FAMILIES)
def test_across_the_ring_without_a_scalar(lbm, oracle_f64, family):
    nx, ny = so.STEADY_SHAPE
    row, drive = so.RING_PLAIN
    case = so.make_case(lbm, nx, ny, row, so.RING_STEPS, drive, scalar=False)
    assert case.force
    refs = flows.reference_of(oracle_f64, ("ring",), case, so.RING_STEPS)
    if family == "ensemble":
        run = lambda runs: dm.drive_ensemble(lbm, case, runs, False)                # noqa: E731
    else:
        run = lambda runs: dm.drive_context(lbm, case, runs, family)                # noqa: E731
    whole, split = run(RING_RUNS[0]), run(RING_RUNS[1])
    for k, (a, b) in enumerate(zip(whole, split)):
        assert np.array_equal(a.states[-1], b.states[-1]), (family, k)
        assert np.array_equal(a.av, b.av) and np.array_equal(a.fx, b.fx) and np.array_equal(a.fy, b.fy), (family, k)
        assert a.av.shape == a.fx.shape == a.fy.shape == (so.RING_STEPS,)
    dm.assert_equals_the_reference(case, refs, whole, RING_RUNS[0], "%s, one call" % family)
    dm.assert_equals_the_reference(case, refs, split, RING_RUNS[1], "%s, three calls" % family)

"""The inputs and constants of tests/test_scalar_options_gpu.py held to what that module needs of them, without a GPU, on the
restatement alone (tests/_scalar_options.py's reference: _scalar_record_ref.buoyant_advance and passive_entry chained).

  1. the rows: all 32, the body force on in the 16 with an odd number of flags set, so every flag meets F0 = 0 and F0 != 0 both
     ways;
  2. the rows are told apart: at both shapes and for every member the state after the first step of a row differs from that of
     every row reached by flipping one of trt, open, wall, les (64 pairs a shape and member), and from the same row with the body
     force flipped; where FORCE is on the force record's first entry is not zero.  A launch that took another instance for a row
     cannot equal that row's reference;
  3. every row at both shapes stays finite in the restatement for 96 steps: the 13 steps the GPU module runs are well inside
     that.  The first states that are not finite: step 97 of member 0 of row (0,0,1,1,0) at 33x19, step 98 of member 2 of the
     row with everything on at 17x16; every row without OPEN stays finite for 130 steps and more;
  4. the steady cases: every member finite through the cap; two different counts among the members that converge, one odd and one
     even, so both arrays hold states; no stop at the first check point; two of the three criteria; over the six cases at least
     two with a member that reaches the cap unconverged.  The stops are printed;
  5. the cases with the scalar set again after three steps: the same conditions on the restatement of that sequence, and the first
     check point reads an entry from before the second set_scalar;
  6. the two cases that cross the ring stay finite through their 300 steps, and their records keep changing across the flush
     points, so an entry written to the wrong slot is seen.

A change of a constant that loses raggedness fails here and not on the GPU."""
import numpy as np
import pytest

import _dp_matrix as dm
import _scalar_options as so
import test_buoy_gpu

once = so.Once()


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def test_the_rows():
    assert len(so.ROWS) == len(set(so.ROWS)) == 32
    opts = [so.options_of(row) for row in so.ROWS]
    assert sum(o[5] for o in opts) == 16 and all(o[5] == sum(o[:5]) % 2 for o in opts)
    for flag in range(5):
        for value in (0, 1):
            assert {o[5] for o in opts if o[flag] == value} == {0, 1}, (flag, value)
    assert set(so.SHAPES) == {(17, 16), (33, 19)} and so.RUNS == [1, 2, 10] and so.GATED_WINDOW == 16
    assert so.BS == test_buoy_gpu.BS and so.C_REFS == test_buoy_gpu.C_REFS          # the per-member b and c_ref of that module


@pytest.mark.parametrize("nx,ny", so.SHAPES)
def test_the_rows_are_told_apart(lbm, oracle_f64, nx, ny):
    first = {}
    for row in so.ROWS:
        for drive in (0, 1):
            first[row, drive] = so.reference(oracle_f64, so.make_case(lbm, nx, ny, row, 1, drive), 1)
    pairs = 0
    for row in so.ROWS:
        drive = so.options_of(row)[5]
        mine = first[row, drive]
        for flag in so.FLIPPED:
            other = tuple(v ^ 1 if i == flag else v for i, v in enumerate(row))
            pairs += 1
            for k in range(3):
                # the same body force on both sides, and the other row's own: one flag apart is another flow either way
                assert not np.array_equal(mine[k].f[1], first[other, drive][k].f[1]), (row, other, k)
                assert not np.array_equal(mine[k].f[1], first[other, drive ^ 1][k].f[1]), (row, other, k)
        for k in range(3):
            assert not np.array_equal(mine[k].f[1], first[row, drive ^ 1][k].f[1]), (row, k)
            assert np.all(np.isfinite(mine[k].f[1])) and np.all(np.isfinite(mine[k].g[1]))
            if row[0]:
                assert mine[k].fx[0] != 0.0 and mine[k].fy[0] != 0.0, (row, k)
            else:
                assert mine[k].fx is None
            # FORCE chooses no other flow: its row pair differs in the record alone
            twin = first[(row[0] ^ 1,) + row[1:], drive][k]
            assert np.array_equal(mine[k].f[1], twin.f[1]) and np.array_equal(mine[k].rec, twin.rec)
    assert pairs == 128                                                             # 64 pairs, each from both of its ends


@pytest.mark.parametrize("nx,ny", so.SHAPES)
def test_every_row_stays_finite(lbm, oracle_f64, nx, ny):
    steps = so.STABLE
    assert steps >= 7 * sum(so.RUNS)
    for row in so.ROWS:
        refs = so.reference(oracle_f64, so.make_case(lbm, nx, ny, row, steps), steps)
        assert so.finite(refs), row
        assert len({r.f[-1].tobytes() for r in refs}) == 3                          # the members are different flows
        # what the GPU module's gate asks of the records it reads
        assert all(np.all(r.rec[0, :sum(so.RUNS)] > 0.0) and np.all(r.rec[1:, :sum(so.RUNS)] != 0.0) for r in refs), row


def passes_the_flow_gates_own_conditions(flow):
    """what _dp_matrix.assert_equals_the_reference asks of a reference before it compares: a mean speed and a force to speak of"""
    return all(t > 0.0 for t in flow.totals) and all(f[2] > 0 and f[3] > 0.0 and max(abs(f[0]), abs(f[1])) > 2e-5 for f in flow.forces)


def steady_reference(lbm, oracle_f64, key, const, again=None):
    row, drive, buoyant = key
    nx, ny = so.STEADY_SHAPE
    steps = (again or 0) + const["cap"] + 1
    case = so.make_case(lbm, nx, ny, row, steps + 2, drive)
    return so.reference(oracle_f64, case, steps, buoyant, again)


def test_the_steady_cases_leave_members_on_both_arrays(lbm, oracle_f64):
    assert [(k[0] + (k[1],), k[2]) for k in so.STEADY] == [(r, b) for b in (True, False)
                                                           for r in ((1, 1, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (0, 0, 1, 0, 0, 0))]
    at_cap = []
    for key, const in so.STEADY.items():
        refs = steady_reference(lbm, oracle_f64, key, const)
        assert so.finite(refs), key
        assert all(r.flow is None or not key[0][0] or passes_the_flow_gates_own_conditions(r.flow) for r in refs), key
        steps, conv = so.wanted_stops([r.rec for r in refs], const)
        print("17x16 <%s> %s on %s, window %d, rel_tol %g, cap %d: stops %s converged %s" %
              (",".join(map(str, so.options_of(key[0], key[1]))), "buoyant" if key[2] else "passive", const["on"], const["window"],
               const["rel_tol"], const["cap"], steps.tolist(), conv.tolist()))
        at_cap.append(so.check_stops(steps, conv, const))
    assert len({c["on"] for c in so.STEADY.values()}) >= 2
    assert sum(1 for v in at_cap if v) >= 2, at_cap


def test_the_cases_with_the_scalar_set_again(lbm, oracle_f64):
    assert so.FIRST % 2 == 1                                                        # the flow on array 1, the scalar anew on array 0
    assert any(k[2] for k in so.AGAIN) and not all(k[2] for k in so.AGAIN) and all(k in so.STEADY for k in so.AGAIN)
    for key, const in so.AGAIN.items():
        refs = steady_reference(lbm, oracle_f64, key, const, so.FIRST)
        plain = steady_reference(lbm, oracle_f64, key, so.STEADY[key])
        assert so.finite(refs), key
        for a, b in zip(refs, plain):
            # the record's first entries are the first run's; the scalar started anew and the next entry is another one
            assert np.array_equal(a.rec[:, :so.FIRST], b.rec[:, :so.FIRST]) and np.all(a.rec[:, so.FIRST] != b.rec[:, so.FIRST])
            assert np.array_equal(a.f[so.FIRST], b.f[so.FIRST])
        steps, conv = so.wanted_stops([r.rec for r in refs], const, so.FIRST)
        print("17x16 <%s> %s, set again after %d steps, on %s, window %d, rel_tol %g, cap %d: stops %s converged %s" %
              (",".join(map(str, so.options_of(key[0], key[1]))), "buoyant" if key[2] else "passive", so.FIRST, const["on"],
               const["window"], const["rel_tol"], const["cap"], steps.tolist(), conv.tolist()))
        so.check_stops(steps, conv, const, so.FIRST)
        # with rel_tol 0.0 nobody stops: the run that is not ragged
        none = dict(const, rel_tol=0.0, cap=2 * const["window"])
        steps, conv = so.wanted_stops([r.rec for r in refs], none, so.FIRST)
        assert steps.tolist() == [so.FIRST + none["cap"]] * 3 and not conv.any()


def test_the_runs_across_the_ring_stay_finite(lbm, oracle_f64):
    nx, ny = so.STEADY_SHAPE
    T = so.RING_STEPS
    row, drive = so.RING_BUOYANT
    refs = once.reference_of(oracle_f64, "ring", so.make_case(lbm, nx, ny, row, T, drive), T)
    assert so.finite(refs) and all(np.all(np.isfinite(r.av)) and np.all(np.isfinite(r.fx)) for r in refs)
    assert all(np.all(r.rec[0] > 0.0) and np.all(r.rec[1:] != 0.0) and np.any(r.fx != 0.0) for r in refs)   # the gates' own conditions
    row, drive = so.RING_PLAIN
    case = so.make_case(lbm, nx, ny, row, T, drive, scalar=False)
    flows = [dm.reference_run(oracle_f64, m, T) for m in case.members]
    assert all(np.all(np.isfinite(fl.states[-1])) and np.all(np.isfinite(fl.totals)) for fl in flows)
    assert all(passes_the_flow_gates_own_conditions(fl) for fl in flows)
    # an entry that lands one slot off, or a flush that starts one entry off, is another value: neighbours differ all the way
    for series in [r.rec[v] for r in refs for v in range(3)] + [r.av for r in refs] + [np.array(fl.totals) for fl in flows]:
        assert series.shape == (T,) and np.all(series[1:] != series[:-1])

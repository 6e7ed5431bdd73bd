"""The body force (include/lbm.h, "Body force") on the numpy float64 restatement tests/_drive_ref.py, without a GPU.

tests/golden/drive.json holds what tests/golden/make_drive.py recorded with that restatement on three flows whose answers are
exact, all from rest at density 0.1 with accel = 0, and on a sweep to steady state.  Here
  1. the restatement's own lines, with F = 0 in place, give _les_ref.step's bits, and with drive None route to it;
  2. the fixture is this restatement's: the Poiseuille entry omega 1.0, Lambda 3/16 is computed again and equals the fixture;
  3. the inputs hold what the gates assume: nine fluid rows, a block that touches no wall, 296 fluid cells;
  4. the gates that tests/test_drive_gpu.py applies to the library's figures are applied to the fixture's: `poiseuille_gates`,
     `hydrostatic_gates`, `balance_gates`, `mirror_gate` and `sweep_gate` of tests/_drive_ref.py, which both modules import.

The gates are conditions the known answers set, not figures of the code under test:
  Poiseuille   with two relaxation times at Lambda = 3/16 a force-driven flow between bounce-back walls is the parabola with the
               walls half-way, to rounding, at any omega; at Lambda = 1/4 it slips by an amount that does not depend on omega;
               with BGK the wall moves with omega.  The wrong operators sit at 4e-3 and above, the right one at 1e-12: the cap of
               1e-9 separates them.  Density uniform, no cross flow.
  hydrostatic  a closed box under gravity is at rest, and its density falls by 3 F_y from row to row.
  balance      in steady state the walls and the block take up exactly the momentum the force feeds in, F_x x N_fluid per step:
               the new term and the existing force record held against each other."""
import sys

import numpy as np

import _drive_ref as ref
import _les_ref
import _open_ref
from _drive_ref import (GATED_OMEGAS, GOLDEN, balance_gates, fixture, hydrostatic_gates, mirror_gate, poiseuille_gates, poiseuille_table,
                        sweep_gate)


def make_drive():
    sys.path.insert(0, GOLDEN)
    try:
        import make_drive as module
    finally:
        sys.path.remove(GOLDEN)
    return module


# ---- 1. the restatement's own lines ----------------------------------------------------------------------------------------

def perturbed(ob, seed=5):
    rng = np.random.default_rng(seed)
    ny, nx = ob.shape
    return _open_ref.rest_state(ref.DENSITY, ny, nx) * (1.0 + 0.1 * (rng.random((9, ny, nx)) - 0.5))


def test_with_zero_force_in_place_the_lines_are_the_les_steps():
    ob = ref.balance_mask()
    f = perturbed(ob)
    blocked = ob != 0
    for magic in (None, ref.L316):
        for c in (None, 0.17):
            want = _les_ref.step(f, ob, 1.3, magic, c=c)
            g = _les_ref.gathered(f, ob)
            with np.errstate(all="ignore"):
                if c:
                    _, om, om_m = _les_ref.rates(g, 1.3, c, magic)
                else:
                    om, om_m = np.float64(1.3), (np.float64(ref._trt_ref.omega_minus(1.3, magic)) if magic else None)
                out, u = ref.collide(g, om, om_m, (0.0, 0.0))
            cells = np.stack([np.where(blocked, g[ref.OPP[k]], out[k]) for k in range(9)])
            assert np.array_equal(cells, want[0]) and np.array_equal(np.where(blocked, 0.0, u), want[1]), (magic, c)
            for off in (None, (0.0, 0.0), (-0.0, 0.0)):
                got = ref.step(f, ob, 1.3, magic, c=c, drive=off)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            on = ref.step(f, ob, 1.3, magic, c=c, drive=(1e-5, 0.0))
            assert not np.array_equal(on[0], want[0])
            assert np.array_equal(on[0][:, blocked], want[0][:, blocked])         # blocked cells take no force
    assert _les_ref.moments is ref._plain_moments                                # the hand-over of the momenta is undone


def test_a_step_adds_the_force_to_the_momentum_and_no_mass():
    """sum of c_k out[k] = sum of c_k g[k] + F and sum of out[k] = sum of g[k], per fluid cell, for both operators"""
    ob = np.zeros((7, 9), dtype=np.int32)
    f = perturbed(ob, 6)
    F = (3e-5, -2e-5)
    for magic in (None, ref.L316, ref.L14):
        for c in (None, 0.17):
            g = np.stack(_les_ref.gathered(f, ob))
            out = ref.step(f, ob, 1.3, magic, c=c, drive=F)[0]
            jx = lambda a: a[1] + a[5] + a[8] - a[3] - a[6] - a[7]
            jy = lambda a: a[2] + a[5] + a[6] - a[4] - a[7] - a[8]
            assert np.max(np.abs(out.sum(axis=0) - g.sum(axis=0))) <= 1e-16
            assert np.max(np.abs(jx(out) - jx(g) - F[0])) <= 1e-17 and np.max(np.abs(jy(out) - jy(g) - F[1])) <= 1e-17, (magic, c)
            # hence the physical velocity of the stored state: its momentum less half the force is the shifted momentum
            ux = ref.fields(out, ob, ref.DENSITY, F)[0]
            assert np.max(np.abs(ux - (jx(g) + 0.5 * F[0]) / g.sum(axis=0))) <= 1e-15


# ---- 2. the fixture is this restatement's ----------------------------------------------------------------------------------

def test_fixture_poiseuille_entry_is_the_restatements():
    fix = fixture()
    p = fix["poiseuille"]
    assert (p["nx"], p["ny"], tuple(p["force"]), p["steps"]) == (8, 11, (1e-6, 0.0), 20000) and len(p["entries"]) == 11
    got = make_drive().poiseuille_entry(1.0, ref.L316)
    want = poiseuille_table(fix)[(ref.L316, 1.0)]
    print("omega 1.0 Lambda 3/16: deviation %.17e (fixture %.17e)" % (got["deviation"], want[0]))
    assert (got["deviation"], got["spread"], got["uy"]) == want


# ---- 3. the inputs ---------------------------------------------------------------------------------------------------------

def test_inputs_hold_what_the_gates_assume():
    ob = ref.channel_mask(ref.POISEUILLE["nx"], ref.POISEUILLE["ny"])
    assert ob.shape == (11, 8) and np.all(ob[0] == 1) and np.all(ob[10] == 1) and not np.any(ob[1:10])   # nine fluid rows
    assert len(ref.parabola(11, 1.0, 1e-6, 0.1)) == 9
    box = ref.box_mask(ref.HYDROSTATIC["nx"], ref.HYDROSTATIC["ny"])
    assert box.shape == (12, 9) and np.all(box[0]) and np.all(box[-1]) and np.all(box[:, 0]) and np.all(box[:, -1])
    assert not np.any(box[1:-1, 1:-1])
    bal = ref.balance_mask()
    assert bal.shape == (15, 24) and np.all(bal[0] == 1) and np.all(bal[14] == 1)
    rows, cols = np.nonzero(bal[1:14])
    assert (rows.min() + 1, rows.max() + 1, cols.min(), cols.max()) == (5, 8, 8, 11) and rows.size == 16
    assert rows.min() + 1 >= 2 and rows.max() + 1 <= 12                          # the block touches no wall
    assert int(np.count_nonzero(bal == 0)) == ref.BALANCE["fluid"] == 296
    assert ref.BALANCE["force"][0] * 296 == 5.92e-4
    assert ref.SWEEP["forces"] == tuple(i * 1e-7 for i in range(1, 9))


# ---- 4. the gates on the fixture's values ----------------------------------------------------------------------------------

def test_poiseuille_gates_hold_on_the_fixture():
    table = poiseuille_table(fixture())
    print("\n".join(poiseuille_gates(table, table)))
    # the figures tell the operators apart: every run that is not Lambda 3/16 misses that gate's cap by six orders
    for (magic, w), (dev, _, _) in table.items():
        assert (dev <= 3e-12) == (magic == ref.L316 and w in GATED_OMEGAS), (magic, w, dev)
        if magic != ref.L316:
            assert dev >= 4e-3
    assert table[(ref.L316, 1.9)][0] < 1e-8                                      # on its way, not there


def test_hydrostatic_gates_hold_on_the_fixture():
    fix = fixture()["hydrostatic"]
    assert (fix["nx"], fix["ny"], tuple(fix["force"]), fix["steps"]) == (9, 12, (0.0, -1e-4), 30000)
    for e in fix["entries"]:
        print(hydrostatic_gates(e["umax"], e["step_error"], e["umax"]))
        assert e["umax"] <= 1e-15


def test_balance_gates_hold_on_the_fixture():
    fix = fixture()["balance"]
    assert (fix["nx"], fix["ny"], tuple(fix["force"]), fix["steps"], fix["fluid"]) == (24, 15, (2e-6, 0.0), 30000, 296)
    for e in fix["entries"]:
        print(balance_gates(e["rel"], e["lift"], max(e["rel"], e["lift"])))
        assert abs(e["fx"] - 5.92e-4) <= 1e-12 * 5.92e-4
    stored = max(fix["mirror_sum"], fix["entries"][0]["rel"])
    print(mirror_gate(fix["entries"][0]["fx"], fix["mirrored"]["fx"], stored))


def test_sweep_gate_holds_on_the_fixture():
    fix = fixture()["sweep"]
    assert all(e["converged"] for e in fix["entries"]) and [e["f_x"] for e in fix["entries"]] == list(ref.SWEEP["forces"])
    print(sweep_gate([e["av"] for e in fix["entries"]], [e["f_x"] for e in fix["entries"]], fix["spread"]))
    assert fix["spread"] <= 1e-6                                                  # linear in the force: the Stokes regime

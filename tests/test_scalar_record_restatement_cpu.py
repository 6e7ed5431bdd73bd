"""tests/_scalar_record_ref.py against its own gates and against tests/golden/scalar_steady.json (written by
tests/golden/make_scalar_steady.py), without a device.

  1. the gate of the restatement: gathered() + collided() are _scalar_ref.step bit for bit, on a mask with held and insulating
     walls and with the inlet and outlet statements; a blocked cell adds +0.0; the sums are the tree's (a hand-built case);
  2. the fixture: the first START entries of the three records of the first member of each sweep are recomputed, bit for bit
     (json carries a double's shortest repr, which reads back as the same double);
  3. the conditions on the chosen inputs of the steady runs, asserted on the fixture: two different stop counts among the members
     that converge, a member of the box at the cap unconverged, no stop at the first check point; and the rule applied to the
     fixture's last entries is consistent with the stops;
  4. each seeded defect misses the fixture; the cavity's figure lies where the fixture says, and its gate is twice its deviation."""
import numpy as np
import pytest

import _buoy_ref as bref
import _dp_matrix as dm
import _scalar_record_ref as rr
import _scalar_ref as sref


@pytest.fixture(scope="module")
def fix():
    return rr.fixture()


def test_the_gather_is_the_scalar_steps_own():
    nx, ny = 17, 16
    ob, _ = dm.matrix_mask(nx, ny, 1)
    rng = np.random.default_rng(5)
    g = sref.init(0.5 + rng.random((ny, nx)))
    g = g * (1.0 + 0.1 * (rng.random(g.shape) - 0.5))
    wall = 2.0 * rng.random((ny, nx))
    wall[rng.random((ny, nx)) < 0.5] = np.nan
    u_x, u_y = 0.1 * (rng.random((ny, nx)) - 0.5), 0.1 * (rng.random((ny, nx)) - 0.5)
    for c_in in (None, 0.5 + rng.random(ny)):
        rr.check_gather(g, ob, u_x, u_y, sref.omega_s(0.1), wall, c_in)
        c, q_x, q_y = rr.cells(g, ob, u_x, u_y, wall, c_in)
        for v in (c, q_x, q_y):
            assert dm.plus_zero(v[ob != 0]) and np.all(np.isfinite(v))
        h = rr.gathered(g, ob, wall, c_in)
        fluid = ob == 0
        assert np.array_equal(c[fluid], ((((h[0] + h[1]) + h[2]) + h[3]) + h[4])[fluid])
        assert np.array_equal(q_x[fluid], (c * u_x)[fluid]) and np.array_equal(q_y[fluid], (c * u_y)[fluid])
    # the inlet and outlet statements enter c
    assert not np.array_equal(rr.cells(g, ob, u_x, u_y, wall, None)[0], rr.cells(g, ob, u_x, u_y, wall, np.ones(ny))[0])


def test_the_sums_are_the_trees():
    """17 cells a row: nine lanes, the ninth without its second cell, in a second segment of which seven lanes are idle.  Values
    that a flat sum rounds otherwise."""
    e = 2.0 ** -53
    v = np.zeros((3, 17))
    v[1] = [1.0] + [e] * 16
    p = [1.0 + e] + [e + e] * 7                                                # the lanes' pair sums: the first loses its e
    assert p[0] == 1.0
    first = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))
    assert first == 1.0 + 14.0 * e
    want = first + (e + 0.0)                                                   # the second segment: one lane, no second cell
    assert want == 1.0 + 16.0 * e                                              # a tie, to even
    got = rr.entry((v, v, v))
    assert got[0] == got[1] == got[2] == want
    left_to_right = 0.0
    for x in v.reshape(-1):
        left_to_right += x
    assert left_to_right == 1.0 != want                                        # the order decides
    assert rr.entry((v,), "flat")[0] == np.sum(v)


@pytest.mark.parametrize("name", ["box", "channel"])
def test_the_fixture_holds_the_restatements_records(fix, name):
    entry = fix[name]
    sweep = rr.BOX if name == "box" else rr.CHANNEL
    first = entry["members"][0]
    assert entry["start"] == rr.START and [entry[k] for k in ("window", "rel_tol", "cap", "which")] == [sweep[k] for k in ("window", "rel_tol", "cap", "which")]
    got = rr.box_records(first, rr.START) if name == "box" else rr.channel_records(first, rr.START)
    for i, n in enumerate(rr.NAMES):
        assert np.array_equal(got[i], np.array(entry["first"][n])), (name, n)
    assert np.any(got[0] != got[0][0]) and np.any(got[1] != 0.0)


def test_the_conditions_on_the_chosen_inputs(fix):
    box, channel = fix["box"], fix["channel"]
    assert box["members"] == list(rr.BOX["Ras"]) == [1e3, 3e3, 1e4] and channel["members"] == list(rr.CHANNEL["Ds"])
    assert (rr.BOX["n"], rr.BOX["H"], rr.BOX["Pr"], rr.BOX["omega"], rr.BOX["c_ref"]) == (12, 10, 0.71, 1.5, 0.5)
    assert (rr.BOX["window"], rr.BOX["rel_tol"], rr.BOX["cap"], rr.BOX["which"]) == (16, 1e-4, 512, "flux_x")
    rr.check_stops(box, rr.BOX, members_at_cap=1)
    rr.check_stops(channel, rr.CHANNEL, members_at_cap=0)
    assert len(set(channel["stops"])) >= 2 and rr.CHANNEL["which"] == "content"
    for entry, sweep in ((box, rr.BOX), (channel, rr.CHANNEL)):
        assert all(s % sweep["window"] == 0 and s <= sweep["cap"] for s in entry["stops"])
        assert all(np.isfinite(v) for last in entry["last"] for v in last)


@pytest.mark.parametrize("defect", rr.DEFECTS)
def test_a_seeded_defect_misses_the_fixture(fix, defect):
    entry = fix["box"]
    got = rr.box_records(entry["members"][0], rr.START, defect)
    hit = {"written": ("content", "flux_x"), "no_half": ("flux_y",), "blocked": ("content",), "flat": ("content",)}[defect]
    for n in hit:
        assert not np.array_equal(got[rr.NAMES.index(n)], np.array(entry["first"][n])), (defect, n)


def test_the_cavity(fix):
    c = fix["cavity"]
    C = bref.CAVITY
    assert (c["Ra"], c["steps"], c["theory"]) == (C["Ra"], C["steps"], C["theory"]) and C["theory"] == 1.118
    cs = bref.cavity()
    assert bref.close(rr.nusselt_convective(c["flux_x"], cs.s.ob, C["H"], cs.s.D), c["nusselt"])
    assert c["deviation"] == abs(c["nusselt"] / c["theory"] - 1.0) and 0.0 < c["deviation"] < 0.01
    # the volume average and the wall's mean gradient (tests/golden/buoy.json's figure) are one heat flux in a steady cavity
    assert abs(c["nusselt"] - c["wall_nusselt"]) < 1e-3 and bref.close(c["wall_nusselt"], bref.fixture()["cavity"]["nusselt"])

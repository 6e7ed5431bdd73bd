"""The two flows with a known answer (tests/_flows_ref.py) on the numpy float64 restatement, without a GPU.

tests/golden/flows.json holds what tests/golden/make_flows.py recorded with tests/_open_ref.py on tests/_trt_ref.py.  Here
  1. the fixture is this restatement's: the channel entry omega 1.0, Lambda 3/16 and the first 2 000 steps of the D = 10
     cylinder are computed again and equal the fixture to 1e-12 relative;
  2. the geometry holds what _flows_ref promises;
  3. the gates that tests/test_flows_gpu.py applies to the library's figures are applied to the fixture's: `channel_gates`,
     `cylinder_gates`, `mirror_gates` and `finer_gates` of tests/_flows_ref.py, which both modules import.

The gates are conditions that the answer known from outside sets, not figures of the code under test:
  channel   with two relaxation times at a fixed magic parameter Lambda the place of a bounce-back wall does not depend on
            omega; at Lambda = 3/16 it is half-way for a parabolic profile, so the computed profile is poiseuille()'s; at
            Lambda = 1/4 and any omega it is where BGK has it at omega = 1 (there tau - 1/2 = 1/2 and Lambda = (tau - 1/2)^2
            = 1/4); with BGK it moves with omega.
  cylinder  Schaefer-Turek 2D-1: C_d 5.57 - 5.59, C_l 0.0104 - 0.0110.  A disc of ten cells is a staircase: 7 % of 5.58 and
            25 % of 0.0107 are what that resolution is given; twenty cells must come closer, within 5 %."""
import os
import sys

import numpy as np

import _flows_ref as flows
import _open_ref
from _flows_ref import BGK_OMEGAS, L316, channel_gates, channel_table, cylinder_gates, finer_gates, fixture, mirror_gates

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53


def make_flows():
    sys.path.insert(0, GOLDEN)
    try:
        import make_flows as module
    finally:
        sys.path.remove(GOLDEN)
    return module


# ---- 1. the fixture is this restatement's --------------------------------------------------------------------------------

def close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


def test_fixture_channel_entry_is_the_restatements():
    fix = fixture()
    assert (fix["channel"]["nx"], fix["channel"]["ny"], fix["channel"]["u_max"], fix["channel"]["steps"]) == (
        flows.CH_NX, flows.CH_NY, flows.CH_U, flows.CH_STEPS)
    assert len(fix["channel"]["entries"]) == 12
    got = make_flows().channel_entry(1.0, L316)
    spread, shape = channel_table(fix)[(L316, 1.0)]
    print("omega 1.0 Lambda 3/16: shape %.17e (fixture %.17e) spread %.17e (fixture %.17e)" % (got["shape"], shape, got["spread"], spread))
    assert close(got["shape"], shape) and close(got["spread"], spread)


def test_fixture_cylinder_start_is_the_restatements():
    fix = fixture()["cylinder"]["10"]
    steps = 2000
    got = make_flows().cylinder_run(10, steps=steps)
    n = steps // fix["every"] + 1
    assert fix["every"] == got["every"] == 250 and len(got["fx"]) == n and got["links"] == fix["links"]
    # from rest nothing pushes the disc: the first entry is rounding of 94 equal pairs, at most the gate between two orders
    assert abs(fix["fx"][0]) <= 8 * fix["links"] * U * fix["mag"][0] and abs(fix["fy"][0]) <= 8 * fix["links"] * U * fix["mag"][0]
    assert got["fx"][0] == fix["fx"][0] and got["fy"][0] == fix["fy"][0]
    for i in range(1, n):
        for key in ("fx", "fy", "mag"):
            assert close(got[key][i], fix[key][i]), (key, i, got[key][i], fix[key][i])
    assert abs(fix["fx"][n - 1]) > 1e-3                                   # ... and then something does


# ---- 2. the geometry -----------------------------------------------------------------------------------------------------

def test_geometry_holds_what_it_promises():
    for D, links, shape in ((10, 94, (43, 220)), (20, 190, (84, 440))):
        c = flows.cylinder_channel(D)
        ob, body, ny, nx = c["ob"], c["body"], c["ny"], c["nx"]
        assert ob.shape == body.shape == shape == (ny, nx) and c["u_in"].shape == (ny,)
        assert _open_ref.force(flows.rest(c), ob, body)[2] == links
        # walls on rows 0 and ny - 1 and nothing else but the disc; the disc touches neither wall nor the open columns
        assert np.all(ob[0] == 1) and np.all(ob[ny - 1] == 1) and np.array_equal(ob[1:ny - 1], body[1:ny - 1])
        rows, cols = np.nonzero(body)
        assert rows.min() >= 2 and rows.max() <= ny - 3 and cols.min() >= 2 and cols.max() <= nx - 3
        assert not np.any(body & (ob == 0))
        # the wall planes lie at y = 1/2 and y = ny - 3/2, the inlet plane at x = 0: 4.1 D between the walls, the centre 2 D
        # from the lower one, 2.1 D from the upper one and 2 D behind the inlet, the channel 22 D long
        lower, upper = 0.5, ny - 1.5
        assert abs((upper - lower) - 4.1 * D) < 1e-12 and c["cy"] - lower == 2.0 * D and abs((upper - c["cy"]) - 2.1 * D) < 1e-12
        assert c["cx"] == 2.0 * D and nx == 22 * D
        # a disc: symmetric about its centre in x and y, pi D^2 / 4 cells within a staircase's margin; the centre lies on a
        # column and between two rows, so it is D rows high and D - 1 columns wide
        assert np.array_equal(body[:, :int(2 * c["cx"]) + 1], body[:, int(2 * c["cx"])::-1])
        assert np.array_equal(body[:int(2 * c["cy"]) + 1], body[int(2 * c["cy"])::-1])
        assert cols.max() - cols.min() + 1 == D - 1 and rows.max() - rows.min() + 1 == D
        assert abs(np.count_nonzero(body) / (np.pi * D * D / 4.0) - 1.0) < 0.05
        # the inlet: the parabola between the wall planes with mean 2/3 of its maximum, Re = U_mean D / nu = 20
        assert c["u_in"][0] == 0.0 and c["u_in"][ny - 1] == 0.0
        assert abs(c["u_in"][1:ny - 1].mean() / c["u_mean"] - 1.0) < 1e-3 and abs(c["u_in"].max() / (1.5 * c["u_mean"]) - 1.0) < 2e-3
        nu = (1.0 / c["omega"] - 0.5) / 3.0
        assert abs(c["u_mean"] * D / nu - 20.0) < 1e-12 and c["magic"] == L316
        # the mirror image: the same case upside down, and twice is the case itself
        m = flows.mirrored(c)
        assert np.array_equal(m["ob"], ob[::-1]) and np.array_equal(m["body"], body[::-1]) and np.array_equal(m["u_in"], c["u_in"][::-1])
        assert abs((m["cy"] - lower) - 2.1 * D) < 1e-12 and upper - m["cy"] == 2.0 * D
        assert not np.array_equal(m["body"], body)
        mm = flows.mirrored(m)
        assert np.array_equal(mm["ob"], ob) and np.array_equal(mm["body"], body) and np.array_equal(mm["u_in"], c["u_in"])
        assert _open_ref.force(flows.rest(m), m["ob"], m["body"])[2] == links
    cd, cl = flows.coefficients(0.1 * 0.04 * 0.04 * 10 / 2.0, -0.1 * 0.04 * 0.04 * 10, 10)
    assert abs(cd - 1.0) < 1e-15 and abs(cl + 2.0) < 1e-15
    assert np.count_nonzero(flows.channel_mask()) == 2 * flows.CH_NX


# ---- 3. the gates on the fixture's values --------------------------------------------------------------------------------

def test_channel_gates_hold_on_the_fixture():
    table = channel_table(fixture())
    assert np.isnan(table[(None, 1.9)][1])                                # BGK diverges there: not a member of any gate
    fig = {k: v for k, v in table.items() if k != (None, 1.9)}
    assert len(fig) == 11
    print("\n".join(channel_gates(fig)))
    # the gates tell the collisions apart: BGK's three figures miss the fixed-Lambda gate
    bgk = [fig[(None, w)][1] for w in BGK_OMEGAS]
    assert max(bgk) / min(bgk) > 1.1 and min(bgk) > 1e-4


def test_cylinder_gates_hold_on_the_fixture():
    fix = fixture()["cylinder"]
    d10, d20 = fix["10"], fix["20"]
    assert d10["steps"] == 40000 and d10["tail"]["first"] == 34000 and d10["links"] == 94 and d20["links"] == 190
    print(cylinder_gates(d10["tail"]))
    print(mirror_gates(d10["tail"], d10["mirrored"]["tail"], d10["mirrored"]))
    assert max(d10["mirrored"]["d_cd"], d10["mirrored"]["d_cl"]) <= 1e-6 * d10["tail"]["cd_mean"]
    # the sampled forces are the record the tail was taken from
    cd, _ = flows.coefficients(d10["fx"], d10["fy"], 10)
    at = np.arange(len(cd)) * d10["every"]
    inside = cd[(at >= 34000) & (at < 40000)]
    assert inside.size == 24 and d10["tail"]["cd_min"] <= inside.min() and inside.max() <= d10["tail"]["cd_max"]
    # D = 20 ran until its own swing met the same 0.2 %
    t20 = d20["tail"]
    assert d20["settled"] and t20["first"] == d20["steps"] - 6000
    assert (t20["cd_max"] - t20["cd_min"]) <= 2e-3 * t20["cd_mean"]
    print(finer_gates(t20, d10["tail"]))

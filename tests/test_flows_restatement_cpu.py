"""The two flows with a known answer (tests/_flows_ref.py) on the numpy float64 restatement, without a GPU.

tests/golden/flows.json holds what tests/golden/make_flows.py recorded with tests/_open_ref.py on tests/_trt_ref.py.  Here
  1. the fixture is this restatement's: the channel entry omega 1.0, Lambda 3/16 and the first 2 000 steps of the D = 10
     cylinder are computed again and equal the fixture to 1e-12 relative;
  2. the geometry holds what _flows_ref promises;
  3. the gates that tests/test_flows_gpu.py applies to the library's figures are applied to the fixture's: `channel_gates`,
     `cylinder_gates`, `mirror_gates` and `finer_gates` below are the ones it imports.

The gates are conditions that the answer known from outside sets, not figures of the code under test:
  channel   with two relaxation times at a fixed magic parameter Lambda the place of a bounce-back wall does not depend on
            omega; at Lambda = 3/16 it is half-way for a parabolic profile, so the computed profile is poiseuille()'s; at
            Lambda = 1/4 and any omega it is where BGK has it at omega = 1 (there tau - 1/2 = 1/2 and Lambda = (tau - 1/2)^2
            = 1/4); with BGK it moves with omega.
  cylinder  Schaefer-Turek 2D-1: C_d 5.57 - 5.59, C_l 0.0104 - 0.0110.  A disc of ten cells is a staircase: 7 % of 5.58 and
            25 % of 0.0107 are what that resolution is given; twenty cells must come closer, within 5 %."""
import json
import os
import sys

import numpy as np

import _flows_ref as flows
import _open_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
L316, L14 = 3.0 / 16.0, 0.25
BGK_OMEGAS = (0.6, 1.0, 1.7)


def fixture():
    with open(os.path.join(GOLDEN, "flows.json")) as f:
        return json.load(f)


def channel_table(fix):
    """{(magic or None, omega): (spread, shape)} of the fixture; the diverged BGK entry holds NaNs"""
    nan = float("nan")
    return {(e["magic"], e["omega"]): (nan if e["spread"] is None else e["spread"], nan if e["shape"] is None else e["shape"])
            for e in fix["channel"]["entries"]}


def make_flows():
    sys.path.insert(0, GOLDEN)
    try:
        import make_flows as module
    finally:
        sys.path.remove(GOLDEN)
    return module


# ---- the gates -----------------------------------------------------------------------------------------------------------

def channel_gates(fig):
    """fig {(magic or None, omega): (spread, shape)} with Lambda = 3/16 and 1/4 at the four omegas and BGK at 0.6, 1.0, 1.7"""
    lines = []
    for magic in (L316, L14):
        shapes = [fig[(magic, w)][1] for w in flows.CH_OMEGAS]
        assert all(s > 0.0 for s in shapes)
        lines.append("Lambda %.4f: shape %s, max / min %.4f (gate 1.1)" % (magic, " ".join("%.4e" % s for s in shapes),
                                                                          max(shapes) / min(shapes)))
        assert max(shapes) / min(shapes) <= 1.1, (magic, shapes)                 # the wall does not move with omega
    bgk = [fig[(None, w)][1] for w in BGK_OMEGAS]
    lines.append("BGK: shape %s, max / min %.2f (gate >= 10)" % (" ".join("%.4e" % s for s in bgk), max(bgk) / min(bgk)))
    assert min(bgk) > 0.0 and max(bgk) / min(bgk) >= 10.0, bgk                   # the figure is not blind: with BGK it moves
    for w in flows.CH_OMEGAS:
        s316, s14 = fig[(L316, w)][1], fig[(L14, w)][1]
        lines.append("omega %.1f: shape at 3/16 %.4e (gate 1e-4), at 1/4 %.4e, ratio %.1f (gate >= 100), 1/4 against BGK at 1: %.2e "
                     "(gate 1e-3)" % (w, s316, s14, s14 / s316, abs(s14 - fig[(None, 1.0)][1]) / fig[(None, 1.0)][1]))
        assert s316 <= 1e-4, (w, s316)                                           # half-way: the parabola itself
        assert s14 >= 100.0 * s316, (w, s14, s316)
        assert abs(s14 - fig[(None, 1.0)][1]) <= 1e-3 * fig[(None, 1.0)][1], (w, s14, fig[(None, 1.0)][1])
    for (magic, w), (spread, _) in sorted(fig.items(), key=str):
        if w <= 1.7:
            lines.append("%s omega %.1f: spread %.2e (gate 1e-9)" % ("BGK" if magic is None else "Lambda %.4f" % magic, w, spread))
            assert abs(spread) <= 1e-9, (magic, w, spread)                       # one flux through every column: settled
    return lines


def tail_of(fx, fy, D, tail=6000):
    """the figures of a record's last `tail` entries, as the fixture's "tail" holds them"""
    cd, cl = flows.coefficients(fx[-tail:], fy[-tail:], D)
    assert cd.shape == (tail,)
    return {"cd_mean": float(cd.mean()), "cd_min": float(cd.min()), "cd_max": float(cd.max()), "cl_mean": float(cl.mean())}


def cylinder_gates(t):
    """t: the figures of the last 6 000 steps at D = 10"""
    cd, cl, swing = t["cd_mean"], t["cl_mean"], (t["cd_max"] - t["cd_min"]) / t["cd_mean"]
    line = ("D 10: C_d %.4f (%+.2f %% of 5.58, gate 7 %%), max - min %.3f %% (gate 0.2 %%), C_l %.5f (%+.1f %% of 0.0107, gate 25 %%)"
            % (cd, 100.0 * (cd / flows.CD_PUBLISHED - 1.0), 100.0 * swing, cl, 100.0 * (cl / flows.CL_PUBLISHED - 1.0)))
    assert abs(cd - flows.CD_PUBLISHED) <= 0.07 * flows.CD_PUBLISHED, line
    assert 0.0 <= swing <= 2e-3, line
    assert cl > 0.0 and abs(cl - flows.CL_PUBLISHED) <= 0.25 * flows.CL_PUBLISHED, line   # the disc is nearer the lower wall
    return line


def mirror_gates(t0, t1, stored):
    """the mirrored member: the same C_d, the opposite C_l, each within 100 x what the restatement's two runs differ by and
    1e-6 of C_d at the most (a flipped sign or a wrong member's record is 1e-2)"""
    d_cd, d_cl = abs(t0["cd_mean"] - t1["cd_mean"]), abs(t0["cl_mean"] + t1["cl_mean"])
    cap = 1e-6 * t0["cd_mean"]
    g_cd, g_cl = min(100.0 * stored["d_cd"], cap), min(100.0 * stored["d_cl"], cap)
    line = "mirrored member: |C_d - C_d'| %.2e (gate %.2e), |C_l + C_l'| %.2e (gate %.2e)" % (d_cd, g_cd, d_cl, g_cl)
    assert d_cd <= g_cd and d_cl <= g_cl, line
    return line


def finer_gates(t20, t10):
    """D = 20 against D = 10: nearer the published drag, and within 5 % of it"""
    e20, e10 = abs(t20["cd_mean"] - flows.CD_PUBLISHED), abs(t10["cd_mean"] - flows.CD_PUBLISHED)
    line = "D 20: C_d %.4f (%+.2f %% of 5.58, gate 5 %% and below D 10's %+.2f %%), C_l %.5f" % (
        t20["cd_mean"], 100.0 * (t20["cd_mean"] / flows.CD_PUBLISHED - 1.0), 100.0 * (t10["cd_mean"] / flows.CD_PUBLISHED - 1.0),
        t20["cl_mean"])
    assert e20 < e10 and e20 <= 0.05 * flows.CD_PUBLISHED, line
    return line


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

"""The passive scalar (include/lbm.h, "Scalar transport"; lbm_dscalar_*) on the GPU: dp_scalar_step and its helper kernels against
tests/_scalar_ref.py, the flow beside it against the flow without it, and the flows with known answers end to end.

The cases, masks, inputs and drivers of the flow are tests/_dp_matrix.py's (make_case with `scalar`; open_context and open_ensemble
set the scalar last, behind the upload): a case has three members, each with its own obstacle map (walls, a block, lips and isolated
cells), omega and state, and here its own diffusivity (0.01, 1/6, 0.4), first field, c_wall (NaN and finite values mixed) and inlet
values.

  1. bits: 33x19 and 17x16 (odd nx, a lane without its second cell, a last segment that is not full), the flow with all options
     off, each of FORCE, TRT, OPEN, WALL, LES and DRIVE alone and all on, LBMDouble at "multistep" 0 and 8 and EnsembleDouble, runs
     of 1, 1, 1 and 7 steps: scalar_cells() and scalar_field() equal the restatement by np.array_equal after each run; a member
     equals its context; 6x5 in the tile forms; a run of 10 against 3 + 7; download -> upload -> run against a plain run;
  2. the flow does not notice: in each of those runs cells, av_vels, the force record and force() are bit-equal to the same run
     without a scalar; off is off (set_scalar(D), then set_scalar(None), equals a handle that never had it); on is on (after one
     step of a non-uniform c0 the field differs from c0 - this, like every test here that calls set_scalar, fails without the
     feature);
  3. - 7. conservation, diffusion, held walls, open ends and Taylor-Aris dispersion: the runs of _scalar_ref.RUNS on the device, the
     issue's gates on the device's figures (_scalar_ref.gates), and for Taylor-Aris the figures against tests/golden/scalar.json to
     1e-9 relative;
  8. errors and what keeps the setting.

The comparisons with numpy rest on the device's double-precision division being correctly rounded, as those of
tests/test_drive_gpu.py do: the velocity a scalar step reads is two divisions per cell.  Bits are asked for, and bits hold: on an
MI355X the populations and the field of all 48 matrix cases, of the 6x5 cases and of the identities equal the restatement by
np.array_equal after every run, and no looser bound is in this module.  The flows give the fixture's figures to the digit:
conservation drift 1.632e-14; diffusion rate over 2 D k^2 +0.936 % / +0.374 % / +0.424 % at D = 0.02 / 0.05 / 0.2; held walls
1.650e-13 / 3.431e-14 / 1.699e-14 / 7.327e-15 from the straight profile at D = 0.02 / 0.1 / 1/6 / 0.3; open ends max |C - 1| 1.443e-13
/ 1.932e-13 at D = 0.01 / 0.05; Taylor-Aris D_eff 0.98481 of D (1 + Pe^2 / 210), the centre at 1.00195 of 0.05, the flow 4.031e-14
off the parabola at the release.  71 cases, 3.7 s; the longest is held walls at D = 0.02 (102 400 steps, 0.8 s).  What the scalar
costs is in profiles/scalar_throughput.txt (tools/scalar_ab.py): 4.11 x on the 64 x 128x128 ensemble, dp_scalar_step alone at 0.90
of the copy rate on one 8192^2 context."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import _dp_matrix as dm
import _scalar_ref as sref
from _dp_matrix import DS, set_scalars
from _force_ref import accelerated

pytestmark = pytest.mark.gpu

LBM_ERR_ARG, LBM_ERR_STATE = 1, 3
SHAPES = dm.SHAPES
RUNS = dm.RUNS
#          force trt open wall les drive
OPTIONS = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), (0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 0), (0, 0, 0, 0, 1, 0),
           (0, 0, 0, 0, 0, 1), (1, 1, 1, 1, 1, 1)]
FAMILIES = [0, 8, "ensemble"]
_refs, _runs = {}, {}


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


@pytest.fixture(scope="module")
def fix():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scalar.json")) as f:
        return json.load(f)


def make_case(lbm, nx, ny, opts, steps=sum(RUNS)):
    """the matrix case with a scalar per member (dm.member_scalar)"""
    force, trt, opened, wall, les, drive = opts
    return dm.make_case(lbm, nx, ny, 3, steps, force, trt, opened, wall="on" if wall else None, les="on" if les else None,
                        drive="on" if drive else None, scalar=True)


def narrow(lbm):
    return dm.narrow_case(lbm, drive="on", scalar=True)


def reference_of(oracle_f64, key, case, steps):
    """per member: the flow's reference states (dm.reference_run) and the scalar's populations after every step"""
    if key in _refs:
        return _refs[key]
    out = []
    for m in case.members:
        flow = dm.reference_run(oracle_f64, m, steps)
        drive = m.drive if isinstance(m.drive, tuple) else None
        g = [sref.init(m.scalar.c0)]
        for n in range(steps):
            f = flow.states[n]
            if m.open is None:
                fa = accelerated(oracle_f64, m.p, m.ob, f)
                assert np.array_equal(fa, sref.accelerate(f, m.ob, m.p.density, m.p.accel))
            else:
                fa = f
            u_x, u_y = sref.velocity(fa, m.ob, drive)
            g.append(sref.step(g[-1], m.ob, u_x, u_y, sref.omega_s(m.scalar.D), m.scalar.wall,
                               m.scalar.inlet if m.open is not None else None))
        out.append(SimpleNamespace(flow=flow, g=g))
    _refs[key] = out
    return out


def drive(lbm, family, case, runs, scalar=True, between=None):
    """per member: the flow's state after each run, av_vels, the force record, force() before each run, and with a scalar
    (set behind the upload by dm.open_context / dm.open_ensemble) its populations and field after each run.  between(handle):
    called behind every run but the last"""
    results = []

    def loop(handle):
        states, now, g, c = [], [], [], []
        for i, r in enumerate(runs):
            now.append(handle.force())
            handle.run(r)
            states.append(handle.download(av_vels=False)[0])
            if scalar:
                g.append(handle.scalar_cells())
                c.append(handle.scalar_field())
                if between is not None and i + 1 < len(runs):
                    between(handle)
        av = handle.download(cells=False)[1]
        return states, now, g, c, av, (handle.force_record() if case.force else None)

    if family == "ensemble":
        with dm.open_ensemble(lbm, case, scalar=scalar) as ens:
            states, now, g, c, av, rec = loop(ens)
        for k in range(case.n):
            results.append(SimpleNamespace(states=[s[k] for s in states], av=av[k], fx=None if rec is None else rec[0][k],
                                           fy=None if rec is None else rec[1][k], now=[(float(a[k]), float(b[k])) for a, b in now],
                                           g=[x[k] for x in g], c=[x[k] for x in c]))
    else:
        for m in case.members:
            with dm.open_context(lbm, case, m, family, scalar=scalar) as sim:
                states, now, g, c, av, rec = loop(sim)
            results.append(SimpleNamespace(states=states, av=av, fx=None if rec is None else rec[0], fy=None if rec is None else rec[1],
                                           now=now, g=g, c=c))
    return results


def run_of(lbm, key, family, case, runs, scalar=True):
    k = (family, scalar) + key
    if k not in _runs:
        _runs[k] = drive(lbm, family, case, runs, scalar)
    return _runs[k]


def assert_scalar_equals_the_reference(case, refs, got, runs, what):
    for k, (m, ref, res) in enumerate(zip(case.members, refs, got)):
        done = 0
        for i, r in enumerate(runs):
            done += r
            differs = int(np.count_nonzero(res.g[i] != ref.g[done]))
            assert np.array_equal(res.g[i], ref.g[done]), (what, k, done, differs)
            assert np.array_equal(res.c[i], sref.field(ref.g[done], m.ob)), (what, k, done)
            assert np.array_equal(res.states[i], ref.flow.states[done]), (what, k, done)
        assert np.all(np.isfinite(res.g[-1]))


def assert_same_flow(a, b, what):
    """two results of one case, member by member: cells, av_vels, force() and the force record, bit for bit"""
    for k, (x, y) in enumerate(zip(a, b)):
        assert all(np.array_equal(s, t) for s, t in zip(x.states, y.states)), (what, k)
        assert np.array_equal(x.av, y.av) and x.now == y.now, (what, k)
        assert (x.fx is None) == (y.fx is None)
        if x.fx is not None:
            assert np.array_equal(x.fx, y.fx) and np.array_equal(x.fy, y.fy), (what, k)


# ---- 1. bits, and 2. the flow does not notice ---------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("opts", OPTIONS)
def test_scalar_equals_the_restatement_and_the_flow_does_not_notice(lbm, oracle_f64, opts, family, nx, ny):
    what = "%s<%s> %dx%d" % (family, ",".join(map(str, opts)), nx, ny)
    case = make_case(lbm, nx, ny, opts)
    refs = reference_of(oracle_f64, (nx, ny) + opts[1:], case, sum(RUNS))
    got = run_of(lbm, (nx, ny) + opts, family, case, RUNS)
    assert_scalar_equals_the_reference(case, refs, got, RUNS, what)
    assert len({r.g[-1].tobytes() for r in got}) == case.n                          # the members carry different scalars
    plain = run_of(lbm, (nx, ny) + opts, family, make_case(lbm, nx, ny, opts), RUNS, scalar=False)
    assert_same_flow(got, plain, what)
    if family == "ensemble":
        for other in (0, 8):                                                        # a member is its context, bit for bit
            ctx = run_of(lbm, (nx, ny) + opts, other, case, RUNS)
            for k, (a, b) in enumerate(zip(got, ctx)):
                assert all(np.array_equal(x, y) for x, y in zip(a.g, b.g)), (what, other, k)
                assert all(np.array_equal(x, y) for x, y in zip(a.c, b.c)), (what, other, k)


@pytest.mark.parametrize("family", [8, "ensemble"])
def test_region_wider_than_the_grid(lbm, oracle_f64, family):
    runs = [1] * 6
    case = narrow(lbm)
    assert (case.nx, case.ny) == (6, 5)
    refs = reference_of(oracle_f64, ("narrow",), case, len(runs))
    got = run_of(lbm, ("narrow",), family, case, runs)
    assert_scalar_equals_the_reference(case, refs, got, runs, "%s 6x5" % family)
    assert_same_flow(got, run_of(lbm, ("narrow",), family, narrow(lbm), runs, scalar=False), "%s 6x5" % family)


@pytest.mark.parametrize("family", FAMILIES)
def test_one_run_of_ten_against_three_and_seven(lbm, family):
    nx, ny = SHAPES[0]
    opts = (1, 1, 0, 1, 0, 1)
    whole = run_of(lbm, ("ten", 10), family, make_case(lbm, nx, ny, opts, 10), [10])
    split = run_of(lbm, ("ten", 3, 7), family, make_case(lbm, nx, ny, opts, 10), [3, 7])
    for k, (a, b) in enumerate(zip(whole, split)):
        assert np.array_equal(a.g[-1], b.g[-1]) and np.array_equal(a.c[-1], b.c[-1]), (family, k)
        assert np.array_equal(a.states[-1], b.states[-1]) and np.array_equal(a.av, b.av), (family, k)


@pytest.mark.parametrize("family", FAMILIES)
def test_download_upload_run_is_a_plain_run(lbm, family):
    nx, ny = SHAPES[1]
    opts = (0, 1, 1, 0, 0, 0)
    plain = run_of(lbm, ("round",), family, make_case(lbm, nx, ny, opts), RUNS)
    seen = []

    def round_trip(handle):
        g = handle.scalar_cells()
        handle.upload_scalar(np.zeros_like(g))
        assert not np.any(handle.scalar_cells()) and not np.any(handle.scalar_field())
        handle.upload_scalar(g)
        seen.append(g)

    again = drive(lbm, family, make_case(lbm, nx, ny, opts), RUNS, between=round_trip)
    assert seen
    for k, (a, b) in enumerate(zip(again, plain)):
        assert all(np.array_equal(x, y) for x, y in zip(a.g, b.g)), (family, k)


@pytest.mark.parametrize("family", FAMILIES)
def test_off_is_off_and_on_is_on(lbm, family):
    nx, ny = SHAPES[0]
    opts = (1, 0, 0, 0, 0, 0)
    case = make_case(lbm, nx, ny, opts)
    never = run_of(lbm, (nx, ny) + opts, family, case, RUNS, scalar=False)
    handles = ([dm.open_ensemble(lbm, case)] if family == "ensemble" else [dm.open_context(lbm, case, m, family) for m in case.members])
    for i, h in enumerate(handles):
        members = case.members if family == "ensemble" else [case.members[i]]
        with h:
            assert h.scalar() is None
            set_scalars(h, members)
            h.run(1)
            c = h.scalar_field().reshape(len(members), ny, nx)
            for m, got in zip(members, c):                                          # on is on: one step has moved the field
                fluid = m.ob == 0
                assert not np.array_equal(got[fluid], m.scalar.c0[fluid])
            h.set_scalar(None)
            assert h.scalar() is None
            h.upload(None if members[0].cells0 is None else
                     (np.stack([m.cells0 for m in members]) if family == "ensemble" else members[0].cells0))
            for r in RUNS:
                h.run(r)
            cells, av = h.download()
            for j, m in enumerate(members):
                k = j if family == "ensemble" else i
                assert np.array_equal(cells[j] if family == "ensemble" else cells, never[k].states[-1]), (family, k)
                assert np.array_equal(av[j] if family == "ensemble" else av, never[k].av), (family, k)


# ---- 3. - 7. the flows with known answers -------------------------------------------------------------------------------------

def device_run(lbm, kind, D):
    """the run _scalar_ref.case(kind, D) on an LBMDouble: (case, {step: field} at its samples, the context's last final_state)"""
    cs = sref.case(kind, D)
    ny, nx = cs.ob.shape
    fl = cs.fl
    p = lbm.make_dparams(nx, ny, cs.spin_up + cs.steps, density=fl.density, accel=fl.accel, omega=fl.omega, obstacles=cs.ob)
    with lbm.LBMDouble(p, cs.ob) as sim:
        if fl.magic:
            sim.set_trt(fl.magic)
        if fl.drive:
            sim.set_drive(fl.drive)
        if fl.opened is not None:
            sim.set_open(*fl.opened)
        sim.upload(cs.f0)
        spun = None
        if cs.spin_up:
            sim.run(cs.spin_up)
            spun = sim.final_state()
        sim.set_scalar(cs.D, cs.c0, cs.wall, cs.inlet)
        seen, done = {}, 0
        for n in cs.samples:
            sim.run(n - done)
            done = n
            seen[n] = sim.scalar_field()
        return cs, seen, spun, sim.final_state()


def entry_of(fix, kind, D):
    (e,) = [e for e in fix["entries"] if e["kind"] == kind and (D is None or e["D"] == D)]
    return e


@pytest.mark.parametrize("kind,D", [r for r in sref.RUNS if r[0] != "taylor"])
def test_flows_with_known_answers(lbm, fix, kind, D):
    cs, seen, _, final = device_run(lbm, kind, D)
    if kind == "open":                                                              # the flow stays uniform: asserted first
        u_x, u_y = final[0], final[1]
        assert np.max(np.abs(u_x - sref.OPEN["u_in"])) <= 1e-10 and np.max(np.abs(u_y)) <= 1e-10
    fig = sref.figures(kind, cs, seen)
    print(kind, D, fig)
    sref.gates(kind, fig, entry_of(fix, kind, D))


def test_taylor_aris_dispersion(lbm, fix):
    cs, seen, spun, _ = device_run(lbm, "taylor", None)
    stored = entry_of(fix, "taylor", None)
    dev = sref.taylor_parabola_deviation(spun[0], spun[3])
    assert dev <= min(100.0 * stored["parabola_deviation"], sref.TAYLOR["parabola_gate"]), dev
    fig = sref.figures("taylor", cs, seen)
    print("taylor", fig, "parabola deviation", dev)
    sref.gates("taylor", fig)
    for key in ("d_eff_ratio", "speed_ratio"):
        assert abs(fig[key] / stored[key] - 1.0) <= 1e-9, (key, fig[key], stored[key])


# ---- 8. errors and what keeps the setting -------------------------------------------------------------------------------------

def test_errors_and_what_keeps_the_setting(lbm):
    lib = lbm.load_library()
    nx, ny = 17, 16
    case = make_case(lbm, nx, ny, (0, 0, 0, 0, 0, 0))
    m = case.members[0]
    s = m.scalar
    ptr = lambda a: a.ctypes.data                                                    # noqa: E731
    c0, wall, inlet = (np.ascontiguousarray(a) for a in (s.c0, s.wall, s.inlet))
    out = np.zeros((5, ny, nx))
    with dm.open_context(lbm, case, m, 0) as sim:
        # off: the three transfers are refused, the getter says off
        for call in (lib.lbm_dscalar_field, lib.lbm_dscalar_download, lib.lbm_dscalar_upload):
            assert call(sim.ctx, ptr(out)) == LBM_ERR_ARG
            assert "scalar is off" in lib.lbm_last_error().decode()
        assert sim.scalar() is None
        sim.set_scalar(s.D, c0, wall, inlet)
        sim.run(2)
        before = sim.scalar_cells()
        bad_c0, bad_wall, bad_in = c0.copy(), wall.copy(), inlet.copy()
        bad_c0[3, 4], bad_wall[0, 2], bad_in[5] = np.nan, np.inf, np.inf
        for args in ((-0.1, ptr(c0), None, None), (float("nan"), ptr(c0), None, None), (float("inf"), ptr(c0), None, None),
                     (0.1, None, None, None), (0.1, ptr(bad_c0), None, None), (0.1, ptr(c0), ptr(bad_wall), None),
                     (0.1, ptr(c0), None, ptr(bad_in))):
            assert lib.lbm_dscalar_set(sim.ctx, *args) == LBM_ERR_ARG, args
        assert lib.lbm_dscalar_get(sim.ctx, None, None, None) == LBM_ERR_ARG
        for call in (lib.lbm_dscalar_field, lib.lbm_dscalar_download, lib.lbm_dscalar_upload):
            assert call(sim.ctx, None) == LBM_ERR_ARG
        # nothing has changed after the refusals
        assert sim.scalar() == (s.D, float(sref.omega_s(s.D))) and np.array_equal(sim.scalar_cells(), before)
        # upload_obstacles keeps the scalar state; set is allowed at any step count
        sim.upload_obstacles(m.ob)
        assert np.array_equal(sim.scalar_cells(), before)
        sim.set_scalar(0.3, 1.0)
        assert sim.steps_done == 2 and np.array_equal(sim.scalar_cells(), sref.init(np.ones((ny, nx))))
    with dm.open_ensemble(lbm, case) as ens:
        ds = np.array(DS)
        c0s = np.ascontiguousarray(np.stack([x.scalar.c0 for x in case.members]))
        for bad, name in ((0.0, "member 1"), (-1.0, "member 1"), (np.nan, "member 1")):
            d = ds.copy()
            d[1] = bad
            assert lib.lbm_dscalar_ens_set(ens.ens, ptr(d), ptr(c0s), None, None) == LBM_ERR_ARG
            assert name in lib.lbm_last_error().decode()
        assert lib.lbm_dscalar_ens_set(ens.ens, ptr(ds), None, None, None) == LBM_ERR_ARG
        bad = c0s.copy()
        bad[2, 1, 1] = np.inf
        assert lib.lbm_dscalar_ens_set(ens.ens, ptr(ds), ptr(bad), None, None) == LBM_ERR_ARG
        assert "member 2" in lib.lbm_last_error().decode()
        assert ens.scalar() is None
        outs = np.zeros((case.n, 5, ny, nx))
        for call in (lib.lbm_dscalar_ens_field, lib.lbm_dscalar_ens_download, lib.lbm_dscalar_ens_upload):
            assert call(ens.ens, ptr(outs)) == LBM_ERR_ARG
            assert "scalar is off" in lib.lbm_last_error().decode()
        set_scalars(ens, case.members)
        ens.run(1)
        before = ens.scalar_cells()
        # a steady run is refused while a scalar is on, under both criteria, and nothing changes
        for on in ("av_vels", "drag"):
            with pytest.raises(lbm.LBMError) as err:
                ens.run_until(4, window=2, rel_tol=1e-3, on=on)
            assert "code %d" % LBM_ERR_ARG in str(err.value) and "gated scalar kernel" in str(err.value)
        assert ens.steps_done == 1 and np.array_equal(ens.scalar_cells(), before)
        ens.set_scalar(None)
        assert ens.scalar() is None
        steps, conv = ens.run_until(4, window=2, rel_tol=0.0)                      # works again
        assert steps.tolist() == [5] * case.n and not conv.any()

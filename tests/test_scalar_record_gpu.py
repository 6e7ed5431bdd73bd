"""The scalar's record (include/lbm.h, "Scalar record"; lbm_drecord_*) and the steady runs that stop each member on it
(lbm_drecord_steady_run) on the GPU: dp_scalar_step_rec<false> and <true>, d2q9_dp_buoyant_gated and the ragged reads against
tests/_scalar_record_ref.py, bit for bit.

The cases, masks, inputs and drivers of the flow are tests/_dp_matrix.py's (a case has three members, each with its own obstacle
map, omega, state and scalar of its own diffusivity); the buoyant members take the b and c_ref of tests/test_buoy_gpu.py.

  1. bits: 33x19 (odd width, three segments, the last partly idle), 17x16 (a lane without a second cell) and 6x5 (less than one
     segment); the flow with all options off, OPEN alone (the inlet and outlet statements enter c) and all on; each passive and
     buoyant; LBMDouble at "multistep" 0 and 8 and EnsembleDouble; runs of 1, 2 and 10 steps: the three records equal the
     restatement by np.array_equal after each run, with both states; a member equals its context; 10 against 3 + 7;
  2. the record changes nothing: cells, scalar populations, av_vels, the force record and the four fields with it on and off;
  3. steady runs: the box sweep (buoyant, on="scalar_flux_x") and the channel sweep (passive, on="scalar"), the wanted stops from
     the fixture (tests/golden/scalar_steady.json: _steady_rule.rule on the restatement's record of a plain run to the cap);
     per member everything equals a fresh EnsembleDouble and an LBMDouble advanced to that member's count by one run; the ragged
     reads, the refusals while ragged, and the upload that ends it;
  4. the known flow: the convective Nusselt number of _buoy_ref.CAVITY from the last entry of flux_x;
  5. the old criteria stay refused with a scalar on; errors, and that a failed call changes nothing.

The comparisons with numpy rest on the device's double-precision division and square root being correctly rounded, as those of
tests/test_scalar_gpu.py do.  Bits are asked for, and bits hold: on an MI355X all 59 cases pass in 2.1 s, the longest the first
(0.3 s, with the library's load) and the cavity's 20000 steps (0.2 s)."""
from types import SimpleNamespace

import numpy as np
import pytest

import _buoy_ref as bref
import _dp_matrix as dm
import _scalar_record_ref as rr
import _scalar_ref as sref
import _steady_rule

pytestmark = pytest.mark.gpu

LBM_ERR_ARG, LBM_ERR_STATE = 1, 3
SHAPES = dm.SHAPES
RUNS = [1, 2, 10]
#          force trt open wall les drive
OPTIONS = [(0, 0, 0, 0, 0, 0), (0, 0, 1, 0, 0, 0), (1, 1, 1, 1, 1, 1)]
FAMILIES = [0, 8, "ensemble"]
BS = [(3e-5, -2e-5), (-1e-5, 4e-5), (2e-5, 1e-5)]                              # per member, tests/test_buoy_gpu.py's
C_REFS = [1.0, 0.8, 1.2]
_refs, _runs = {}, {}


@pytest.fixture(scope="module")
def fix():
    return rr.fixture()


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def make_case(lbm, nx, ny, opts, steps=sum(RUNS)):
    force, trt, opened, wall, les, drive = opts
    return dm.make_case(lbm, nx, ny, 3, steps, force, trt, opened, wall="on" if wall else None, les="on" if les else None,
                        drive="on" if drive else None, scalar=True)


def narrow(lbm, buoyant):
    case = dm.narrow_case(lbm, drive="on" if buoyant else None, scalar=True)
    case.steps = sum(RUNS)
    for m in case.members:
        m.p.max_iters = sum(RUNS)
    return case


def setting_of(m, k):
    return bref.setting(m.ob, m.p.density, m.p.accel, m.p.omega, BS[k], C_REFS[k], m.scalar.D, magic=m.magic, opened=m.open,
                        wall=m.wall if isinstance(m.wall, tuple) else None, les=m.les if isinstance(m.les, float) else None,
                        drive=m.drive if isinstance(m.drive, tuple) else None, c_wall=m.scalar.wall, c_in=m.scalar.inlet)


def reference_of(oracle_f64, key, case, steps, buoyant):
    """per member: both states after every step (index 0: before the first) and the three records, float64[3, steps]"""
    key = (buoyant,) + key
    if key in _refs:
        return _refs[key]
    out = []
    for k, m in enumerate(case.members):
        f, g, rec = [m.cells0], [sref.init(m.scalar.c0)], []
        if buoyant:
            s = setting_of(m, k)
            for _ in range(steps):
                f1, g1, r = rr.buoyant_advance(f[-1], g[-1], s)[:3]
                f.append(f1), g.append(g1), rec.append(r)
        else:
            # the flow by the routed reference of tests/_dp_matrix.py, the scalar on the state each flow step streams
            f = dm.reference_run(oracle_f64, m, steps).states
            drive = m.drive if isinstance(m.drive, tuple) else None
            for n in range(steps):
                fa = f[n] if m.open is not None else sref.accelerate(f[n], m.ob, m.p.density, m.p.accel)
                g1, r = rr.passive_entry(fa, g[-1], m.ob, sref.omega_s(m.scalar.D), drive, m.scalar.wall,
                                         m.scalar.inlet if m.open is not None else None)
                g.append(g1), rec.append(r)
        out.append(SimpleNamespace(f=f, g=g, rec=np.array(rec).T))
    _refs[key] = out
    return out


def set_buoyancy(handle, ks):
    if len(ks) == 1:
        handle.set_buoyancy(BS[ks[0]], C_REFS[ks[0]])
    else:
        handle.set_buoyancy([BS[k] for k in ks], [C_REFS[k] for k in ks])


def drive(lbm, family, case, runs, buoyant, record=True):
    """per member: the flow's state, the scalar's populations, final_state and the three records after each run, av_vels and the
    force record"""
    results = []

    def loop(handle, ks):
        assert not handle.scalar_record_on()
        if buoyant:
            set_buoyancy(handle, ks)
        if record:
            handle.set_scalar_record(True)
        assert handle.scalar_record_on() == record
        states, g, fin, rec = [], [], [], []
        for r in runs:
            handle.run(r)
            states.append(handle.download(av_vels=False)[0])
            g.append(handle.scalar_cells())
            fin.append(handle.final_state())
            rec.append(handle.scalar_record() if record else None)
        return states, g, fin, rec, handle.download(cells=False)[1], (handle.force_record() if case.force else None)

    if family == "ensemble":
        with dm.open_ensemble(lbm, case, scalar=True) as ens:
            states, g, fin, rec, av, force = loop(ens, list(range(case.n)))
        for k in range(case.n):
            results.append(SimpleNamespace(states=[s[k] for s in states], g=[x[k] for x in g], fin=[[a[k] for a in x] for x in fin],
                                           rec=[None if r is None else np.stack([v[k] for v in r]) for r in rec], av=av[k],
                                           fx=None if force is None else force[0][k], fy=None if force is None else force[1][k]))
    else:
        for k, m in enumerate(case.members):
            with dm.open_context(lbm, case, m, family, scalar=True) as sim:
                states, g, fin, rec, av, force = loop(sim, [k])
            results.append(SimpleNamespace(states=states, g=g, fin=fin, rec=[None if r is None else np.stack(r) for r in rec], av=av,
                                           fx=None if force is None else force[0], fy=None if force is None else force[1]))
    return results


def run_of(lbm, key, family, case, runs, buoyant, record=True):
    k = (family, buoyant, record) + key
    if k not in _runs:
        _runs[k] = drive(lbm, family, case, runs, buoyant, record)
    return _runs[k]


def assert_equals_the_reference(refs, got, runs, what):
    for k, (ref, res) in enumerate(zip(refs, got)):
        done = 0
        for i, r in enumerate(runs):
            done += r
            assert np.array_equal(res.g[i], ref.g[done]), (what, k, done)
            assert np.array_equal(res.states[i], ref.f[done]), (what, k, done)
            assert res.rec[i].shape == (3, done)
            for v, name in enumerate(rr.NAMES):
                assert np.array_equal(res.rec[i][v], ref.rec[v, :done]), (what, k, done, name, res.rec[i][v], ref.rec[v, :done])
        assert np.all(np.isfinite(res.rec[-1])) and np.all(res.rec[-1][0] > 0.0) and np.all(res.rec[-1][1:] != 0.0), (what, k)


def assert_same_bits(a, b, what, records=True):
    for k, (x, y) in enumerate(zip(a, b)):
        assert all(np.array_equal(s, t) for s, t in zip(x.states, y.states)), (what, k)
        assert all(np.array_equal(s, t) for s, t in zip(x.g, y.g)), (what, k)
        assert all(np.array_equal(s, t) for p, q in zip(x.fin, y.fin) for s, t in zip(p, q)), (what, k)
        assert np.array_equal(x.av, y.av), (what, k)
        assert (x.fx is None) == (y.fx is None)
        if x.fx is not None:
            assert np.array_equal(x.fx, y.fx) and np.array_equal(x.fy, y.fy), (what, k)
        if records:
            assert all(np.array_equal(s, t) for s, t in zip(x.rec, y.rec)), (what, k)


# ---- 1. bits ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("buoyant", [False, True], ids=["passive", "buoyant"])
@pytest.mark.parametrize("opts", OPTIONS)
def test_the_record_equals_the_restatement(lbm, oracle_f64, opts, buoyant, family, nx, ny):
    what = "%s %s<%s> %dx%d" % ("buoyant" if buoyant else "passive", family, ",".join(map(str, opts)), nx, ny)
    case = make_case(lbm, nx, ny, opts)
    refs = reference_of(oracle_f64, (nx, ny) + opts, case, sum(RUNS), buoyant)
    got = run_of(lbm, (nx, ny) + opts, family, case, RUNS, buoyant)
    assert_equals_the_reference(refs, got, RUNS, what)
    assert len({r.rec[-1].tobytes() for r in got}) == case.n                        # the members are different scalars
    if family == "ensemble":
        for other in (0, 8):                                                        # a member is its context, bit for bit
            assert_same_bits(got, run_of(lbm, (nx, ny) + opts, other, case, RUNS, buoyant), what)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("buoyant", [False, True], ids=["passive", "buoyant"])
def test_less_than_one_segment(lbm, oracle_f64, buoyant, family):
    case = narrow(lbm, buoyant)
    assert (case.nx, case.ny) == (6, 5)
    refs = reference_of(oracle_f64, ("narrow",), case, sum(RUNS), buoyant)
    got = run_of(lbm, ("narrow",), family, case, RUNS, buoyant)
    assert_equals_the_reference(refs, got, RUNS, "%s 6x5" % family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("buoyant", [False, True], ids=["passive", "buoyant"])
def test_one_run_of_ten_against_three_and_seven(lbm, buoyant, family):
    nx, ny = SHAPES[0]
    opts = (1, 1, 0, 1, 0, 1)
    whole = run_of(lbm, ("ten", 10), family, make_case(lbm, nx, ny, opts, 10), [10], buoyant)
    split = run_of(lbm, ("ten", 3, 7), family, make_case(lbm, nx, ny, opts, 10), [3, 7], buoyant)
    for k, (a, b) in enumerate(zip(whole, split)):
        assert np.array_equal(a.g[-1], b.g[-1]) and np.array_equal(a.states[-1], b.states[-1]), (family, k)
        assert np.array_equal(a.rec[-1], b.rec[-1]) and np.array_equal(b.rec[0], a.rec[-1][:, :3]), (family, k)
        assert np.array_equal(a.av, b.av) and np.array_equal(a.fx, b.fx) and np.array_equal(a.fy, b.fy), (family, k)


# ---- 2. the record changes nothing ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("buoyant", [False, True], ids=["passive", "buoyant"])
def test_the_record_changes_nothing(lbm, buoyant, family):
    nx, ny = SHAPES[0]
    opts = (1, 1, 1, 1, 1, 1)
    on = run_of(lbm, (nx, ny) + opts, family, make_case(lbm, nx, ny, opts), RUNS, buoyant)
    off = run_of(lbm, (nx, ny) + opts, family, make_case(lbm, nx, ny, opts), RUNS, buoyant, record=False)
    assert on[0].fx is not None and all(r is None for r in off[0].rec)
    assert_same_bits(on, off, "%s record on against off" % family, records=False)


# ---- 3. steady runs ------------------------------------------------------------------------------------------------------------

def open_sweep(lbm, setups, cap, one=None):
    """the members of a sweep (rr.box / rr.channel setups) as one uploaded EnsembleDouble with scalars, buoyancy where the setup
    has it, and the record on; one: that member alone as an LBMDouble"""
    buoyant = hasattr(setups[0], "s")
    ob = setups[0].s.ob if buoyant else setups[0].ob
    ny, nx = ob.shape
    if buoyant:
        params = [lbm.make_dparams(nx, ny, cap, density=cs.s.density, accel=cs.s.accel, omega=cs.s.omega, obstacles=ob) for cs in setups]
        Ds, walls = [cs.s.D for cs in setups], [cs.s.c_wall for cs in setups]
    else:
        params = [lbm.make_dparams(nx, ny, cap, density=cs.fl.density, accel=cs.fl.accel, omega=cs.fl.omega, obstacles=ob) for cs in setups]
        Ds, walls = [cs.D for cs in setups], [cs.wall for cs in setups]
    if one is not None:
        cs = setups[one]
        h = lbm.LBMDouble(params[one], ob)
        h.upload(cs.f0)
        h.set_scalar(Ds[one], cs.c0, walls[one])
        if buoyant:
            h.set_buoyancy(cs.s.b, cs.s.c_ref)
    else:
        h = lbm.EnsembleDouble(params, ob)
        h.upload(np.stack([cs.f0 for cs in setups]))
        h.set_scalar(Ds, np.stack([cs.c0 for cs in setups]), np.stack(walls))
        if buoyant:
            h.set_buoyancy([cs.s.b for cs in setups], [cs.s.c_ref for cs in setups])
    h.set_scalar_record(True)
    return h


def everything(h, k=None):
    """what a member is compared in: cells, scalar populations, av_vels, the three records, final_state"""
    cells, av = h.download()
    out = [cells, h.scalar_cells(), av] + list(h.scalar_record()) + list(h.final_state()) + [h.scalar_field()]
    return out if k is None else [a[k] for a in out]


@pytest.mark.parametrize("name", ["box", "channel"])
def test_a_steady_run_stops_each_member_on_its_own_record(lbm, fix, name):
    sweep, make = (rr.BOX, rr.box) if name == "box" else (rr.CHANNEL, rr.channel)
    stored = fix[name]
    rr.check_stops(stored, sweep, members_at_cap=1 if name == "box" else 0)
    setups = [make(v) for v in stored["members"]]
    n, cap, window, tol = len(setups), sweep["cap"], sweep["window"], sweep["rel_tol"]
    on = rr.CRITERIA[sweep["which"]]
    which = rr.NAMES.index(sweep["which"])
    # the wanted stops never come from run_until: the fixture's, and the rule on the device's own record of a plain run to the cap
    with open_sweep(lbm, setups, cap) as ens:
        ens.run(cap)
        whole = ens.scalar_record()
    want_steps, want_conv = _steady_rule.rule(np.ascontiguousarray(whole[which]), 0, cap, window, tol)
    assert want_steps.tolist() == stored["stops"] and want_conv.tolist() == stored["converged"]
    for k in range(n):
        for v in range(3):
            assert bref.close(whole[v][k, stored["stops"][k] - 1], stored["last"][k][v]), (name, k, v)
    with open_sweep(lbm, setups, cap) as ens:
        steps, conv = ens.run_until(cap, window=window, rel_tol=tol, on=on)
        assert steps.tolist() == stored["stops"] and conv.tolist() == stored["converged"], (steps, conv)
        ms, mc = ens.member_steps()
        assert ms.tolist() == stored["stops"] and mc.tolist() == stored["converged"] and ens.steps_done == max(stored["stops"])
        got = everything(ens)
        T = ens.steps_done
        for k in range(n):
            c = stored["stops"][k]
            for v in range(3):
                assert np.array_equal(got[3 + v][k, :c], whole[v][k, :c]), (name, k, v)
                assert dm.plus_zero(got[3 + v][k, c:]) and got[3 + v].shape == (n, T), (name, k, v)      # +0.0 beyond its count
            assert dm.plus_zero(got[2][k, c:])
        # per member: a fresh ensemble and a context advanced to that member's count by one run
        for k in range(n):
            c = stored["stops"][k]
            mine = [a[k] for a in got]
            with open_sweep(lbm, setups, cap) as fresh:
                fresh.run(c)
                ref = everything(fresh, k)
            with open_sweep(lbm, setups, cap, one=k) as sim:
                sim.run(c)
                ctx = everything(sim)
            for i, (a, b, d) in enumerate(zip(mine, ref, ctx)):
                a = a[:c] if 2 <= i <= 5 else a
                assert np.array_equal(a, b) and np.array_equal(a, d), (name, k, i)
        ragged = len(set(stored["stops"])) > 1
        assert ragged
        # while ragged: the reads above returned each member's own state; run, set and upload of the scalar are refused
        before = ens.scalar_cells()
        lib = lbm.load_library()
        with pytest.raises(lbm.LBMError) as err:
            ens.run(1)
        assert "code %d" % LBM_ERR_STATE in str(err.value) and "different step counts" in str(err.value)
        with pytest.raises(lbm.LBMError) as err:
            ens.upload_scalar(before)
        assert "code %d" % LBM_ERR_STATE in str(err.value) and "different step counts" in str(err.value)
        D = np.full(n, 0.1)
        c0 = np.zeros((n,) + before.shape[2:])
        assert lib.lbm_dscalar_ens_set(ens.ens, D.ctypes.data, c0.ctypes.data, None, None) == LBM_ERR_STATE
        assert np.array_equal(ens.scalar_cells(), before) and ens.scalar_record_on()
        # the upload of the flow ends it: the scalar populations are unchanged, and one more step is a context's from those two states
        flow = got[0]
        ens.upload(flow)
        assert np.array_equal(ens.scalar_cells(), before) and ens.steps_done == 0
        ens.run(1)
        after = everything(ens)
        for k in range(n):
            with open_sweep(lbm, setups, cap, one=k) as sim:
                sim.upload(flow[k])
                sim.upload_scalar(before[k])
                sim.run(1)
                ctx = everything(sim)
            for i, (a, d) in enumerate(zip([x[k] for x in after], ctx)):
                assert np.array_equal(a, d), (name, "after the upload", k, i)


# ---- 4. a known flow -----------------------------------------------------------------------------------------------------------

def test_the_cavitys_convective_nusselt_number(lbm, fix):
    C = bref.CAVITY
    cs = bref.cavity()
    stored = fix["cavity"]
    with open_sweep(lbm, [cs], C["steps"], one=0) as sim:
        sim.run(C["steps"])
        flux_x = sim.scalar_record()[1]
    nu = rr.nusselt_convective(flux_x[-1], cs.s.ob, C["H"], cs.s.D)
    print("cavity: 1 + <c u_x> H / (kappa dC) = %.10f after %d steps (fixture %.10f, de Vahl Davis 1.118; the restatement deviates "
          "by %.3e)" % (nu, C["steps"], stored["nusselt"], stored["deviation"]))
    assert bref.close(nu, stored["nusselt"])
    assert abs(stored["nusselt"] / C["theory"] - 1.0) <= 2.0 * stored["deviation"] and abs(nu / C["theory"] - 1.0) <= 2.0 * stored["deviation"]


# ---- 5. the old criteria, errors, and what a failed call changes ---------------------------------------------------------------

def test_the_old_criteria_stay_refused(lbm):
    case = make_case(lbm, 17, 16, (1, 0, 0, 0, 0, 0))
    with dm.open_ensemble(lbm, case, scalar=True) as ens:
        ens.set_scalar_record(True)
        ens.run(1)
        before = everything(ens)
        for on in ("av_vels", "drag"):
            with pytest.raises(lbm.LBMError) as err:
                ens.run_until(4, window=2, rel_tol=1e-3, on=on)
            assert "code %d" % LBM_ERR_ARG in str(err.value) and "gated scalar kernel" in str(err.value)
        assert ens.steps_done == 1 and all(np.array_equal(a, b) for a, b in zip(everything(ens), before))
        steps, conv = ens.run_until(4, window=2, rel_tol=0.0, on="scalar_flux_y")    # the scalar's criterion runs
        assert steps.tolist() == [5] * case.n and not conv.any()


def test_errors_and_that_a_failed_call_changes_nothing(lbm):
    lib = lbm.load_library()
    case = make_case(lbm, 17, 16, (0, 0, 0, 0, 0, 0))
    m = case.members[0]
    out = np.full(16, 7.0)
    with dm.open_context(lbm, case, m, 0) as sim:
        # needs a scalar
        assert lib.lbm_drecord_set(sim.ctx, 1) == LBM_ERR_ARG
        assert "scalar is off" in lib.lbm_last_error().decode() and not sim.scalar_record_on()
        dm.set_scalars(sim, [m])
        assert lib.lbm_drecord_set(sim.ctx, 2) == LBM_ERR_ARG
        # a read while it is off
        assert lib.lbm_drecord(sim.ctx, out.ctypes.data, None, None) == LBM_ERR_STATE
        assert "no scalar record" in lib.lbm_last_error().decode() and np.all(out == 7.0)
        sim.set_scalar_record(True)
        sim.set_scalar_record(False)
        sim.set_scalar_record(True)
        assert lib.lbm_drecord(sim.ctx, None, None, None) == LBM_ERR_ARG
        # the scalar cannot go while its record is on; setting it again and uploading it are allowed and keep the entries
        assert lib.lbm_dscalar_set(sim.ctx, 0.0, None, None, None) == LBM_ERR_STATE
        assert "record is on" in lib.lbm_last_error().decode() and sim.scalar() is not None and sim.scalar_record_on()
        sim.run(2)
        first = [a.copy() for a in sim.scalar_record()]
        for value in (0, 1):                                                          # only before the first step, off included
            assert lib.lbm_drecord_set(sim.ctx, value) == LBM_ERR_STATE
            assert "2 done" in lib.lbm_last_error().decode()
        assert sim.scalar_record_on()
        sim.set_scalar(m.scalar.D, m.scalar.c0, m.scalar.wall, m.scalar.inlet)
        sim.upload_scalar(sim.scalar_cells())
        assert all(np.array_equal(a, b) for a, b in zip(sim.scalar_record(), first))
        sim.run(1)
        again = sim.scalar_record()
        assert all(a.shape == (3,) and np.array_equal(a[:2], b) for a, b in zip(again, first))
        assert np.array_equal(again[0][2], again[0][0])                              # the scalar started anew from c0: the first entry's content
        # one output alone
        only = np.zeros(3)
        assert lib.lbm_drecord(sim.ctx, None, only.ctypes.data, None) == 0 and np.array_equal(only, again[1])
        sim.upload(m.cells0)                                                         # the upload keeps the setting and starts anew
        assert sim.scalar_record_on() and all(a.shape == (0,) for a in sim.scalar_record())
        sim.set_scalar_record(False)
        sim.set_scalar(None)
        assert sim.scalar() is None and not sim.scalar_record_on()
    with dm.open_ensemble(lbm, case) as ens:
        assert lib.lbm_drecord_ens_set(ens.ens, 1) == LBM_ERR_ARG
        assert "scalar is off" in lib.lbm_last_error().decode()
        dm.set_scalars(ens, case.members)
        # a steady run without the record, and a bad `which` with it
        before = ens.scalar_cells()
        assert lib.lbm_drecord_steady_run(ens.ens, 4, 2, 1e-3, 0) == LBM_ERR_ARG
        assert "record" in lib.lbm_last_error().decode()
        assert lib.lbm_drecord_ens(ens.ens, out.ctypes.data, None, None) == LBM_ERR_STATE and np.all(out == 7.0)
        ens.set_scalar_record(True)
        for which in (-1, 3):
            assert lib.lbm_drecord_steady_run(ens.ens, 4, 2, 1e-3, which) == LBM_ERR_ARG
        assert lib.lbm_drecord_ens(ens.ens, None, None, None) == LBM_ERR_ARG
        assert lib.lbm_dscalar_ens_set(ens.ens, None, None, None, None) == LBM_ERR_STATE
        assert ens.steps_done == 0 and np.array_equal(ens.scalar_cells(), before) and ens.scalar_record_on()
        with pytest.raises(ValueError):
            ens.run_until(4, on="scalar_flux_z")
        ens.run(1)
        assert lib.lbm_drecord_ens_set(ens.ens, 0) == LBM_ERR_STATE and ens.scalar_record_on()

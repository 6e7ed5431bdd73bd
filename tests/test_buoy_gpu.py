"""Buoyancy (include/lbm.h, "Buoyancy"; lbm_dbuoy_*) on the GPU: dp_scalar_step<true>, d2q9_dp_buoyant and the output stage
against tests/_buoy_ref.py, bit for bit, and the flows with known answers end to end.

The cases, masks, inputs and drivers of the flow are tests/_dp_matrix.py's (make_case with `scalar`; open_context and open_ensemble
set the scalar behind the upload, and set_buoyancy follows it here): a case has three members, each with its own obstacle map,
omega, state, scalar and here its own b and c_ref.

  1. bits: 33x19 and 17x16 (odd nx, a lane without its second cell, a last segment that is not full) and 6x5, the flow with all
     options off, each of FORCE, TRT, OPEN, WALL, LES and set_drive alone and all on, LBMDouble at "multistep" 0 and 8 and
     EnsembleDouble, runs of 1, 2 and 10 steps: cells, scalar populations, av_vels, the force record and the four fields of
     final_state equal the restatement by np.array_equal after each run; a member equals its context; "multistep" 0 and 8 agree;
     a run of 10 against 3 + 7; download -> upload of both states -> run against a plain run;
  2. the tie to the existing kernels: c0 = 0, c_ref = 0, insulating walls, b != 0 and set_drive((1e-6, 0)) keep C at exactly 0,
     and cells and av_vels equal a handle with the same drive, a passive scalar and no buoyancy (d2q9_dp_step<..., DRIVE>); off is
     off;
  3. the flows: the stratified layer comes to rest, Rayleigh-Benard onset between Ra 1500 and 1900 in one ensemble, the
     side-heated cavity's Nusselt number; the fixture's figures (tests/golden/buoy.json, from the restatement) to 1e-9 relative,
     the rounding-level figure of the layer at rest under 100 x the restatement's own;
  4. errors and what keeps the setting.

The comparisons with numpy rest on the device's double-precision division and square root being correctly rounded, as those of
tests/test_scalar_gpu.py do.  Bits are asked for, and bits hold: on an MI355X all 67 cases pass in 2.6 s, the longest the
layer's 20000 steps."""
from types import SimpleNamespace

import numpy as np
import pytest

import _buoy_ref as bref
import _dp_matrix as dm
import _scalar_ref as sref

pytestmark = pytest.mark.gpu

LBM_ERR_ARG, LBM_ERR_STATE = 1, 3
SHAPES = dm.SHAPES
RUNS = [1, 2, 10]
#          force trt open wall les drive
OPTIONS = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), (0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 0), (0, 0, 0, 0, 1, 0),
           (0, 0, 0, 0, 0, 1), (1, 1, 1, 1, 1, 1)]
FAMILIES = [0, 8, "ensemble"]
BS = [(3e-5, -2e-5), (-1e-5, 4e-5), (2e-5, 1e-5)]                              # per member: b, of the size of dm.FORCES
C_REFS = [1.0, 0.8, 1.2]                                                      # c0 lies in 0.5 .. 1.5
_refs, _runs = {}, {}


@pytest.fixture(scope="module")
def fix():
    return bref.fixture()


def make_case(lbm, nx, ny, opts, steps=sum(RUNS)):
    force, trt, opened, wall, les, drive = opts
    return dm.make_case(lbm, nx, ny, 3, steps, force, trt, opened, wall="on" if wall else None, les="on" if les else None,
                        drive="on" if drive else None, scalar=True)


def narrow(lbm):
    case = dm.narrow_case(lbm, drive="on", scalar=True)
    case.steps = sum(RUNS)
    for m in case.members:
        m.p.max_iters = sum(RUNS)
    return case


def setting_of(m, k):
    return bref.setting(m.ob, m.p.density, m.p.accel, m.p.omega, BS[k], C_REFS[k], m.scalar.D, magic=m.magic, opened=m.open,
                        wall=m.wall if isinstance(m.wall, tuple) else None, les=m.les if isinstance(m.les, float) else None,
                        drive=m.drive if isinstance(m.drive, tuple) else None, c_wall=m.scalar.wall, c_in=m.scalar.inlet)


def reference_of(key, case, steps):
    """per member: both states and the output stage's fields after every step (index 0: before the first), and the records"""
    if key in _refs:
        return _refs[key]
    out = []
    for k, m in enumerate(case.members):
        s = setting_of(m, k)
        counted = bref.counted_cells(m.ob, m.body, m.open is not None) if case.force else None
        f, g = [m.cells0], [sref.init(m.scalar.c0)]
        av, fx, fy = [], [], []
        for _ in range(steps):
            f1, g1, u, fa = bref.advance(f[-1], g[-1], s)
            a, x, y = bref.record(u, fa, m.ob, m.p.free_cells_inv, counted)
            f.append(f1), g.append(g1), av.append(a), fx.append(x), fy.append(y)
        out.append(SimpleNamespace(s=s, f=f, g=g, av=np.array(av), fx=np.array(fx), fy=np.array(fy)))
    _refs[key] = out
    return out


def set_buoyancy(handle, ks):
    """the members' b and c_ref, read back"""
    if len(ks) == 1:
        handle.set_buoyancy(BS[ks[0]], C_REFS[ks[0]])
        assert handle.buoyancy() == (BS[ks[0]], C_REFS[ks[0]])
    else:
        handle.set_buoyancy([BS[k] for k in ks], [C_REFS[k] for k in ks])
        assert np.array_equal(handle.buoyancy(), [BS[k] + (C_REFS[k],) for k in ks])


def drive(lbm, family, case, runs, buoyant=True, between=None):
    """per member: the flow's state, the scalar's populations and final_state after each run, av_vels and the force record.
    between(handle): called behind every run but the last"""
    results = []

    def loop(handle, ks):
        assert handle.buoyancy() is None
        if buoyant:
            set_buoyancy(handle, ks)
        states, g, fin = [], [], []
        for i, r in enumerate(runs):
            handle.run(r)
            states.append(handle.download(av_vels=False)[0])
            g.append(handle.scalar_cells())
            fin.append(handle.final_state())
            if between is not None and i + 1 < len(runs):
                between(handle)
        return states, g, fin, handle.download(cells=False)[1], (handle.force_record() if case.force else None)

    if family == "ensemble":
        with dm.open_ensemble(lbm, case, scalar=True) as ens:
            states, g, fin, av, rec = loop(ens, list(range(case.n)))
        for k in range(case.n):
            results.append(SimpleNamespace(states=[s[k] for s in states], g=[x[k] for x in g], fin=[[a[k] for a in x] for x in fin],
                                           av=av[k], fx=None if rec is None else rec[0][k], fy=None if rec is None else rec[1][k]))
    else:
        for k, m in enumerate(case.members):
            with dm.open_context(lbm, case, m, family, scalar=True) as sim:
                states, g, fin, av, rec = loop(sim, [k])
            results.append(SimpleNamespace(states=states, g=g, fin=fin, av=av, fx=None if rec is None else rec[0],
                                           fy=None if rec is None else rec[1]))
    return results


def run_of(lbm, key, family, case, runs, buoyant=True):
    k = (family, buoyant) + key
    if k not in _runs:
        _runs[k] = drive(lbm, family, case, runs, buoyant)
    return _runs[k]


def assert_equals_the_reference(case, refs, got, runs, what):
    for k, (m, ref, res) in enumerate(zip(case.members, refs, got)):
        done = 0
        for i, r in enumerate(runs):
            done += r
            assert np.array_equal(res.g[i], ref.g[done]), (what, k, done, int(np.count_nonzero(res.g[i] != ref.g[done])))
            assert np.array_equal(res.states[i], ref.f[done]), (what, k, done, int(np.count_nonzero(res.states[i] != ref.f[done])))
            want = bref.final_state(ref.f[done], ref.g[done], ref.s)
            for name, a, b in zip(("u_x", "u_y", "u", "pressure"), res.fin[i], want):
                assert np.array_equal(a, b), (what, k, done, name)
        assert res.av.shape == (done,) and np.array_equal(res.av, ref.av), (what, k, res.av, ref.av)
        if case.force:
            assert np.array_equal(res.fx, ref.fx) and np.array_equal(res.fy, ref.fy), (what, k, res.fx, ref.fx, res.fy, ref.fy)
            assert np.any(res.fx != 0.0)
        assert np.all(np.isfinite(res.g[-1])) and np.all(np.isfinite(res.states[-1]))


def assert_same_bits(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert all(np.array_equal(s, t) for s, t in zip(x.states, y.states)), (what, k)
        assert all(np.array_equal(s, t) for s, t in zip(x.g, y.g)), (what, k)
        assert all(np.array_equal(s, t) for p, q in zip(x.fin, y.fin) for s, t in zip(p, q)), (what, k)
        assert np.array_equal(x.av, y.av), (what, k)
        assert (x.fx is None) == (y.fx is None)
        if x.fx is not None:
            assert np.array_equal(x.fx, y.fx) and np.array_equal(x.fy, y.fy), (what, k)


# ---- 1. bits ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("opts", OPTIONS)
def test_both_states_equal_the_restatement(lbm, opts, family, nx, ny):
    what = "%s<%s> %dx%d" % (family, ",".join(map(str, opts)), nx, ny)
    case = make_case(lbm, nx, ny, opts)
    refs = reference_of((nx, ny) + opts, case, sum(RUNS))
    got = run_of(lbm, (nx, ny) + opts, family, case, RUNS)
    assert_equals_the_reference(case, refs, got, RUNS, what)
    assert len({r.states[-1].tobytes() for r in got}) == case.n                     # the members are different flows
    # buoyancy changes the flow: the passive path's first step is another one
    passive = run_of(lbm, (nx, ny) + opts, family, make_case(lbm, nx, ny, opts), RUNS, buoyant=False)
    assert all(not np.array_equal(a.states[0], b.states[0]) for a, b in zip(got, passive))
    if family == "ensemble":
        for other in (0, 8):                                                        # a member is its context, bit for bit
            assert_same_bits(got, run_of(lbm, (nx, ny) + opts, other, case, RUNS), what)
    if family == 8:                                                                 # "multistep" chooses nothing
        assert_same_bits(got, run_of(lbm, (nx, ny) + opts, 0, case, RUNS), what)


@pytest.mark.parametrize("family", FAMILIES)
def test_region_wider_than_the_grid(lbm, family):
    case = narrow(lbm)
    assert (case.nx, case.ny) == (6, 5)
    refs = reference_of(("narrow",), case, sum(RUNS))
    got = run_of(lbm, ("narrow",), family, case, RUNS)
    assert_equals_the_reference(case, refs, got, RUNS, "%s 6x5" % family)


@pytest.mark.parametrize("family", FAMILIES)
def test_one_run_of_ten_against_three_and_seven(lbm, family):
    nx, ny = SHAPES[0]
    opts = (1, 1, 0, 1, 0, 1)
    whole = run_of(lbm, ("ten", 10), family, make_case(lbm, nx, ny, opts, 10), [10])
    split = run_of(lbm, ("ten", 3, 7), family, make_case(lbm, nx, ny, opts, 10), [3, 7])
    for k, (a, b) in enumerate(zip(whole, split)):
        assert np.array_equal(a.g[-1], b.g[-1]) and np.array_equal(a.states[-1], b.states[-1]), (family, k)
        assert np.array_equal(a.av, b.av) and np.array_equal(a.fx, b.fx) and np.array_equal(a.fy, b.fy), (family, k)
        assert all(np.array_equal(s, t) for s, t in zip(a.fin[-1], b.fin[-1])), (family, k)


@pytest.mark.parametrize("family", FAMILIES)
def test_download_upload_of_both_states_changes_nothing(lbm, family):
    nx, ny = SHAPES[1]
    opts = (0, 1, 1, 0, 0, 0)
    plain = run_of(lbm, ("round",), family, make_case(lbm, nx, ny, opts), RUNS)
    seen = []

    def round_trip(handle):
        g = handle.scalar_cells()
        handle.upload_scalar(np.zeros_like(g))
        assert not np.any(handle.scalar_cells())
        handle.upload_scalar(g)
        seen.append(g)

    again = drive(lbm, family, make_case(lbm, nx, ny, opts), RUNS, between=round_trip)
    assert seen
    assert_same_bits(again, plain, family)
    # the flow's state too: upload() starts a new record, so the second half is a handle of its own
    case = make_case(lbm, nx, ny, opts)
    handles = ([dm.open_ensemble(lbm, case, scalar=True)] if family == "ensemble" else
               [dm.open_context(lbm, case, m, family, scalar=True) for m in case.members])
    for i, h in enumerate(handles):
        ks = list(range(case.n)) if family == "ensemble" else [i]
        with h:
            set_buoyancy(h, ks)
            h.run(RUNS[0])
            cells, g = h.download(av_vels=False)[0], h.scalar_cells()
            h.upload(cells)
            h.upload_scalar(g)
            assert h.buoyancy() is not None                                         # upload keeps the setting
            h.run(RUNS[1])
            cells, g = h.download(av_vels=False)[0], h.scalar_cells()
            for j, k in enumerate(ks):
                assert np.array_equal(cells[j] if family == "ensemble" else cells, plain[k].states[1]), (family, k)
                assert np.array_equal(g[j] if family == "ensemble" else g, plain[k].g[1]), (family, k)


# ---- 2. the tie to the existing kernels, and off is off -----------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES)
def test_a_scalar_that_stays_zero_is_the_body_force_alone(lbm, family):
    nx, ny = SHAPES[0]
    case = dm.make_case(lbm, nx, ny, 3, sum(RUNS), 1, 1, 0)
    f0 = (1e-6, 0.0)

    def run(buoyant, multistep):
        out = []
        handles = ([dm.open_ensemble(lbm, case)] if family == "ensemble" else [dm.open_context(lbm, case, m, multistep) for m in case.members])
        for i, h in enumerate(handles):
            ks = list(range(case.n)) if family == "ensemble" else [i]
            with h:
                # set_drive before the first step; the upload has been done, the record is empty
                h.set_drive(f0)
                h.set_scalar([dm.DS[k] for k in ks] if family == "ensemble" else dm.DS[i], 0.0)
                if buoyant:
                    h.set_buoyancy(BS[0] if len(ks) == 1 else [BS[k] for k in ks], 0.0)
                for r in RUNS:
                    h.run(r)
                cells, av = h.download()
                assert not np.any(h.scalar_cells())                                 # C is exactly 0 for ever
                out.append((cells, av, h.force_record(), h.final_state()))
        return out

    passive = run(False, 0 if family != "ensemble" else None)                       # d2q9_dp_step<..., DRIVE> in the contexts
    buoyant = run(True, family if family != "ensemble" else None)
    for a, b in zip(buoyant, passive):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


@pytest.mark.parametrize("family", FAMILIES)
def test_off_is_off(lbm, family):
    nx, ny = SHAPES[0]
    opts = (1, 0, 0, 0, 0, 1)
    case = make_case(lbm, nx, ny, opts)
    never = run_of(lbm, (nx, ny) + opts, family, case, RUNS, buoyant=False)
    handles = ([dm.open_ensemble(lbm, case, scalar=True)] if family == "ensemble" else
               [dm.open_context(lbm, case, m, family, scalar=True) for m in case.members])
    for i, h in enumerate(handles):
        ks = list(range(case.n)) if family == "ensemble" else [i]
        with h:
            set_buoyancy(h, ks)
            h.set_buoyancy(None if family == "ensemble" else (0.0, 0.0))
            assert h.buoyancy() is None
            for r in RUNS:
                h.run(r)
            cells, av = h.download()
            g = h.scalar_cells()
            for j, k in enumerate(ks):
                assert np.array_equal(cells[j] if family == "ensemble" else cells, never[k].states[-1]), (family, k)
                assert np.array_equal(av[j] if family == "ensemble" else av, never[k].av), (family, k)
                assert np.array_equal(g[j] if family == "ensemble" else g, never[k].g[-1]), (family, k)


# ---- 3. the flows with known answers ------------------------------------------------------------------------------------------

def open_flow(lbm, setups, steps):
    """the setups (one: an LBMDouble, more: the members of one EnsembleDouble) uploaded, with scalar and buoyancy set"""
    s0 = setups[0].s
    ny, nx = s0.ob.shape
    params = [lbm.make_dparams(nx, ny, steps, density=s0.density, accel=s0.accel, omega=cs.s.omega, obstacles=s0.ob) for cs in setups]
    if len(setups) == 1:
        cs = setups[0]
        h = lbm.LBMDouble(params[0], s0.ob)
        h.upload(cs.f0)
        h.set_scalar(cs.s.D, cs.c0, cs.s.c_wall)
        h.set_buoyancy(cs.s.b, cs.s.c_ref)
    else:
        h = lbm.EnsembleDouble(params, s0.ob)
        h.upload(np.stack([cs.f0 for cs in setups]))
        h.set_scalar([cs.s.D for cs in setups], np.stack([cs.c0 for cs in setups]), np.stack([cs.s.c_wall for cs in setups]))
        h.set_buoyancy([cs.s.b for cs in setups], [cs.s.c_ref for cs in setups])
    return h


def test_a_stratified_layer_comes_to_rest(lbm, fix):
    L = bref.LAYER
    cs = bref.layer(L["Ra"])
    with open_flow(lbm, [cs], L["steps"]) as sim:
        sim.run(1000)
        early = bref.max_uy(sim.final_state()[1], cs.s.ob)
        sim.run(L["steps"] - 1000)
        late = bref.max_uy(sim.final_state()[1], cs.s.ob)
        c = sim.scalar_field()
    print("stratified rest: max |u_y| %.3e after 1000 steps (fixture %.3e), %.3e after %d (fixture %.3e)" %
          (early, fix["rest"]["history"]["1000"], late, L["steps"], fix["rest"]["max_uy"]))
    assert bref.close(early, fix["rest"]["history"]["1000"])                        # the same digits while the layer still moves
    assert 0.0 <= late <= 100.0 * fix["rest"]["max_uy"]                             # rounding level: 100 x the restatement's own
    assert sref.walls_figure(c) <= 100.0 * fix["rest"]["profile"]                   # and the conduction profile stands


def test_rayleigh_benard_onset(lbm, fix):
    O = bref.ONSET
    setups = [bref.layer(Ra, O["eps"]) for Ra in O["Ras"]]
    ob = setups[0].s.ob
    with open_flow(lbm, setups, O["steps"]) as ens:
        ens.run(O["t0"])
        a0 = [bref.max_uy(u, ob) for u in ens.final_state()[1]]
        ens.run(O["steps"] - O["t0"])
        a1 = [bref.max_uy(u, ob) for u in ens.final_state()[1]]
    r0, r1, ra_c = bref.onset_figures(a0, a1)
    stored = fix["onset"]
    print("onset: rates %.6e at Ra 1500, %.6e at Ra 1900 per step, Ra_c %.2f (fixture %.2f, theory 1707.76)" % (r0, r1, ra_c, stored["Ra_c"]))
    assert a1[0] < a0[0] and a1[1] > a0[1]                                          # falls below the onset, rises above it
    assert abs(ra_c / O["theory"] - 1.0) <= 2.0 * stored["deviation"]
    assert bref.close(r0, stored["rates"][0]) and bref.close(r1, stored["rates"][1]) and bref.close(ra_c, stored["Ra_c"])


def test_side_heated_cavity(lbm, fix):
    C = bref.CAVITY
    cs = bref.cavity()
    with open_flow(lbm, [cs], C["steps"]) as sim:
        sim.run(C["steps"])
        nu = bref.nusselt(sim.scalar_field())
        u = float(np.max(sim.final_state()[2]))
    stored = fix["cavity"]
    print("cavity: Nu %.10f after %d steps (fixture %.10f, de Vahl Davis 1.118), max |u| %.4e" % (nu, C["steps"], stored["nusselt"], u))
    assert abs(nu / C["theory"] - 1.0) <= 2.0 * stored["deviation"]
    assert bref.close(nu, stored["nusselt"]) and bref.close(u, stored["max_u"])


# ---- 4. errors and what keeps the setting -------------------------------------------------------------------------------------

def test_errors_and_what_keeps_the_setting(lbm):
    lib = lbm.load_library()
    nx, ny = 17, 16
    case = make_case(lbm, nx, ny, (0, 0, 0, 0, 0, 0))
    m = case.members[0]
    ptr = lambda a: a.ctypes.data                                                    # noqa: E731
    with dm.open_context(lbm, case, m, 0) as sim:
        # needs a scalar; off is accepted without one
        assert lib.lbm_dbuoy_set(sim.ctx, 0.0, 1e-5, 0.5) == LBM_ERR_STATE
        assert "scalar is off" in lib.lbm_last_error().decode()
        sim.set_buoyancy((0.0, 0.0))
        assert sim.buoyancy() is None
        dm.set_scalars(sim, [m])
        sim.set_buoyancy((0.0, 1e-5), 0.5)
        assert sim.buoyancy() == ((0.0, 1e-5), 0.5)
        for bad in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 1e-5, np.nan)):
            assert lib.lbm_dbuoy_set(sim.ctx, *bad) == LBM_ERR_ARG
        assert lib.lbm_dbuoy_get(sim.ctx, None, None, None) == LBM_ERR_ARG
        # the scalar cannot go while the flow reads it; setting it again and uploading it are allowed
        assert lib.lbm_dscalar_set(sim.ctx, 0.0, None, None, None) == LBM_ERR_STATE
        assert "buoyancy is on" in lib.lbm_last_error().decode()
        assert sim.scalar() is not None and sim.buoyancy() == ((0.0, 1e-5), 0.5)
        sim.set_scalar(0.2, 1.0)
        sim.upload_scalar(sim.scalar_cells())
        sim.upload_obstacles(m.ob)
        sim.upload(m.cells0)
        assert sim.buoyancy() == ((0.0, 1e-5), 0.5)
        sim.run(2)
        # only before the first step, off included; nothing changes
        for args in ((1e-5, 0.0, 0.5), (0.0, 0.0, 0.0)):
            assert lib.lbm_dbuoy_set(sim.ctx, *args) == LBM_ERR_STATE
            assert "2 done" in lib.lbm_last_error().decode()
        assert sim.buoyancy() == ((0.0, 1e-5), 0.5)
        sim.upload(m.cells0)
        sim.set_buoyancy(None)
        assert sim.buoyancy() is None
        sim.set_scalar(None)
        assert sim.scalar() is None
    with dm.open_ensemble(lbm, case) as ens:
        b = np.array([BS[k] + (C_REFS[k],) for k in range(case.n)])
        assert lib.lbm_dbuoy_ens_set(ens.ens, ptr(b)) == LBM_ERR_STATE
        assert "scalar is off" in lib.lbm_last_error().decode()
        dm.set_scalars(ens, case.members)
        for at, bad, word in (((1, 0), np.nan, "member 1"), ((2, 2), np.inf, "member 2"), ((1, slice(0, 2)), 0.0, "member 1")):
            v = b.copy()
            v[at] = bad
            assert lib.lbm_dbuoy_ens_set(ens.ens, ptr(v)) == LBM_ERR_ARG
            assert word in lib.lbm_last_error().decode()
        assert ens.buoyancy() is None                                               # everything is checked before anything changes
        assert lib.lbm_dbuoy_ens_get(ens.ens, None, None) == LBM_ERR_ARG
        ens.set_buoyancy([BS[k] for k in range(case.n)], C_REFS)
        assert np.array_equal(ens.buoyancy(), b)
        assert lib.lbm_dscalar_ens_set(ens.ens, None, None, None, None) == LBM_ERR_STATE
        assert ens.scalar() is not None
        ens.run(1)
        assert lib.lbm_dbuoy_ens_set(ens.ens, None) == LBM_ERR_STATE
        assert lib.lbm_dbuoy_ens_set(ens.ens, ptr(b)) == LBM_ERR_STATE
        # a steady run stays refused while a scalar is on
        with pytest.raises(lbm.LBMError) as err:
            ens.run_until(4, window=2, rel_tol=1e-3)
        assert "gated scalar kernel" in str(err.value)
        assert ens.steps_done == 1 and np.array_equal(ens.buoyancy(), b)

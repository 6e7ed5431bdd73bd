"""The moving-wall entry points (lbm_dwall_*).

Without a device: header, binding and library agree on the four names and their argument types, the header holds the
statements that define the rule, NULL handles are refused, and so are one NULL component beside the other, a wall density
that is not finite and positive and four NULL outputs, before anything of the handle is read.

On the GPU (marked): every refusal that needs a handle - an entry that is not finite, a non-zero entry on a fluid cell (the
message names the cell, and the member), a bad rho_wall per member, LBM_ERR_STATE after a step.  After each refusal wall()
returns the previous setting and a step equals the previous setting's reference (tests/_dp_matrix.reference_step), bit for bit.  Set, get,
off round trip; upload and upload_obstacles keep the setting, and a velocity is read only while its cell is blocked."""
import ctypes
import os
import re

import numpy as np
import pytest

import _dp_matrix as dm
from conftest import ROOT

LBM_ERR_ARG, LBM_ERR_STATE = 1, 3

NAMES = ["lbm_dwall_ens_get", "lbm_dwall_ens_set", "lbm_dwall_get", "lbm_dwall_set"]


def header_text():
    return open(os.path.join(ROOT, "include", "lbm.h")).read()


def test_error_codes_are_the_headers():
    code = header_text()
    assert re.search(r"#define LBM_ERR_ARG %d\b" % LBM_ERR_ARG, code) and re.search(r"#define LBM_ERR_STATE %d\b" % LBM_ERR_STATE, code)


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm_dwall_[a-z_]+)\s*\(", code)))
    assert syms == NAMES
    assert sorted(s for s in lbm.ABI_SYMBOLS if s.startswith("lbm_dwall_")) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
    vp, dbl, ci = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    assert lib.lbm_dwall_set.argtypes == [vp, vp, vp, dbl]
    assert lib.lbm_dwall_get.argtypes == [vp, ctypes.POINTER(ci), vp, vp, ctypes.POINTER(dbl)]
    assert lib.lbm_dwall_ens_set.argtypes == [vp, vp, vp, vp]
    assert lib.lbm_dwall_ens_get.argtypes == [vp, ctypes.POINTER(ci), vp, vp, vp]
    # the header's prototypes, as the binding declares them
    for proto in ("int lbm_dwall_set(lbm_dp *d, const double *u_x , const double *u_y , double rho_wall);",
                  "int lbm_dwall_get(const lbm_dp *d, int *on_out, double *u_x_out, double *u_y_out, double *rho_wall_out);",
                  "int lbm_dwall_ens_set(lbm_dens *e, const double *u_x , const double *u_y, const double *rho_wall );",
                  "int lbm_dwall_ens_get(const lbm_dens *e, int *on_out, double *u_x_out, double *u_y_out, double *rho_wall_out );"):
        assert proto in code, proto
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in ("set_wall", "wall"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls in (lbm.LBM, lbm.Ensemble):                                      # fp32: out of scope, said in lbm.h
        assert not hasattr(cls, "set_wall") and not hasattr(cls, "wall"), cls.__name__


def test_the_definition_is_in_the_header():
    lines = [" ".join(l.lstrip(" *").split()) for l in header_text().splitlines()]
    text = "\n".join(lines)
    rule = ["rx = rho_wall * u_x; ry = rho_wall * u_y;",
            "a = (2.0 / 3.0) * rx; b = (2.0 / 3.0) * ry;",
            "p = (1.0 / 6.0) * (rx + ry); q = (1.0 / 6.0) * (ry - rx);",
            "out[0] = g[0];",
            "out[1] = g[3] + a; out[3] = g[1] - a;",
            "out[2] = g[4] + b; out[4] = g[2] - b;",
            "out[5] = g[7] + p; out[7] = g[5] - p;",
            "out[6] = g[8] + q; out[8] = g[6] - q;"]
    assert "\n".join(rule) in text                                               # the statements, consecutive and in order
    assert text.index("---- Open boundaries") < text.index("---- Moving walls")
    joined = " ".join(lines)
    for phrase in ("Off by default", "both compare equal to 0.0 is a resting wall", "signed zeros survive",
                   "one IEEE operation per written operator", "The cell still returns |u| = 0", "Nothing else moves: av_vels",
                   "the four fields", "the Reynolds number", "the force definition and the order of its sums",
                   "the body rules including the open-column rule", "accelerate_flow", "both steady criteria",
                   "adds or removes mass", "the caller's business", "Only while steps_done is 0", "keep the setting",
                   "read only while its cell is blocked", "after a refusal nothing has changed",
                   'It composes with "force", body maps, TRT and open boundaries', "Out of scope: fp32"):
        assert phrase in joined, phrase


def test_null_handles(lbm):
    lib = lbm.load_library()
    buf = (ctypes.c_double * 8)(*([0.01] * 8))
    rho = (ctypes.c_double * 2)(0.1, 0.1)
    on = ctypes.c_int(7)
    vb, vr = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(rho, ctypes.c_void_p)
    pr = ctypes.cast(rho, ctypes.POINTER(ctypes.c_double))
    calls = {"context": [lambda: lib.lbm_dwall_set(None, vb, vb, 0.1), lambda: lib.lbm_dwall_set(None, None, None, 0.0),
                         lambda: lib.lbm_dwall_get(None, ctypes.byref(on), vb, vb, pr)],
             "ensemble": [lambda: lib.lbm_dwall_ens_set(None, vb, vb, vr), lambda: lib.lbm_dwall_ens_set(None, None, None, None),
                          lambda: lib.lbm_dwall_ens_get(None, ctypes.byref(on), vb, vb, vr)]}
    for noun, group in calls.items():
        for call in group:
            assert call() == LBM_ERR_ARG
            msg = lib.lbm_last_error().decode()
            assert "NULL" in msg and noun in msg, msg
    assert on.value == 7 and list(buf) == [0.01] * 8 and list(rho) == [0.1, 0.1]


def test_bad_arguments_are_refused_before_the_handle_is_read(lbm):
    """The handle is a block of zero bytes, not a context: the refusal comes before anything of it is read, and without a
    device"""
    lib = lbm.load_library()
    fake = ctypes.create_string_buffer(0)
    h = ctypes.cast(fake, ctypes.c_void_p)
    u = (ctypes.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    vu = ctypes.cast(u, ctypes.c_void_p)
    for bad in (float("nan"), float("inf"), -float("inf"), -0.1, 0.0):
        assert lib.lbm_dwall_set(h, vu, vu, bad) == LBM_ERR_ARG, bad
        assert "rho_wall" in lib.lbm_last_error().decode()
    # exactly one component
    for call, tail in ((lib.lbm_dwall_set, (0.1,)), (lib.lbm_dwall_ens_set, (vu,))):
        for ux, uy, missing in ((vu, None, "u_y is NULL"), (None, vu, "u_x is NULL")):
            assert call(h, ux, uy, *tail) == LBM_ERR_ARG
            assert missing in lib.lbm_last_error().decode(), lib.lbm_last_error()
    assert lib.lbm_dwall_ens_set(h, vu, vu, None) == LBM_ERR_ARG
    assert "rho_wall is NULL" in lib.lbm_last_error().decode()
    for call in (lib.lbm_dwall_get, lib.lbm_dwall_ens_get):
        assert call(h, None, None, None, None) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "NULL" in msg and all(name in msg for name in ("on_out", "u_x_out", "u_y_out", "rho_wall_out")), msg


# ---- with a device ----------------------------------------------------------------------------------------------------------

NX, NY = 17, 16


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def wall_case(lbm, steps=8):
    """walls on rows 0 and NY - 1 and a block; every blocked cell moves but the bottom wall"""
    from _dp_states import random_state
    rng = np.random.default_rng(99)
    ob = np.zeros((NY, NX), dtype=np.int32)
    ob[0] = ob[NY - 1] = 1
    ob[6:9, 5:8] = 1
    p = lbm.make_dparams(NX, NY, steps, density=0.1, accel=0.005, omega=1.3, obstacles=ob)
    u_x = np.where(ob != 0, 0.1 * (rng.random((NY, NX)) - 0.5), 0.0)
    u_y = np.where(ob != 0, 0.1 * (rng.random((NY, NX)) - 0.5), 0.0)
    u_x[0] = u_y[0] = 0.0
    return p, ob, random_state(rng, 0.1, NY, NX), u_x, u_y


def ptr(a):
    return a.ctypes.data


def same_setting(got, u_x, u_y, rho):
    return got is not None and got[0].tobytes() == u_x.tobytes() and got[1].tobytes() == u_y.tobytes() and np.array_equal(got[2], rho)


@pytest.mark.gpu
def test_context_refusals_leave_the_setting(lbm, oracle_f64):
    lib = lbm.load_library()
    p, ob, cells0, u_x, u_y = wall_case(lbm)
    rho = 0.0985
    wall = (u_x, u_y, rho)
    want, _, _ = dm.reference_step(oracle_f64, p, ob, None, cells0, None, None, wall)
    plain, _, _ = dm.reference_step(oracle_f64, p, ob, None, cells0, None, None, None)
    assert not np.array_equal(want, plain)
    on = ctypes.c_int()
    with lbm.LBMDouble(p, ob) as sim:
        assert sim.wall() is None                                                 # off by default
        sim.upload(cells0)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], plain)
        assert lib.lbm_dwall_set(sim.ctx, ptr(u_x), ptr(u_y), rho) == LBM_ERR_STATE   # after a step
        assert b"first step" in lib.lbm_last_error()
        assert sim.wall() is None
        sim.upload(cells0)                                                        # accepted again
        sim.set_wall(u_x, u_y, rho)
        assert same_setting(sim.wall(), u_x, u_y, rho)

        def refused(ux, uy, r, *words):
            assert lib.lbm_dwall_set(sim.ctx, None if ux is None else ptr(ux), None if uy is None else ptr(uy), r) == LBM_ERR_ARG
            msg = lib.lbm_last_error().decode()
            assert all(w in msg for w in words), msg
            assert same_setting(sim.wall(), u_x, u_y, rho)                        # the previous setting, on the host ...
            sim.upload(cells0)
            sim.run(1)
            assert np.array_equal(sim.download(av_vels=False)[0], want), words    # ... and on the device
            sim.upload(cells0)

        half = 0.5 * u_x
        refused(half, None, rho, "u_y is NULL")
        refused(None, half, rho, "u_x is NULL")
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            refused(half, u_y, bad, "rho_wall")
        for (y, x), bad in (((NY - 1, 3), float("nan")), ((7, 6), float("inf")), ((0, 0), -float("inf"))):
            for which in (0, 1):
                maps = [half.copy(), u_y.copy()]
                maps[which][y, x] = bad
                refused(maps[0], maps[1], rho, "not finite", "y %d, x %d" % (y, x))
        for (y, x) in ((1, 0), (7, 4), (NY - 2, NX - 1)):
            assert ob[y, x] == 0
            for which in (0, 1):
                maps = [half.copy(), u_y.copy()]
                maps[which][y, x] = 1e-300
                refused(maps[0], maps[1], rho, "fluid cell", "y %d, x %d" % (y, x))
        assert lib.lbm_dwall_get(sim.ctx, None, None, None, None) == LBM_ERR_ARG
        assert lib.lbm_dwall_get(sim.ctx, ctypes.byref(on), None, None, None) == 0 and on.value == 1
        # -0.0 on a fluid cell compares equal to zero: accepted, and the step is the same
        signed = u_x.copy()
        signed[ob == 0] = -0.0
        sim.set_wall(signed, u_y, rho)
        assert same_setting(sim.wall(), signed, u_y, rho)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], want)
        assert lib.lbm_dwall_set(sim.ctx, None, None, 0.0) == LBM_ERR_STATE
        assert same_setting(sim.wall(), signed, u_y, rho)


@pytest.mark.gpu
def test_context_round_trip_and_what_keeps_the_setting(lbm, oracle_f64):
    p, ob, cells0, u_x, u_y = wall_case(lbm)
    plain, _, _ = dm.reference_step(oracle_f64, p, ob, None, cells0, None, None, None)
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_wall(u_x, u_y)                                                    # rho_wall None: the params' density
        assert same_setting(sim.wall(), u_x, u_y, p.density)
        sim.set_wall(None, None)                                                  # off
        assert sim.wall() is None
        sim.set_wall(None, None)                                                  # off while off
        sim.upload(cells0)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], plain)
        sim.upload(cells0)
        sim.set_wall(u_x, u_y, 0.102)
        want, _, _ = dm.reference_step(oracle_f64, p, ob, None, cells0, None, None, (u_x, u_y, 0.102))
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], want)
        sim.upload(cells0)                                                        # uploads keep the setting
        sim.upload_obstacles(ob)
        assert same_setting(sim.wall(), u_x, u_y, 0.102)
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], want)
        # another map: the block is gone, a new cell is blocked.  The block's velocities are no longer read, the new cell's
        # velocity is the zero it was given as a fluid cell, and get() returns what was set
        other = ob.copy()
        other[6:9, 5:8] = 0
        other[3, 12] = 1
        sim.upload(cells0)
        sim.upload_obstacles(other)
        assert same_setting(sim.wall(), u_x, u_y, 0.102)
        po = lbm.make_dparams(NX, NY, 8, density=0.1, accel=0.005, omega=1.3, obstacles=other)
        moved, _, _ = dm.reference_step(oracle_f64, po, other, None, cells0, None, None, (u_x, u_y, 0.102))
        sim.run(1)
        assert np.array_equal(sim.download(av_vels=False)[0], moved)


@pytest.mark.gpu
def test_ensemble_refusals_round_trip_and_uploads(lbm, oracle_f64):
    lib = lbm.load_library()
    p, ob, cells0, u_x, u_y = wall_case(lbm)
    n = 3
    params = lbm.sweep_dparams(p, omega=[1.2, 1.7, 1.0])
    ux = np.stack([u_x, 0.5 * u_x, -u_x])
    uy = np.stack([u_y, u_y, 0.25 * u_y])
    rhos = np.array([0.1, 0.102, 0.099])
    start = np.stack([cells0] * n)
    want = np.stack([dm.reference_step(oracle_f64, params[m], ob, None, cells0, None, None, (ux[m], uy[m], rhos[m]))[0]
                     for m in range(n)])
    with lbm.EnsembleDouble(params, ob) as ens:
        assert ens.wall() is None
        ens.set_wall(ux, uy, rhos)
        assert same_setting(ens.wall(), ux, uy, rhos)

        def refused(a, b, r, *words):
            args = [None if v is None else ptr(v) for v in (a, b, r)]
            assert lib.lbm_dwall_ens_set(ens.ens, *args) == LBM_ERR_ARG
            msg = lib.lbm_last_error().decode()
            assert all(w in msg for w in words), msg
            assert same_setting(ens.wall(), ux, uy, rhos)
            ens.upload(start)
            ens.run(1)
            assert np.array_equal(ens.download(av_vels=False)[0], want), words
            ens.upload(start)

        half = 0.5 * ux
        refused(half, None, rhos, "u_y is NULL")
        refused(None, half, rhos, "u_x is NULL")
        refused(half, uy, None, "rho_wall is NULL")
        for member, bad in ((1, 0.0), (2, float("nan")), (0, -1.0), (2, float("inf"))):
            r = rhos.copy()
            r[member] = bad
            refused(half, uy, r, "member %d" % member, "rho_wall")
        for member, (y, x), bad in ((1, (NY - 1, 3), float("nan")), (2, (7, 6), float("inf"))):
            a = half.copy()
            a[member, y, x] = bad
            refused(a, uy, rhos, "not finite", "member %d" % member, "y %d, x %d" % (y, x))
        for member, (y, x) in ((0, (1, 0)), (2, (NY - 2, NX - 1))):
            b = uy.copy()
            b[member, y, x] = -0.01
            refused(half, b, rhos, "fluid cell", "member %d" % member, "y %d, x %d" % (y, x))
        assert lib.lbm_dwall_ens_get(ens.ens, None, None, None, None) == LBM_ERR_ARG
        ens.run(2)
        cells = ens.download(av_vels=False)[0]
        assert lib.lbm_dwall_ens_set(ens.ens, None, None, None) == LBM_ERR_STATE
        assert lib.lbm_dwall_ens_set(ens.ens, ptr(ux), ptr(uy), ptr(rhos)) == LBM_ERR_STATE
        ens.upload(start)                                                         # keeps the setting
        assert same_setting(ens.wall(), ux, uy, rhos)
        ens.run(2)
        assert np.array_equal(ens.download(av_vels=False)[0], cells)
        # one map for all, rho_wall from the members' densities; one value for all; off
        ens.upload(start)
        ens.set_wall(u_x, u_y)
        assert same_setting(ens.wall(), np.stack([u_x] * n), np.stack([u_y] * n), np.array([q.density for q in params]))
        ens.set_wall(u_x, u_y, 0.2)
        assert np.array_equal(ens.wall()[2], [0.2] * n)
        ens.set_wall(None, None)
        assert ens.wall() is None
        ens.run(1)
        plain = np.stack([dm.reference_step(oracle_f64, params[m], ob, None, cells0, None, None, None)[0] for m in range(n)])
        assert np.array_equal(ens.download(av_vels=False)[0], plain)

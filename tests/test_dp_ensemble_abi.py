"""The double-precision ensemble entry points (lbm_dens_*) as far as they go without a device: exported symbols, the NULL
conventions, every argument error of lbm_dens_create (reported before a device is touched), and sweep_dparams."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = ["lbm_dens_create", "lbm_dens_upload", "lbm_dens_run", "lbm_dens_run_timed", "lbm_dens_sync", "lbm_dens_download",
         "lbm_dens_final_state", "lbm_dens_reynolds", "lbm_dens_steps_done", "lbm_dens_members", "lbm_dens_destroy"]


def dens_header_symbols():
    text = open(os.path.join(ROOT, "include", "lbm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lbm_dens_[a-z_]+)\s*\(", text)))


def test_library_exports_every_dp_ensemble_symbol(lbm):
    lib = lbm.load_library()
    syms = dens_header_symbols()
    assert syms == sorted(NAMES) and len(syms) == 11
    for s in syms:
        assert s in lbm.ABI_SYMBOLS and hasattr(lib, s), s


def test_null_dp_ensemble(lbm):
    lib = lbm.load_library()
    assert lib.lbm_dens_steps_done(None) == -1
    assert lib.lbm_dens_members(None) == -1
    assert lib.lbm_dens_run(None, 1) == LBM_ERR_ARG
    assert b"NULL" in lib.lbm_last_error()
    for call in (lambda: lib.lbm_dens_upload(None, None), lambda: lib.lbm_dens_sync(None),
                 lambda: lib.lbm_dens_download(None, None, None), lambda: lib.lbm_dens_reynolds(None, None),
                 lambda: lib.lbm_dens_final_state(None, None, None, None, None),
                 lambda: lib.lbm_dens_run_timed(None, 1, None)):
        assert call() == LBM_ERR_ARG and lib.lbm_last_error()
    lib.lbm_dens_destroy(None)  # a no-op, like lbm_destroy(NULL)


def members(lbm, n, nx=16, ny=16, max_iters=4, **kw):
    return (lbm.DParams * n)(*[lbm.make_dparams(nx, ny, max_iters, **dict({"omega": 1.0 + 0.1 * i}, **kw)) for i in range(n)])


def refused(lbm, params, obstacles, n, expect=None):
    """lbm_dens_create must answer LBM_ERR_ARG, leave a message and leave *out NULL"""
    lib = lbm.load_library()
    out = ctypes.c_void_p(0xdead)  # *out is written even on failure
    rc = lib.lbm_dens_create(ctypes.byref(out), params, obstacles.ctypes.data if obstacles is not None else None, n)
    msg = lib.lbm_last_error().decode()
    assert rc == LBM_ERR_ARG, (rc, msg)
    assert msg and not out.value
    if expect:
        assert expect in msg, msg
    return msg


def test_create_refuses_bad_arguments_without_a_device(lbm):
    lib = lbm.load_library()
    ob = np.zeros((2, 16, 16), dtype=np.int32)
    # member count
    refused(lbm, members(lbm, 2), ob, 0, "members")
    refused(lbm, members(lbm, 2), ob, -3, "members")
    refused(lbm, members(lbm, 2), ob, 65536, "members")
    # NULL pointers
    refused(lbm, None, ob, 2, "NULL")
    refused(lbm, members(lbm, 2), None, 2, "NULL")
    assert lib.lbm_dens_create(None, members(lbm, 2), ob.ctypes.data, 2) == LBM_ERR_ARG
    # members that differ in nx, ny or max_iters: the member is named
    p = members(lbm, 2)
    p[1].nx = 32
    refused(lbm, p, ob, 2, "member 1")
    p = members(lbm, 2)
    p[1].ny = 17
    refused(lbm, p, ob, 2, "member 1")
    p = members(lbm, 2)
    p[1].max_iters = 5
    assert "member 1" in refused(lbm, p, ob, 2, "max_iters")
    # a grid under 3x3
    for nx, ny in ((2, 16), (16, 2), (0, 0), (-5, 16), (3, 2)):
        refused(lbm, members(lbm, 1, nx, ny), ob, 1, "3x3")
    # max_iters under 1
    for it in (0, -1):
        refused(lbm, members(lbm, 2, max_iters=it), ob, 2, "max_iters")
    # a member's omega or density not finite and positive, accel not finite (lbm_dp_create's rules), in any member
    for bad in (0.0, -1.85, math.inf, -math.inf, math.nan):
        for k in (0, 1):
            p = members(lbm, 2)
            p[k].omega = bad
            assert "member %d" % k in refused(lbm, p, ob, 2, "omega")
            p = members(lbm, 2)
            p[k].density = bad
            assert "member %d" % k in refused(lbm, p, ob, 2, "density")
    for bad in (math.nan, math.inf, -math.inf):
        p = members(lbm, 2)
        p[1].accel = bad
        assert "member 1" in refused(lbm, p, ob, 2, "accel")


def test_create_refuses_members_above_the_lds_form_bound(lbm):
    # 2048 x 2048 is far above the 300 x 1024 cells up to which lbm_dp itself takes the LDS-tile form: the message sends the
    # caller to lbm_dp_*.  The obstacle pointer is never read (the refusal comes first), so one row stands in for the map
    msg = refused(lbm, members(lbm, 2, 2048, 2048), np.zeros((1, 2048), dtype=np.int32), 2, "lbm_dp_")
    assert "2048" in msg
    # the bound itself: 300 x 1024 cells are accepted as far as the arguments go (what follows needs a device)
    lib = lbm.load_library()
    out = ctypes.c_void_p()
    ob = np.zeros((1, 300, 1024), dtype=np.int32)
    rc = lib.lbm_dens_create(ctypes.byref(out), members(lbm, 1, 1024, 300), ob.ctypes.data, 1)
    if rc == 0:
        lib.lbm_dens_destroy(out)
    else:
        assert rc != LBM_ERR_ARG, lib.lbm_last_error()
    refused(lbm, members(lbm, 1, 1024, 301), np.zeros((1, 1024), dtype=np.int32), 1, "lbm_dp_")


def test_sweep_dparams_and_binding_checks(lbm):
    base = lbm.make_dparams(16, 16, 4, density=0.1)
    sweep = lbm.sweep_dparams(base, omega=[1.0, 1.5, 1.9], accel=[0.002, 0.004, 0.1])
    assert all(isinstance(p, lbm.DParams) for p in sweep)
    assert [p.omega for p in sweep] == [1.0, 1.5, 1.9]
    assert [p.accel for p in sweep] == [0.002, 0.004, 0.1]
    # 0.1 stays the fp64 literal, never a widened float
    assert sweep[2].accel == 0.1 and sweep[2].accel != float(np.float32(0.1))
    assert all(p.density == 0.1 and p.density != float(np.float32(0.1)) for p in sweep)
    assert all(p.nx == 16 and p.ny == 16 and p.max_iters == 4 and p.free_cells_inv == base.free_cells_inv for p in sweep)
    only_omega = lbm.sweep_dparams(base, omega=[1.1, 1.2])
    assert [p.omega for p in only_omega] == [1.1, 1.2] and all(p.accel == base.accel for p in only_omega)
    only_accel = lbm.sweep_dparams(base, accel=[0.001])
    assert only_accel[0].accel == 0.001 and only_accel[0].omega == base.omega
    sweep[0].omega = 1.2
    assert sweep[1].omega == 1.5 and base.omega == 1.85   # copies, not views
    with pytest.raises(lbm.LBMError):
        lbm.EnsembleDouble([], np.zeros((16, 16), dtype=np.int32))
    with pytest.raises(lbm.LBMError):   # fp32 Params are not silently converted
        lbm.EnsembleDouble([lbm.make_params(16, 16, 4)], np.zeros((16, 16), dtype=np.int32))


def test_dp_ensemble_has_no_cpu_fallback(lbm):
    """without a GPU a valid ensemble must fail loudly, never compute on the host; with one it is created on the device"""
    n = ctypes.c_int()
    hip = ctypes.CDLL("libamdhip64.so")
    gpu = hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0
    base = lbm.make_dparams(16, 16, 4)
    ob = np.zeros((16, 16), dtype=np.int32)
    if gpu:
        with lbm.EnsembleDouble(lbm.sweep_dparams(base, omega=[1.0, 1.5]), ob) as ens:
            assert ens.n == 2 and ens.steps_done == 0
        return
    with pytest.raises(lbm.LBMError) as e:
        lbm.EnsembleDouble(lbm.sweep_dparams(base, omega=[1.0, 1.5]), ob)
    assert "HIP" in str(e.value) or "device" in str(e.value)

"""The ensemble entry points (lbm_ens_*) as far as they go without a device: exported symbols, the NULL conventions and
every argument error of lbm_ens_create, which must be reported before a device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LBM_ERR_ARG = 1


def ens_header_symbols():
    text = open(os.path.join(ROOT, "include", "lbm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lbm_ens_[a-z_]+)\s*\(", text)))


def test_library_exports_every_ensemble_symbol(lbm):
    lib = lbm.load_library()
    syms = ens_header_symbols()
    assert syms == sorted(["lbm_ens_create", "lbm_ens_upload", "lbm_ens_run", "lbm_ens_run_timed", "lbm_ens_sync",
                           "lbm_ens_download", "lbm_ens_final_state", "lbm_ens_reynolds", "lbm_ens_steps_done",
                           "lbm_ens_members", "lbm_ens_destroy"])
    for s in syms:
        assert s in lbm.ABI_SYMBOLS and hasattr(lib, s), s


def test_null_ensemble(lbm):
    lib = lbm.load_library()
    assert lib.lbm_ens_steps_done(None) == -1
    assert lib.lbm_ens_members(None) == -1
    assert lib.lbm_ens_run(None, 1) == LBM_ERR_ARG
    assert b"NULL" in lib.lbm_last_error()
    for call in (lambda: lib.lbm_ens_upload(None, None), lambda: lib.lbm_ens_sync(None),
                 lambda: lib.lbm_ens_download(None, None, None), lambda: lib.lbm_ens_reynolds(None, None),
                 lambda: lib.lbm_ens_final_state(None, None, None, None, None),
                 lambda: lib.lbm_ens_run_timed(None, 1, None)):
        assert call() == LBM_ERR_ARG and lib.lbm_last_error()
    lib.lbm_ens_destroy(None)  # a no-op, like lbm_destroy(NULL)


def members(lbm, n, nx=16, ny=16, max_iters=4):
    return (lbm.Params * n)(*[lbm.make_params(nx, ny, max_iters, omega=1.0 + 0.1 * i) for i in range(n)])


def refused(lbm, params, obstacles, n, expect=None):
    """lbm_ens_create must answer LBM_ERR_ARG, leave a message and leave *out NULL"""
    lib = lbm.load_library()
    out = ctypes.c_void_p(0xdead)  # *out is written even on failure
    rc = lib.lbm_ens_create(ctypes.byref(out), params, obstacles.ctypes.data if obstacles is not None else None, n)
    msg = lib.lbm_last_error().decode()
    assert rc == LBM_ERR_ARG, (rc, msg)
    assert msg and not out.value
    if expect:
        assert expect in msg, msg
    return msg


def test_create_refuses_bad_arguments_without_a_device(lbm):
    lib = lbm.load_library()
    ob = np.zeros((2, 16, 16), dtype=np.int32)
    refused(lbm, members(lbm, 2), ob, 0)
    refused(lbm, members(lbm, 2), ob, -3)
    refused(lbm, members(lbm, 2), ob, 65536)
    refused(lbm, None, ob, 2, "NULL")
    refused(lbm, members(lbm, 2), None, 2, "NULL")
    assert lib.lbm_ens_create(None, members(lbm, 2), ob.ctypes.data, 2) == LBM_ERR_ARG
    p = members(lbm, 2)
    p[1].nx = 32
    refused(lbm, p, ob, 2, "member 1")
    p = members(lbm, 2)
    p[1].ny = 17
    refused(lbm, p, ob, 2, "member 1")
    p = members(lbm, 2)
    p[1].max_iters = 5
    refused(lbm, p, ob, 2, "max_iters")
    refused(lbm, members(lbm, 1, 2, 2), ob, 1)
    p = members(lbm, 1)
    p[0].max_iters = -1
    refused(lbm, p, ob, 1)


def test_create_refuses_members_that_are_not_launch_bound(lbm):
    # 2048 x 2048 is far above the 300 x 1024 cells up to which a grid is launch-bound: ordinary contexts serve it.  The
    # obstacle pointer is never read (the refusal comes first), so one row stands in for the map
    msg = refused(lbm, members(lbm, 2, 2048, 2048), np.zeros((1, 2048), dtype=np.int32), 2, "ordinary contexts")
    assert "2048" in msg
    # the bound itself: 300 x 1024 cells are accepted as far as the arguments go (what follows needs a device)
    lib = lbm.load_library()
    out = ctypes.c_void_p()
    ob = np.zeros((1, 300, 1024), dtype=np.int32)
    rc = lib.lbm_ens_create(ctypes.byref(out), members(lbm, 1, 1024, 300), ob.ctypes.data, 1)
    if rc == 0:
        lib.lbm_ens_destroy(out)
    else:
        assert rc != LBM_ERR_ARG, lib.lbm_last_error()
    refused(lbm, members(lbm, 1, 1024, 301), np.zeros((1, 1024), dtype=np.int32), 1, "ordinary contexts")


def test_sweep_params_and_binding_checks(lbm):
    base = lbm.make_params(16, 16, 4, density=0.11)
    sweep = lbm.sweep_params(base, omega=[1.0, 1.5, 1.9], accel=[0.002, 0.004, 0.01])
    assert [round(p.omega, 4) for p in sweep] == [1.0, 1.5, 1.9]
    assert [round(p.accel, 4) for p in sweep] == [0.002, 0.004, 0.01]
    assert all(p.nx == 16 and p.max_iters == 4 and p.density == base.density for p in sweep)
    sweep[0].omega = 1.2
    assert round(sweep[1].omega, 4) == 1.5 and round(base.omega, 4) == 1.85   # copies, not views
    with pytest.raises(lbm.LBMError):
        lbm.Ensemble([], np.zeros((16, 16), dtype=np.int32))


@pytest.mark.parametrize("sweep, make, ptype", [("sweep_params", "make_params", "Params"),
                                                ("sweep_dparams", "make_dparams", "DParams")])
def test_sweep_members_equal_members_built_field_by_field(lbm, sweep, make, ptype):
    """a swept member holds, byte for byte, what assigning its fields one by one to a fresh structure gives"""
    ob = np.zeros((16, 24), dtype=np.int32)
    ob[3, 5:9] = 1
    base = getattr(lbm, make)(24, 16, 7, reynolds_dim=3, density=0.11, accel=0.0051, omega=1.85, obstacles=ob)
    omega, accel = [1.0, 1.7, 0.1 + 0.2, 1.99], [0.002, 1e-3 / 3, 0.01, 0.0051]
    got = getattr(lbm, sweep)(base, omega=omega, accel=accel)
    assert len(got) == 4
    for i, g in enumerate(got):
        p = getattr(lbm, ptype)()
        p.nx, p.ny, p.max_iters, p.reynolds_dim = 24, 16, 7, 3
        p.density, p.free_cells_inv = base.density, base.free_cells_inv
        p.accel = accel[i]
        p.omega = omega[i]
        assert isinstance(g, getattr(lbm, ptype)) and bytes(g) == bytes(p), i


def test_ensemble_has_no_cpu_fallback(lbm):
    """without a GPU a valid ensemble must fail loudly, never compute on the host"""
    n = ctypes.c_int()
    hip = ctypes.CDLL("libamdhip64.so")
    if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    base = lbm.make_params(16, 16, 4)
    with pytest.raises(lbm.LBMError) as e:
        lbm.Ensemble(lbm.sweep_params(base, omega=[1.0, 1.5]), np.zeros((16, 16), dtype=np.int32))
    assert "HIP" in str(e.value) or "device" in str(e.value)

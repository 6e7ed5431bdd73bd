"""The double-precision entry points (lbm_dp_*) as far as they go without a device: exported symbols, the NULL conventions,
every argument error of lbm_dp_create (reported before a device is touched) and the binding's fp64 input parsing."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, input_files

LBM_ERR_ARG = 1

DP_SYMBOLS = ["lbm_dp_create", "lbm_dp_upload", "lbm_dp_upload_obstacles", "lbm_dp_run", "lbm_dp_run_timed", "lbm_dp_sync",
              "lbm_dp_download", "lbm_dp_final_state", "lbm_dp_reynolds", "lbm_dp_steps_done", "lbm_dp_set_option",
              "lbm_dp_get_option", "lbm_dp_destroy"]


def dp_header_symbols():
    text = open(os.path.join(ROOT, "include", "lbm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lbm_dp_[a-z_]+)\s*\(", text)))


def test_library_exports_every_dp_symbol(lbm):
    lib = lbm.load_library()
    assert dp_header_symbols() == sorted(DP_SYMBOLS)
    for s in DP_SYMBOLS:
        assert s in lbm.ABI_SYMBOLS and hasattr(lib, s), s


def test_dparams_layout(lbm):
    # four ints, then four doubles: 16 + 32 bytes, no padding
    assert ctypes.sizeof(lbm.DParams) == 48
    assert [f[0] for f in lbm.DParams._fields_] == [f[0] for f in lbm.Params._fields_]
    assert [f[1] for f in lbm.DParams._fields_][4:] == [ctypes.c_double] * 4


def test_null_dp_context(lbm):
    lib = lbm.load_library()
    assert lib.lbm_dp_steps_done(None) == -1
    assert lib.lbm_dp_run(None, 1) == LBM_ERR_ARG
    assert b"NULL" in lib.lbm_last_error()
    v = ctypes.c_long()
    for call in (lambda: lib.lbm_dp_upload(None, None), lambda: lib.lbm_dp_sync(None),
                 lambda: lib.lbm_dp_upload_obstacles(None, None),
                 lambda: lib.lbm_dp_download(None, None, None), lambda: lib.lbm_dp_reynolds(None, None),
                 lambda: lib.lbm_dp_final_state(None, None, None, None, None),
                 lambda: lib.lbm_dp_run_timed(None, 1, None),
                 lambda: lib.lbm_dp_set_option(None, b"multistep", 0),
                 lambda: lib.lbm_dp_get_option(None, b"multistep", ctypes.byref(v))):
        assert call() == LBM_ERR_ARG and lib.lbm_last_error()
    lib.lbm_dp_destroy(None)  # a no-op, like lbm_destroy(NULL)


def refused(lbm, params, obstacles, expect=None):
    """lbm_dp_create must answer LBM_ERR_ARG, leave a message and leave *out NULL"""
    lib = lbm.load_library()
    out = ctypes.c_void_p(0xdead)  # *out is written even on failure
    rc = lib.lbm_dp_create(ctypes.byref(out), ctypes.byref(params) if params is not None else None,
                           obstacles.ctypes.data if obstacles is not None else None)
    msg = lib.lbm_last_error().decode()
    assert rc == LBM_ERR_ARG, (rc, msg)
    assert msg and not out.value
    if expect:
        assert expect in msg, msg
    return msg


def test_create_refuses_bad_arguments_without_a_device(lbm):
    lib = lbm.load_library()
    ob = np.zeros((16, 16), dtype=np.int32)
    # NULL pointers
    refused(lbm, None, ob, "NULL")
    refused(lbm, lbm.make_dparams(16, 16, 4), None, "NULL")
    assert lib.lbm_dp_create(None, ctypes.byref(lbm.make_dparams(16, 16, 4)), ob.ctypes.data) == LBM_ERR_ARG
    # nx or ny below 3
    for nx, ny in ((2, 16), (16, 2), (0, 0), (-5, 16), (3, 2)):
        refused(lbm, lbm.make_dparams(nx, ny, 4), ob, "3x3")
    # max_iters below 1
    for it in (0, -1):
        refused(lbm, lbm.make_dparams(16, 16, it), ob, "max_iters")
    # omega or density non-finite or not positive
    for bad in (0.0, -1.85, math.inf, -math.inf, math.nan):
        refused(lbm, lbm.make_dparams(16, 16, 4, omega=bad), ob, "omega")
        refused(lbm, lbm.make_dparams(16, 16, 4, density=bad), ob, "density")
    refused(lbm, lbm.make_dparams(16, 16, 4, accel=math.nan), ob, "accel")


def test_binding_refuses_fp32_params(lbm):
    with pytest.raises(lbm.LBMError):
        lbm.LBMDouble(lbm.make_params(16, 16, 4), np.zeros((16, 16), dtype=np.int32))


def test_read_inputs_double_parses_the_fp64_literals(lbm):
    expect = {"128x128": 15876, "128x256": 32130, "256x256": 64516, "1024x1024": 1043462}
    for size, free in expect.items():
        p, ob = lbm.read_inputs_double(*input_files(size))
        assert isinstance(p, lbm.DParams)
        # the doubles nearest the file's decimal literals (0.1, 0.005, 1.85, ...), not widened floats
        tok = open(input_files(size)[0]).read().split()
        assert (p.density, p.accel, p.omega) == tuple(float(t) for t in tok[4:7])
        assert p.density == 0.1 and p.density != float(np.float32(0.1))
        assert int(ob.size - ob.sum()) == free
        assert p.free_cells_inv == 1.0 / free
        q, ob32 = lbm.read_inputs(*input_files(size))
        assert (p.nx, p.ny, p.max_iters, p.reynolds_dim) == (q.nx, q.ny, q.max_iters, q.reynolds_dim)
        assert np.array_equal(ob, ob32)
    p = lbm.make_dparams(4, 4, 1, obstacles=np.ones((4, 4), dtype=np.int32))
    assert p.free_cells_inv == math.inf


def test_dp_context_has_no_cpu_fallback(lbm):
    """without a GPU a valid double-precision context must fail loudly, never compute on the host"""
    n = ctypes.c_int()
    hip = ctypes.CDLL("libamdhip64.so")
    if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(lbm.LBMError) as e:
        lbm.LBMDouble(lbm.make_dparams(16, 16, 4), np.zeros((16, 16), dtype=np.int32))
    assert "HIP" in str(e.value) or "device" in str(e.value)

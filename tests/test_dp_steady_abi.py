"""The steady-run entry points of the double-precision ensembles (lbm_dsteady_*) as far as they go without a device:
exported symbols, the NULL convention and every argument refusal of lbm_dsteady_run, which must come before the ensemble is
dereferenced or a device is touched."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

LBM_ERR_ARG = 1


def dsteady_header_symbols():
    text = open(os.path.join(ROOT, "include", "lbm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lbm_dsteady_[a-z_]+)\s*\(", text)))


def test_library_exports_every_dp_steady_symbol(lbm):
    lib = lbm.load_library()
    syms = dsteady_header_symbols()
    assert syms == ["lbm_dsteady_run", "lbm_dsteady_steps"]
    for s in syms:
        assert s in lbm.ABI_SYMBOLS and hasattr(lib, s), s
    # a prefix of its own: the pinned lists of lbm_steady_, lbm_dens_, lbm_dp_ and lbm_ens_ names are not touched
    assert not any(s.startswith(("lbm_steady_", "lbm_dens_", "lbm_dp_", "lbm_ens_")) for s in syms)
    assert lib.lbm_dsteady_run.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double]
    assert lib.lbm_dsteady_steps.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(lbm.EnsembleDouble, "run_until") and hasattr(lbm.EnsembleDouble, "member_steps")
    # the fp32 ensemble keeps its own, on its own entry points
    assert hasattr(lbm.Ensemble, "run_until") and hasattr(lbm.Ensemble, "member_steps")
    assert lbm.Ensemble._steady == "lbm_steady" and lbm.EnsembleDouble._steady == "lbm_dsteady"


def test_null_dp_ensemble(lbm):
    lib = lbm.load_library()
    assert lib.lbm_dsteady_run(None, 10, 2, 1e-3) == LBM_ERR_ARG
    assert b"NULL" in lib.lbm_last_error()
    steps = np.zeros(4, dtype=np.int32)
    assert lib.lbm_dsteady_steps(None, steps.ctypes.data, None) == LBM_ERR_ARG
    assert b"NULL" in lib.lbm_last_error()
    assert lib.lbm_dsteady_steps(None, None, None) == LBM_ERR_ARG
    assert not steps.any()


def test_run_refuses_bad_arguments_before_it_reads_the_ensemble(lbm):
    """the ensemble pointer is the address of a page of 0xff bytes, no lbm_dens: an entry point that read it before it
    validated would take garbage for its fields (a member count of -1, a wild stream) instead of answering LBM_ERR_ARG"""
    lib = lbm.load_library()
    fake = ctypes.create_string_buffer(b"\xff" * 4096, 4096)
    e = ctypes.cast(fake, ctypes.c_void_p)
    for args, word in (((-1, 4, 1e-3), "max_steps"), ((-400, 4, 1e-3), "max_steps"),
                       ((10, 0, 1e-3), "window"), ((10, -7, 1e-3), "window"),
                       ((10, 4, -1e-9), "rel_tol"), ((10, 4, -1.0), "rel_tol"),
                       ((10, 4, float("nan")), "rel_tol"), ((10, 4, float("inf")), "rel_tol"),
                       ((10, 4, float("-inf")), "rel_tol"),
                       # several at once, and with max_steps == 0 (a no-op only for valid arguments)
                       ((-1, 0, float("nan")), "max_steps"), ((0, 0, 1e-3), "window"), ((0, 4, float("nan")), "rel_tol")):
        rc = lib.lbm_dsteady_run(e, *args)
        msg = lib.lbm_last_error().decode()
        assert rc == LBM_ERR_ARG, (args, rc, msg)
        assert word in msg, (args, msg)
    assert fake.raw == b"\xff" * 4096

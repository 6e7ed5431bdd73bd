"""The force entry points (lbm_dforce_*, option "force") as far as they go without a device: header, binding and library
agree on the six names, NULL handles and NULL-both-outputs are refused with LBM_ERR_ARG and a message that names the
argument, before anything is dereferenced."""
import ctypes
import os
import re

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = ["lbm_dforce", "lbm_dforce_ens", "lbm_dforce_ens_get_option", "lbm_dforce_ens_record", "lbm_dforce_ens_set_option",
         "lbm_dforce_record"]


def header_text():
    text = open(os.path.join(ROOT, "include", "lbm.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    syms = sorted(set(re.findall(r"\b(lbm_dforce[a-z_]*)\s*\(", header_text())))
    assert syms == sorted(NAMES)
    for s in syms:
        assert s in lbm.ABI_SYMBOLS and hasattr(lib, s), s
    vp, cp = ctypes.c_void_p, ctypes.c_char_p
    assert lib.lbm_dforce_record.argtypes == [vp, vp, vp]
    assert lib.lbm_dforce_ens_record.argtypes == [vp, vp, vp] and lib.lbm_dforce_ens.argtypes == [vp, vp, vp]
    assert lib.lbm_dforce_ens_set_option.argtypes == [vp, cp, ctypes.c_long]
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in ("set_option", "get_option", "force", "force_record"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
    assert not hasattr(lbm.Ensemble, "force") and not hasattr(lbm.LBM, "force")     # fp32: out of scope, said in lbm.h


def test_the_contract_is_in_the_header():
    text = open(os.path.join(ROOT, "include", "lbm.h")).read()
    for phrase in ("s = f_k(x) + f_opp(k)(o)", "AFTER accelerate_flow", "between two blocked cells do not count",
                   "exactly +0.0", "Out of scope: fp32"):
        assert phrase in text, phrase
    assert "No options" not in text          # an lbm_dens has one now


def test_null_handles(lbm):
    lib = lbm.load_library()
    out = (ctypes.c_double * 4)()
    v = ctypes.c_long()
    p = ctypes.cast(out, ctypes.c_void_p)
    d1, d2 = ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_double())
    calls = {"context": [lambda: lib.lbm_dforce_record(None, p, p), lambda: lib.lbm_dforce(None, d1, d2)],
             "ensemble": [lambda: lib.lbm_dforce_ens_record(None, p, p), lambda: lib.lbm_dforce_ens(None, p, p),
                          lambda: lib.lbm_dforce_ens_set_option(None, b"force", 1),
                          lambda: lib.lbm_dforce_ens_get_option(None, b"force", ctypes.byref(v))]}
    for noun, group in calls.items():
        for call in group:
            assert call() == LBM_ERR_ARG
            msg = lib.lbm_last_error().decode()
            assert "NULL" in msg and noun in msg, msg
    assert lib.lbm_dp_set_option(None, b"force", 1) == LBM_ERR_ARG
    assert lib.lbm_dp_get_option(None, b"force", ctypes.byref(v)) == LBM_ERR_ARG


def test_null_outputs_are_refused_before_the_handle_is_read(lbm):
    """both outputs NULL: LBM_ERR_ARG with the arguments' names.  The handle is a block of zero bytes, not a context: the
    refusal comes before anything of it is read, and without a device"""
    lib = lbm.load_library()
    fake = ctypes.create_string_buffer(4096)
    for call, names in ((lib.lbm_dforce_record, ("fx_out", "fy_out")), (lib.lbm_dforce, ("fx", "fy")),
                        (lib.lbm_dforce_ens_record, ("fx_out", "fy_out")), (lib.lbm_dforce_ens, ("fx", "fy"))):
        assert call(ctypes.cast(fake, ctypes.c_void_p), None, None) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "NULL" in msg and all(n in msg for n in names), msg
    h = ctypes.cast(fake, ctypes.c_void_p)
    assert lib.lbm_dforce_ens_set_option(h, None, 1) == LBM_ERR_ARG and b"key" in lib.lbm_last_error()
    assert lib.lbm_dforce_ens_get_option(h, None, None) == LBM_ERR_ARG and b"key" in lib.lbm_last_error()
    assert lib.lbm_dforce_ens_get_option(h, b"force", None) == LBM_ERR_ARG and b"value" in lib.lbm_last_error()

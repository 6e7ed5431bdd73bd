"""The buoyancy entry points (lbm_dbuoy_*) as far as they go without a device: header, binding and library agree on the four names and
their argument types, the header holds the statement block that defines the force, consecutive and in order, its section follows
"Scalar transport", NULL handles are refused, and non-finite values and all-NULL outputs are refused before anything of the handle
is read.  The fp32 classes have no set_buoyancy.  What needs a handle that exists is in tests/test_buoy_gpu.py (errors and what
keeps the setting).  This module fails on a library without the feature."""
import ctypes
import os
import re

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = sorted("lbm_dbuoy_" + e + s for e in ("", "ens_") for s in ("set", "get"))
METHODS = ("set_buoyancy", "buoyancy")


def header_text():
    return open(os.path.join(ROOT, "include", "lbm.h")).read()


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    code = " ".join(re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S).split())
    syms = sorted(set(re.findall(r"\b(lbm_dbuoy_[a-z_]+)\s*\(", code)))
    assert syms == NAMES and len(NAMES) == 4
    assert sorted(s for s in lbm.ABI_SYMBOLS if s.startswith("lbm_dbuoy_")) == NAMES
    assert not any(s.startswith("lbm_dscalar_") for s in NAMES)                # tests/test_scalar_abi.py pins those ten
    for s in syms:
        assert hasattr(lib, s), s
    vp, dbl, pi, pd = ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    assert lib.lbm_dbuoy_set.argtypes == [vp, dbl, dbl, dbl]
    assert lib.lbm_dbuoy_get.argtypes == [vp, pi, vp, pd]
    assert lib.lbm_dbuoy_ens_set.argtypes == [vp, vp]
    assert lib.lbm_dbuoy_ens_get.argtypes == [vp, pi, vp]
    for proto in ("int lbm_dbuoy_set(lbm_dp *d, double b_x, double b_y, double c_ref);",
                  "int lbm_dbuoy_get(const lbm_dp *d, int *on_out, double *b_out , double *c_ref_out);",
                  "int lbm_dbuoy_ens_set(lbm_dens *e, const double *b );",
                  "int lbm_dbuoy_ens_get(const lbm_dens *e, int *on_out, double *b_out );"):
        assert proto in code, proto
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in METHODS:
            assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls in (lbm.LBM, lbm.Ensemble):                                        # fp32: gets nothing, said in lbm.h
        assert not any(hasattr(cls, method) for method in METHODS), cls.__name__


def test_the_definition_is_in_the_header():
    lines = [" ".join(l.lstrip(" *").split()) for l in header_text().splitlines()]
    text = "\n".join(lines)
    block = ["C = (((g[0] + g[1]) + g[2]) + g[3]) + g[4];",
             "d = C - c_ref;",
             "F_x = F0_x + b_x * d;",
             "F_y = F0_y + b_y * d;"]
    assert "\n".join(block) in text                                            # the statements, consecutive and in order
    at = text.index("\n".join(block))
    order = ["---- Body force", "---- Scalar transport", "---- Buoyancy"]
    where = [text.index(s) for s in order]
    assert where == sorted(where)
    assert text.index("lbm_dscalar_ens_upload(") < text.index("---- Buoyancy") < at < text.index("lbm_dbuoy_set(")
    joined = " ".join(lines)
    for phrase in ("five STORED scalar values", "(0.0, 0.0) while that is off", "NOT multiplied by the cell's density",
                   "Ra = (|b| dC / rho0) H^3 / (nu kappa)", "contraction off", "one IEEE operation per written operator",
                   "Blocked cells take no force", "Scalar step n still runs before flow step n",
                   "the scalar array that scalar step n has just written", "less half of this F",
                   "per cell, from the two momentum sums", "This section lifts those two remarks",
                   "ONE kernel form, and the option \"multistep\" chooses nothing", "Only with a scalar on",
                   "only while steps_done is 0", "the twin rule of lbm_ddrive_ens_set",
                   "Switching the scalar off while buoyancy is on is LBM_ERR_STATE", "Everything is checked before anything changes",
                   "Steady runs stay refused while a scalar is on", "Out of scope: fp32"):
        assert phrase in joined, phrase
    # the sections before it keep their words (tests/test_scalar_abi.py, tests/test_drive_abi.py pin more of them)
    for phrase in ("PASSIVE", "a scalar that acts back on the flow (buoyancy)", "a force proportional to the local density"):
        assert phrase in joined[:joined.index("---- Buoyancy")], phrase


def test_null_handles(lbm):
    lib = lbm.load_library()
    buf = (ctypes.c_double * 8)(*([7.0] * 8))
    vb = ctypes.cast(buf, ctypes.c_void_p)
    pd = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))
    on = ctypes.c_int(7)
    calls = {"context": [lambda: lib.lbm_dbuoy_set(None, 0.0, 1e-5, 0.5), lambda: lib.lbm_dbuoy_set(None, 0.0, 0.0, 0.0),
                         lambda: lib.lbm_dbuoy_get(None, ctypes.byref(on), vb, pd)],
             "ensemble": [lambda: lib.lbm_dbuoy_ens_set(None, vb), lambda: lib.lbm_dbuoy_ens_set(None, None),
                          lambda: lib.lbm_dbuoy_ens_get(None, ctypes.byref(on), vb)]}
    for noun, group in calls.items():
        for call in group:
            assert call() == LBM_ERR_ARG
            msg = lib.lbm_last_error().decode()
            assert "NULL" in msg and noun in msg, msg
    assert list(buf) == [7.0] * 8 and on.value == 7


def test_bad_arguments_are_refused_before_the_handle_is_read(lbm):
    """The handle is a block of zero bytes, not a context: the refusal comes before anything of it is read, and without a
    device"""
    lib = lbm.load_library()
    fake = ctypes.create_string_buffer(0)
    h = ctypes.cast(fake, ctypes.c_void_p)
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 1e-5, 0.5), (1e-5, nan, 0.5), (0.0, 1e-5, nan), (inf, 0.0, 0.0), (0.0, -inf, 0.0), (0.0, 1e-5, inf), (0.0, 0.0, nan)):
        assert lib.lbm_dbuoy_set(h, *bad) == LBM_ERR_ARG, bad
        assert "buoyancy must be finite" in lib.lbm_last_error().decode()
    for get, names in ((lib.lbm_dbuoy_get, (None, None, None)), (lib.lbm_dbuoy_ens_get, (None, None))):
        assert get(h, *names) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "NULL" in msg and "on_out" in msg and "b_out" in msg, msg

"""The two-relaxation-time entry points (lbm_dtrt_*) as far as they go without a device: header, binding and library agree on
the four names and their argument types, the header holds the two statement blocks that define the operator, NULL handles
are refused, a magic parameter that is negative, NaN or infinite is refused before anything of the handle is read, and so
are two NULL outputs."""
import ctypes
import os
import re

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = ["lbm_dtrt_ens_get", "lbm_dtrt_ens_set", "lbm_dtrt_get", "lbm_dtrt_set"]


def header_text():
    return open(os.path.join(ROOT, "include", "lbm.h")).read()


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm_dtrt_[a-z_]+)\s*\(", code)))
    assert syms == NAMES
    assert sorted(s for s in lbm.ABI_SYMBOLS if s.startswith("lbm_dtrt_")) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
    vp, dbl = ctypes.c_void_p, ctypes.c_double
    assert lib.lbm_dtrt_set.argtypes == [vp, dbl]
    assert lib.lbm_dtrt_get.argtypes == [vp, ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
    assert lib.lbm_dtrt_ens_set.argtypes == [vp, vp]
    assert lib.lbm_dtrt_ens_get.argtypes == [vp, vp, vp]
    # the header's prototypes, as the binding declares them
    for proto in ("int lbm_dtrt_set(lbm_dp *d, double magic);",
                  "int lbm_dtrt_get(const lbm_dp *d, double *magic_out, double *omega_minus_out);",
                  "int lbm_dtrt_ens_set(lbm_dens *e, const double *magic );",
                  "int lbm_dtrt_ens_get(const lbm_dens *e, double *magic_out , double *omega_minus_out );"):
        assert proto in code, proto
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in ("set_trt", "trt"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls in (lbm.LBM, lbm.Ensemble):                                      # fp32: out of scope, said in lbm.h
        assert not hasattr(cls, "set_trt") and not hasattr(cls, "trt"), cls.__name__


def test_the_definition_is_in_the_header():
    lines = [" ".join(l.lstrip(" *").split()) for l in header_text().splitlines()]
    text = "\n".join(lines)
    host = ["tp = 1.0 / omega - 0.5;", "tm = magic / tp + 0.5;", "omega_m = 1.0 / tm;"]
    cell = ["out[0] = g[0] + omega * (eq[0] - g[0]);",
            "for (k, q) in (1,3), (2,4), (5,7), (6,8):",
            "a = eq[k] - g[k]; b = eq[q] - g[q];",
            "sp = 0.5 * (a + b); sm = 0.5 * (a - b);",
            "rp = omega * sp; rm = omega_m * sm;",
            "out[k] = g[k] + (rp + rm);",
            "out[q] = g[q] + (rp - rm);"]
    for block in (host, cell):
        assert "\n".join(block) in text, block                                 # the statements, consecutive and in order
    assert text.index("---- Drag of a body") < text.index("---- Two relaxation times")
    joined = " ".join(lines)
    for phrase in ("Lambda = (1/omega - 1/2) (1/omega_m - 1/2)", "Off by default", "Only while steps_done is 0",
                   "keep the setting", "all members TRT", "all BGK", "viscosity still comes from omega",
                   "Out of scope: fp32"):
        assert phrase in joined, phrase


def test_null_handles(lbm):
    lib = lbm.load_library()
    out = (ctypes.c_double * 4)()
    magic = (ctypes.c_double * 4)(0.25, 0.25, 0.25, 0.25)
    po = ctypes.cast(out, ctypes.POINTER(ctypes.c_double))
    vo, vm = ctypes.cast(out, ctypes.c_void_p), ctypes.cast(magic, ctypes.c_void_p)
    calls = {"context": [lambda: lib.lbm_dtrt_set(None, 0.25), lambda: lib.lbm_dtrt_set(None, 0.0),
                         lambda: lib.lbm_dtrt_get(None, po, po)],
             "ensemble": [lambda: lib.lbm_dtrt_ens_set(None, vm), lambda: lib.lbm_dtrt_ens_set(None, None),
                          lambda: lib.lbm_dtrt_ens_get(None, vo, vo)]}
    for noun, group in calls.items():
        for call in group:
            assert call() == LBM_ERR_ARG
            msg = lib.lbm_last_error().decode()
            assert "NULL" in msg and noun in msg, msg


def test_bad_arguments_are_refused_before_the_handle_is_read(lbm):
    """The handle is a block of zero bytes, not a context: the refusal comes before anything of it is read, and without a
    device"""
    lib = lbm.load_library()
    fake = ctypes.create_string_buffer(0)
    h = ctypes.cast(fake, ctypes.c_void_p)
    for bad in (float("nan"), float("inf"), -float("inf"), -0.25, -1e-300):
        assert lib.lbm_dtrt_set(h, bad) == LBM_ERR_ARG, bad
        assert "magic" in lib.lbm_last_error().decode()
    for call in (lib.lbm_dtrt_get, lib.lbm_dtrt_ens_get):
        assert call(h, None, None) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "NULL" in msg and "magic_out" in msg and "omega_minus_out" in msg, msg

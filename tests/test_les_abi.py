"""The subgrid-viscosity entry points (lbm_dles_*) as far as they go without a device: header, binding and library agree on the
four names and their argument types, the header holds the two statement blocks that define the model, consecutive and in order,
its section follows "Moving walls", NULL handles are refused, a Smagorinsky constant that is negative, NaN or infinite is refused
before anything of the handle is read, and so are two NULL outputs.  The fp32 classes have no set_les."""
import ctypes
import os
import re

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = ["lbm_dles_ens_get", "lbm_dles_ens_set", "lbm_dles_get", "lbm_dles_set"]


def header_text():
    return open(os.path.join(ROOT, "include", "lbm.h")).read()


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm_dles_[a-z_]+)\s*\(", code)))
    assert syms == NAMES
    assert sorted(s for s in lbm.ABI_SYMBOLS if s.startswith("lbm_dles_")) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
    vp, dbl = ctypes.c_void_p, ctypes.c_double
    assert lib.lbm_dles_set.argtypes == [vp, dbl]
    assert lib.lbm_dles_get.argtypes == [vp, ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
    assert lib.lbm_dles_ens_set.argtypes == [vp, vp]
    assert lib.lbm_dles_ens_get.argtypes == [vp, vp, vp]
    # the header's prototypes, as the binding declares them
    for proto in ("int lbm_dles_set(lbm_dp *d, double c);",
                  "int lbm_dles_get(const lbm_dp *d, double *c_out, double *les_k_out);",
                  "int lbm_dles_ens_set(lbm_dens *e, const double *c );",
                  "int lbm_dles_ens_get(const lbm_dens *e, double *c_out , double *les_k_out );"):
        assert proto in code, proto
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in ("set_les", "les"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls in (lbm.LBM, lbm.Ensemble):                                      # fp32: gets nothing, said in lbm.h
        assert not hasattr(cls, "set_les") and not hasattr(cls, "les"), cls.__name__


def test_the_definition_is_in_the_header():
    lines = [" ".join(l.lstrip(" *").split()) for l in header_text().splitlines()]
    text = "\n".join(lines)
    host = ["tau0 = 1.0 / omega;", "les_k = (18.0 * sqrt(2.0)) * (c * c);"]
    cell = ["d57 = g[5] + g[7]; d68 = g[6] + g[8]; dgs = d57 + d68;",
            "p = dens * (1.0 / 3.0);",
            "pxx = ((g[1] + g[3]) + dgs) - (p + (u_x * u_x) * densinv);",
            "pyy = ((g[2] + g[4]) + dgs) - (p + (u_y * u_y) * densinv);",
            "pxy = (d57 - d68) - (u_x * u_y) * densinv;",
            "q = sqrt((pxx * pxx + pyy * pyy) + 2.0 * (pxy * pxy));",
            "tau = 0.5 * (tau0 + sqrt(tau0 * tau0 + les_k * (q * densinv)));",
            "om = 1.0 / tau;"]
    second = ["tp = tau - 0.5;", "tm = magic / tp + 0.5;", "omega_m = 1.0 / tm;"]
    for block in (host, cell, second):
        assert "\n".join(block) in text, block                                 # the statements, consecutive and in order
    assert text.index("\n".join(host)) < text.index("\n".join(cell)) < text.index("\n".join(second))
    # the section order: the new section is the last one, behind "Moving walls"
    order = ["---- Two relaxation times", "---- Open boundaries", "---- Moving walls", "---- Subgrid viscosity"]
    at = [text.index(s) for s in order]
    assert at == sorted(at)
    assert text.index("---- Subgrid viscosity") < text.index("\n".join(host))
    assert text.index("lbm_dwall_ens_get(") < text.index("---- Subgrid viscosity") < text.index("lbm_dles_set(")
    joined = " ".join(lines)
    for phrase in ("Off by default", "sqrt(2.0) is the correctly rounded double", "c_s^2 = 1/3", "contraction off",
                   "one IEEE operation per written operator", "BGK: the relaxation lines read om where they read omega",
                   "rp = om * sp", "out[0] uses om", "tp = tau - 0.5 in place of 1.0 / omega - 0.5",
                   "om = 1.0 / (1.0 / omega)", "promised BGK's bits nowhere", "Nothing else moves: accelerate_flow",
                   "bounce-back and moving walls", "the force and its body maps", "the order of every sum", "the four fields",
                   "viscosity stays the molecular one from omega", "both steady runs", "Only while steps_done is 0",
                   "keep the setting", "set in either order", "after a refusal nothing has changed", "Out of scope: fp32"):
        assert phrase in joined, phrase


def test_null_handles(lbm):
    lib = lbm.load_library()
    out = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    c = (ctypes.c_double * 4)(0.17, 0.17, 0.17, 0.17)
    po = ctypes.cast(out, ctypes.POINTER(ctypes.c_double))
    vo, vc = ctypes.cast(out, ctypes.c_void_p), ctypes.cast(c, ctypes.c_void_p)
    calls = {"context": [lambda: lib.lbm_dles_set(None, 0.17), lambda: lib.lbm_dles_set(None, 0.0),
                         lambda: lib.lbm_dles_get(None, po, po)],
             "ensemble": [lambda: lib.lbm_dles_ens_set(None, vc), lambda: lib.lbm_dles_ens_set(None, None),
                          lambda: lib.lbm_dles_ens_get(None, vo, vo)]}
    for noun, group in calls.items():
        for call in group:
            assert call() == LBM_ERR_ARG
            msg = lib.lbm_last_error().decode()
            assert "NULL" in msg and noun in msg, msg
    assert list(out) == [7.0] * 4 and list(c) == [0.17] * 4


def test_bad_arguments_are_refused_before_the_handle_is_read(lbm):
    """The handle is a block of zero bytes, not a context: the refusal comes before anything of it is read, and without a
    device"""
    lib = lbm.load_library()
    fake = ctypes.create_string_buffer(0)
    h = ctypes.cast(fake, ctypes.c_void_p)
    for bad in (float("nan"), float("inf"), -float("inf"), -0.17, -1e-300):
        assert lib.lbm_dles_set(h, bad) == LBM_ERR_ARG, bad
        assert "Smagorinsky constant" in lib.lbm_last_error().decode()
    for call in (lib.lbm_dles_get, lib.lbm_dles_ens_get):
        assert call(h, None, None) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "NULL" in msg and "c_out" in msg and "les_k_out" in msg, msg

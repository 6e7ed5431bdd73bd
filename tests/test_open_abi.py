"""The open-boundary entry points (lbm_dopen_*) as far as they go without a device: header, binding and library agree on the
four names and their argument types, the header holds the two statement blocks that define the boundary fix, NULL handles
are refused, and so are an outlet density that is not finite and positive, before anything of the handle is read, and
three NULL outputs."""
import ctypes
import os
import re

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = ["lbm_dopen_ens_get", "lbm_dopen_ens_set", "lbm_dopen_get", "lbm_dopen_set"]


def header_text():
    return open(os.path.join(ROOT, "include", "lbm.h")).read()


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm_dopen_[a-z_]+)\s*\(", code)))
    assert syms == NAMES
    assert sorted(s for s in lbm.ABI_SYMBOLS if s.startswith("lbm_dopen_")) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
    vp, dbl, ci = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
    assert lib.lbm_dopen_set.argtypes == [vp, vp, dbl]
    assert lib.lbm_dopen_get.argtypes == [vp, ctypes.POINTER(ci), vp, ctypes.POINTER(dbl)]
    assert lib.lbm_dopen_ens_set.argtypes == [vp, vp, vp]
    assert lib.lbm_dopen_ens_get.argtypes == [vp, ctypes.POINTER(ci), vp, vp]
    # the header's prototypes, as the binding declares them
    for proto in ("int lbm_dopen_set(lbm_dp *d, const double *u_in , double rho_out);",
                  "int lbm_dopen_get(const lbm_dp *d, int *on_out, double *u_in_out , double *rho_out_out);",
                  "int lbm_dopen_ens_set(lbm_dens *e, const double *u_in , const double *rho_out );",
                  "int lbm_dopen_ens_get(const lbm_dens *e, int *on_out, double *u_in_out , double *rho_out_out );"):
        assert proto in code, proto
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in ("set_open", "open"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls in (lbm.LBM, lbm.Ensemble):                                      # fp32: out of scope, said in lbm.h
        assert not hasattr(cls, "set_open") and not hasattr(cls, "open"), cls.__name__


def test_the_definition_is_in_the_header():
    lines = [" ".join(l.lstrip(" *").split()) for l in header_text().splitlines()]
    text = "\n".join(lines)
    inlet = ["s0 = (g[0] + g[2]) + g[4]; s1 = (g[3] + g[6]) + g[7];",
             "rho = (s0 + 2.0 * s1) / (1.0 - u);",
             "ru = rho * u; d = 0.5 * (g[2] - g[4]);",
             "g[1] = g[3] + (2.0 / 3.0) * ru;",
             "g[5] = (g[7] - d) + (1.0 / 6.0) * ru;",
             "g[8] = (g[6] + d) + (1.0 / 6.0) * ru;"]
    outlet = ["s0 = (g[0] + g[2]) + g[4]; s1 = (g[1] + g[5]) + g[8];",
              "ru = (s0 + 2.0 * s1) - rho_out; d = 0.5 * (g[2] - g[4]);",
              "g[3] = g[1] - (2.0 / 3.0) * ru;",
              "g[7] = (g[5] + d) - (1.0 / 6.0) * ru;",
              "g[6] = (g[8] - d) - (1.0 / 6.0) * ru;"]
    for block in (inlet, outlet):
        assert "\n".join(block) in text, block                                 # the statements, consecutive and in order
    assert text.index("---- Two relaxation times") < text.index("---- Open boundaries")
    assert text.index("Inlet, x == 0, fluid, u = u_in[y]:") < text.index("Outlet, x == nx - 1, fluid, rho_out:")
    joined = " ".join(lines)
    for phrase in ("Off by default", "gather, boundary fix, collision", "No accelerate_flow", "Blocked cells are untouched",
                   "count as outside every body", "Only while steps_done is 0", "keep the setting",
                   "all open or all periodic", "After a refusal nothing has changed", "Out of scope: fp32"):
        assert phrase in joined, phrase


def test_null_handles(lbm):
    lib = lbm.load_library()
    buf = (ctypes.c_double * 8)(*([0.01] * 8))
    rho = (ctypes.c_double * 2)(0.1, 0.1)
    on = ctypes.c_int(7)
    vb, vr = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(rho, ctypes.c_void_p)
    pr = ctypes.cast(rho, ctypes.POINTER(ctypes.c_double))
    calls = {"context": [lambda: lib.lbm_dopen_set(None, vb, 0.1), lambda: lib.lbm_dopen_set(None, None, 0.0),
                         lambda: lib.lbm_dopen_get(None, ctypes.byref(on), vb, pr)],
             "ensemble": [lambda: lib.lbm_dopen_ens_set(None, vb, vr), lambda: lib.lbm_dopen_ens_set(None, None, None),
                          lambda: lib.lbm_dopen_ens_get(None, ctypes.byref(on), vb, vr)]}
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
    u = (ctypes.c_double * 4)(0.01, 0.01, 0.01, 0.01)
    vu = ctypes.cast(u, ctypes.c_void_p)
    for bad in (float("nan"), float("inf"), -float("inf"), -0.1, 0.0):
        assert lib.lbm_dopen_set(h, vu, bad) == LBM_ERR_ARG, bad
        assert "rho_out" in lib.lbm_last_error().decode()
    for call in (lib.lbm_dopen_get, lib.lbm_dopen_ens_get):
        assert call(h, None, None, None) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "NULL" in msg and "on_out" in msg and "u_in_out" in msg and "rho_out_out" in msg, msg

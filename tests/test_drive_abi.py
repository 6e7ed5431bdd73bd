"""The body-force entry points (lbm_ddrive_*) as far as they go without a device: header, binding and library agree on the four
names and their argument types, the header holds the statement blocks that define the force, consecutive and in order, its
section follows "Subgrid viscosity", NULL handles are refused, a component that is NaN or infinite is refused before anything of
the handle is read, and so are two NULL outputs.  The fp32 classes have no set_drive.  What needs a handle that exists - the
refusal once steps are done, the member with a zero force and its message, that nothing changes after a refusal, the round
trips, any order with TRT and the subgrid model - is in tests/test_drive_gpu.py (errors and what keeps the setting)."""
import ctypes
import os
import re

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = ["lbm_ddrive_ens_get", "lbm_ddrive_ens_set", "lbm_ddrive_get", "lbm_ddrive_set"]


def header_text():
    return open(os.path.join(ROOT, "include", "lbm.h")).read()


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm_ddrive_[a-z_]+)\s*\(", code)))
    assert syms == NAMES
    assert sorted(s for s in lbm.ABI_SYMBOLS if s.startswith("lbm_ddrive_")) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
    vp, dbl = ctypes.c_void_p, ctypes.c_double
    assert lib.lbm_ddrive_set.argtypes == [vp, dbl, dbl]
    assert lib.lbm_ddrive_get.argtypes == [vp, ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
    assert lib.lbm_ddrive_ens_set.argtypes == [vp, vp]
    assert lib.lbm_ddrive_ens_get.argtypes == [vp, ctypes.POINTER(ctypes.c_int), vp]
    for proto in ("int lbm_ddrive_set(lbm_dp *d, double f_x, double f_y);",
                  "int lbm_ddrive_get(const lbm_dp *d, double *f_x_out, double *f_y_out);",
                  "int lbm_ddrive_ens_set(lbm_dens *e, const double *f );",
                  "int lbm_ddrive_ens_get(const lbm_dens *e, int *on_out, double *f_out );"):
        assert proto in code, proto
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in ("set_drive", "drive"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls in (lbm.LBM, lbm.Ensemble):                                      # fp32: gets nothing, said in lbm.h
        assert not hasattr(cls, "set_drive") and not hasattr(cls, "drive"), cls.__name__


def test_the_definition_is_in_the_header():
    lines = [" ".join(l.lstrip(" *").split()) for l in header_text().splitlines()]
    text = "\n".join(lines)
    shift = ["u_x = ((g[1] - g[3]) + (diag_a + diag_b)) + 0.5 * F_x;",
             "u_y = ((g[2] - g[4]) + (diag_a - diag_b)) + 0.5 * F_y;"]
    source = ["v_x = u_x * densinv; v_y = u_y * densinv;",
              "uF = v_x * F_x + v_y * F_y; t3 = 3.0 * uF;",
              "se[0] = w[0] * (0.0 - t3);",
              "for k = 1..8:",
              "cv = uvec[k] * densinv;",
              "se[k] = w[k] * (9.0 * (cv * cF[k]) - t3);",
              "so[k] = s[k] * cF[k];"]
    bgk = ["BGK: out[0] = (g[0] + omega * (eq[0] - g[0])) + pe * se[0];",
           "out[k] = (g[k] + omega * (eq[k] - g[k])) + pe * (se[k] + so[k]); k = 1..8"]
    trt = ["fe = pe * se[k]; fo = po * so[k];",
           "out[k] = (g[k] + (rp + rm)) + (fe + fo);",
           "out[q] = (g[q] + (rp - rm)) + (fe - fo);"]
    for block in (shift, source, bgk, trt):
        assert "\n".join(block) in text, block                                 # the statements, consecutive and in order
    at = [text.index("\n".join(b)) for b in (shift, source, bgk, trt)]
    assert at == sorted(at)
    # the section order: the new section is the last one, behind "Subgrid viscosity"
    order = ["---- Moving walls", "---- Subgrid viscosity", "---- Body force"]
    where = [text.index(s) for s in order]
    assert where == sorted(where)
    assert text.index("lbm_dles_ens_get(") < text.index("---- Body force") < at[0] < text.index("lbm_ddrive_set(")
    joined = " ".join(lines)
    for phrase in ("Off by default", "NOT multiplied by the cell's density", "contraction off",
                   "one IEEE operation per written operator", "pe = 1.0 - 0.5 * omega", "po = 1.0 - 0.5 * omega_m",
                   "cF[5] = F_x + F_y", "cF[8] = F_x - F_y", "s[5..8] = 1.0 / 12.0", "exact at Lambda = 3/16",
                   "the cell's own om and, with TRT, its own omega_m", "correction of the stress estimate is out of scope",
                   "sum of c_k out[k] = sum of c_k g[k] + F", "subtracts 0.5 * F_x and 0.5 * F_y",
                   "Nothing else moves: blocked cells bounce back", "take no force", "accelerate_flow stays and composes",
                   "the order of every sum", "both steady criteria", "Only while steps_done is 0", "keep the setting",
                   "set in any order", "after a refusal nothing has changed", "Out of scope: fp32"):
        assert phrase in joined, phrase


def test_null_handles(lbm):
    lib = lbm.load_library()
    out = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    f = (ctypes.c_double * 4)(1e-6, 2e-6, 3e-6, 4e-6)
    on = ctypes.c_int(7)
    po = ctypes.cast(out, ctypes.POINTER(ctypes.c_double))
    vo, vf = ctypes.cast(out, ctypes.c_void_p), ctypes.cast(f, ctypes.c_void_p)
    calls = {"context": [lambda: lib.lbm_ddrive_set(None, 1e-6, 0.0), lambda: lib.lbm_ddrive_set(None, 0.0, 0.0),
                         lambda: lib.lbm_ddrive_get(None, po, po)],
             "ensemble": [lambda: lib.lbm_ddrive_ens_set(None, vf), lambda: lib.lbm_ddrive_ens_set(None, None),
                          lambda: lib.lbm_ddrive_ens_get(None, ctypes.byref(on), vo)]}
    for noun, group in calls.items():
        for call in group:
            assert call() == LBM_ERR_ARG
            msg = lib.lbm_last_error().decode()
            assert "NULL" in msg and noun in msg, msg
    assert list(out) == [7.0] * 4 and list(f) == [1e-6, 2e-6, 3e-6, 4e-6] and on.value == 7


def test_bad_arguments_are_refused_before_the_handle_is_read(lbm):
    """The handle is a block of zero bytes, not a context: the refusal comes before anything of it is read, and without a
    device"""
    lib = lbm.load_library()
    fake = ctypes.create_string_buffer(0)
    h = ctypes.cast(fake, ctypes.c_void_p)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for pair in ((bad, 0.0), (0.0, bad), (1e-6, bad), (bad, bad)):
            assert lib.lbm_ddrive_set(h, *pair) == LBM_ERR_ARG, pair
            assert "body force must be finite" in lib.lbm_last_error().decode()
    assert lib.lbm_ddrive_get(h, None, None) == LBM_ERR_ARG
    msg = lib.lbm_last_error().decode()
    assert "NULL" in msg and "f_x_out" in msg and "f_y_out" in msg, msg
    assert lib.lbm_ddrive_ens_get(h, None, None) == LBM_ERR_ARG
    msg = lib.lbm_last_error().decode()
    assert "NULL" in msg and "on_out" in msg and "f_out" in msg, msg

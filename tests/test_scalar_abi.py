"""The scalar entry points (lbm_dscalar_*) as far as they go without a device: header, binding and library agree on the ten names and
their argument types, the header holds the statement blocks that define the scalar, consecutive and in order, its section follows
"Body force", NULL handles are refused, and a negative or non-finite diffusivity, a NULL c0 beside a positive diffusivity and all-NULL
outputs are refused before anything of the handle is read.  The fp32 classes have no set_scalar.  What needs a handle that exists is
in tests/test_scalar_gpu.py (errors and what keeps the setting)."""
import ctypes
import os
import re

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = sorted("lbm_dscalar_" + e + s for e in ("", "ens_") for s in ("set", "get", "field", "download", "upload"))
METHODS = ("set_scalar", "scalar", "scalar_field", "scalar_cells", "upload_scalar")


def header_text():
    return open(os.path.join(ROOT, "include", "lbm.h")).read()


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    code = " ".join(re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S).split())
    syms = sorted(set(re.findall(r"\b(lbm_dscalar_[a-z_]+)\s*\(", code)))
    assert syms == NAMES and len(NAMES) == 10
    assert sorted(s for s in lbm.ABI_SYMBOLS if s.startswith("lbm_dscalar_")) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
    vp, dbl, pi, pd = ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    assert lib.lbm_dscalar_set.argtypes == [vp, dbl, vp, vp, vp]
    assert lib.lbm_dscalar_get.argtypes == [vp, pi, pd, pd]
    assert lib.lbm_dscalar_ens_set.argtypes == [vp, vp, vp, vp, vp]
    assert lib.lbm_dscalar_ens_get.argtypes == [vp, pi, vp, vp]
    for e in ("", "ens_"):
        for s in ("field", "download", "upload"):
            assert getattr(lib, "lbm_dscalar_" + e + s).argtypes == [vp, vp]
    for proto in ("int lbm_dscalar_set(lbm_dp *d, double diffusivity, const double *c0 , const double *c_wall , const double *c_in );",
                  "int lbm_dscalar_get(const lbm_dp *d, int *on_out, double *diffusivity_out, double *omega_s_out);",
                  "int lbm_dscalar_field(lbm_dp *d, double *c_out );",
                  "int lbm_dscalar_download(lbm_dp *d, double *g_out );",
                  "int lbm_dscalar_upload(lbm_dp *d, const double *g );",
                  "int lbm_dscalar_ens_set(lbm_dens *e, const double *diffusivity , const double *c0 , const double *c_wall , "
                  "const double *c_in );",
                  "int lbm_dscalar_ens_get(const lbm_dens *e, int *on_out, double *diffusivity_out , double *omega_s_out );",
                  "int lbm_dscalar_ens_field(lbm_dens *e, double *c_out );",
                  "int lbm_dscalar_ens_download(lbm_dens *e, double *g_out );",
                  "int lbm_dscalar_ens_upload(lbm_dens *e, const double *g );"):
        assert proto in code, proto
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in METHODS:
            assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls in (lbm.LBM, lbm.Ensemble):                                      # fp32: gets nothing, said in lbm.h
        assert not any(hasattr(cls, method) for method in METHODS), cls.__name__


def test_the_definition_is_in_the_header():
    lines = [" ".join(l.lstrip(" *").split()) for l in header_text().splitlines()]
    text = "\n".join(lines)
    host = ["omega_s = 1.0 / (3.0 * D + 0.5);"]
    gather = ["h[0] = g[0](x);",
              "for k = 1..4:",
              "q fluid: h[k] = g[k](q);",
              "q blocked, c_wall(q) NaN: h[k] = g[opp(k)](x);",
              "q blocked, c_wall(q) finite: h[k] = (1.0 / 3.0) * c_wall(q) - g[opp(k)](x);"]
    ends = ["column 0: h[1] = c_in(y) - (((h[0] + h[2]) + h[3]) + h[4]);",
            "column nx - 1: h[3] = g[3](x);"]
    collision = ["C = (((h[0] + h[1]) + h[2]) + h[3]) + h[4];",
                 "a_x = 3.0 * (C * u_x); a_y = 3.0 * (C * u_y);",
                 "e[0] = (1.0 / 3.0) * C;",
                 "e[1] = (1.0 / 6.0) * (C + a_x);",
                 "e[3] = (1.0 / 6.0) * (C - a_x);",
                 "e[2] = (1.0 / 6.0) * (C + a_y);",
                 "e[4] = (1.0 / 6.0) * (C - a_y);",
                 "for k = 0..4:",
                 "g'[k] = h[k] + omega_s * (e[k] - h[k]);"]
    blocks = (host, gather, ends, collision)
    for block in blocks:
        assert "\n".join(block) in text, block                                 # the statements, consecutive and in order
    at = [text.index("\n".join(b)) for b in blocks]
    assert at == sorted(at)
    order = ["---- Subgrid viscosity", "---- Body force", "---- Scalar transport"]
    where = [text.index(s) for s in order]
    assert where == sorted(where)
    assert text.index("lbm_ddrive_ens_get(") < text.index("---- Scalar transport") < at[0] < at[-1] < text.index("lbm_dscalar_set(")
    joined = " ".join(lines)
    for phrase in ("PASSIVE", "Off by default", "speeds k = 0..4 are the flow's speeds 0..4", "1 <-> 3 and 2 <-> 4",
                   "contraction off", "one IEEE operation per written operator", "Scalar step n runs BEFORE flow step n",
                   "after step n's accelerate_flow", "every launch of a run advances ONE step", "insulating wall (half-way bounce-back)",
                   "copied through unchanged", "a blocked cell 0.0", "(1.0 / 3.0) * c0 for k = 0, (1.0 / 6.0) * c0 for the others",
                   "the physical velocity", "Between runs at any step count", "keep the scalar and its state",
                   "c_wall is only ever read at blocked cells", "after a refusal nothing has changed",
                   "would need a gated scalar kernel, which is out of scope", "Out of scope: fp32"):
        assert phrase in joined, phrase


def test_null_handles(lbm):
    lib = lbm.load_library()
    buf = (ctypes.c_double * 8)(*([7.0] * 8))
    vb = ctypes.cast(buf, ctypes.c_void_p)
    pd = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))
    on = ctypes.c_int(7)
    calls = {"context": [lambda: lib.lbm_dscalar_set(None, 0.1, vb, None, None), lambda: lib.lbm_dscalar_set(None, 0.0, None, None, None),
                         lambda: lib.lbm_dscalar_get(None, ctypes.byref(on), pd, pd), lambda: lib.lbm_dscalar_field(None, vb),
                         lambda: lib.lbm_dscalar_download(None, vb), lambda: lib.lbm_dscalar_upload(None, vb)],
             "ensemble": [lambda: lib.lbm_dscalar_ens_set(None, vb, vb, None, None), lambda: lib.lbm_dscalar_ens_set(None, None, None, None, None),
                          lambda: lib.lbm_dscalar_ens_get(None, ctypes.byref(on), vb, vb), lambda: lib.lbm_dscalar_ens_field(None, vb),
                          lambda: lib.lbm_dscalar_ens_download(None, vb), lambda: lib.lbm_dscalar_ens_upload(None, vb)]}
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
    c0 = (ctypes.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    vc = ctypes.cast(c0, ctypes.c_void_p)
    for bad in (float("nan"), float("inf"), -float("inf"), -0.05):
        assert lib.lbm_dscalar_set(h, bad, vc, None, None) == LBM_ERR_ARG, bad
        assert "diffusivity must be finite" in lib.lbm_last_error().decode()
    assert lib.lbm_dscalar_set(h, 0.1, None, None, None) == LBM_ERR_ARG
    assert "c0 is NULL" in lib.lbm_last_error().decode()
    assert lib.lbm_dscalar_ens_set(h, vc, None, None, None) == LBM_ERR_ARG
    assert "c0 is NULL" in lib.lbm_last_error().decode()
    for get in (lib.lbm_dscalar_get, lib.lbm_dscalar_ens_get):
        assert get(h, None, None, None) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "NULL" in msg and "on_out" in msg and "omega_s_out" in msg, msg
    for name in ("field", "download", "upload", "ens_field", "ens_download", "ens_upload"):
        assert getattr(lib, "lbm_dscalar_" + name)(h, None) == LBM_ERR_ARG
        assert "NULL" in lib.lbm_last_error().decode()

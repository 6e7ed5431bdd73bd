"""The entry points of the scalar's record (lbm_drecord_*, lbm_drecord_ens_*, lbm_drecord_steady_run) as far as they
go without a device: header, binding and library agree on the seven names and their argument types, the header holds the three
statements and the order of the sums in a section of its own behind "Buoyancy", NULL handles are refused, and all-NULL outputs, a
`which` outside 0 .. 2 and bad steady-run arguments are refused before anything of the handle is read.  The fp32 classes get
nothing.  What needs a handle that exists (the record with the scalar off, after a step, the scalar switched off under it, a
read or a steady run without it, and that a failed call changes nothing) is in tests/test_scalar_record_gpu.py.  This module
fails on a library without the feature."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = sorted(["lbm_drecord" + e + s for e in ("", "_ens") for s in ("_set", "_get", "")] + ["lbm_drecord_steady_run"])
METHODS = ("set_scalar_record", "scalar_record_on", "scalar_record")


def header_text():
    return open(os.path.join(ROOT, "include", "lbm.h")).read()


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    code = " ".join(re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S).split())
    syms = sorted(set(re.findall(r"\b(lbm_drecord[a-z_]*)\s*\(", code)))
    assert syms == NAMES and len(NAMES) == 7
    assert sorted(s for s in lbm.ABI_SYMBOLS if s.startswith("lbm_drecord")) == NAMES
    assert not any(s.startswith("lbm_dscalar_") for s in NAMES)                # tests/test_scalar_abi.py pins those ten
    for s in syms:
        assert hasattr(lib, s), s
    vp, ci, dbl, pi = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_int)
    for e in ("", "_ens"):
        assert getattr(lib, "lbm_drecord" + e + "_set").argtypes == [vp, ci]
        assert getattr(lib, "lbm_drecord" + e + "_get").argtypes == [vp, pi]
        assert getattr(lib, "lbm_drecord" + e).argtypes == [vp, vp, vp, vp]
    assert lib.lbm_drecord_steady_run.argtypes == [vp, ci, ci, dbl, ci]
    for proto in ("int lbm_drecord_set(lbm_dp *d, int on);",
                  "int lbm_drecord_get(const lbm_dp *d, int *on_out);",
                  "int lbm_drecord(lbm_dp *d, double *content_out , double *flux_x_out , double *flux_y_out );",
                  "int lbm_drecord_ens_set(lbm_dens *e, int on);",
                  "int lbm_drecord_ens_get(const lbm_dens *e, int *on_out);",
                  "int lbm_drecord_ens(lbm_dens *e, double *content_out , double *flux_x_out , double *flux_y_out );",
                  "int lbm_drecord_steady_run(lbm_dens *e, int max_steps, int window, double rel_tol, int which);"):
        assert proto in code, proto
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in METHODS:
            assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls in (lbm.LBM, lbm.Ensemble):                                        # fp32: gets nothing, said in lbm.h
        assert not any(hasattr(cls, method) for method in METHODS), cls.__name__
    assert lbm.EnsembleDouble.SCALAR_CRITERIA == {"scalar": 0, "scalar_flux_x": 1, "scalar_flux_y": 2}


def test_the_definition_is_in_the_header():
    lines = [" ".join(l.lstrip(" *").split()) for l in header_text().splitlines()]
    text = "\n".join(lines)
    block = ["c = (((h[0] + h[1]) + h[2]) + h[3]) + h[4]; content: the sum of c",
             "q_x = c * u_x; flux_x: the sum of q_x",
             "q_y = c * u_y; flux_y: the sum of q_y"]
    assert "\n".join(block) in text                                            # the statements, consecutive and in order
    at = text.index("\n".join(block))
    assert text.index("lbm_dbuoy_ens_get(") < text.index("---- Scalar record") < at < text.index("lbm_drecord_set(")
    joined = " ".join(lines)
    for phrase in ("FLUID cells", "five gathered values behind the wall, inlet and outlet statements",
                   "with buoyancy less half of the cell's own force", "A blocked cell adds +0.0", "contraction off",
                   "one IEEE operation per written operator", "a + b, or a + 0.0 where the lane has no second cell",
                   "the tree of xor 1, 2, 4", "from a ring of the scalar's own", "flux_x / N_fluid * H / (D dC)",
                   "are the same bits with the record on as with it off", "Only with a scalar on (otherwise LBM_ERR_ARG)",
                   "only while steps_done is 0", "Switching the scalar off while the record is on is LBM_ERR_STATE",
                   "leave the recorded entries as they are", "fabs(A(s) - A(s - window)) <= rel_tol * fabs(A(s))",
                   "d2q9_dp_ensemble_gated at depth 1", "d2q9_dp_buoyant_gated", "holds +0.0 from its own count on",
                   "which outside 0 .. 2", "Out of scope: fp32"):
        assert phrase in joined, phrase
    # the sections before it keep their words: the two remarks this one lifts
    before = joined[:joined.index("---- Scalar record")]
    assert before.count("a member that stops would need a gated scalar kernel, which is out of scope") == 1
    assert "Steady runs stay refused while a scalar is on" in before


def test_null_handles(lbm):
    lib = lbm.load_library()
    buf = (ctypes.c_double * 8)(*([7.0] * 8))
    vb = ctypes.cast(buf, ctypes.c_void_p)
    on = ctypes.c_int(7)
    calls = {"context": [lambda: lib.lbm_drecord_set(None, 1), lambda: lib.lbm_drecord_get(None, ctypes.byref(on)),
                         lambda: lib.lbm_drecord(None, vb, vb, vb)],
             "ensemble": [lambda: lib.lbm_drecord_ens_set(None, 1), lambda: lib.lbm_drecord_ens_get(None, ctypes.byref(on)),
                          lambda: lib.lbm_drecord_ens(None, vb, vb, vb), lambda: lib.lbm_drecord_steady_run(None, 8, 4, 1e-3, 0)]}
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
    for read in (lib.lbm_drecord, lib.lbm_drecord_ens):
        assert read(h, None, None, None) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "all NULL" in msg and "content_out" in msg and "flux_x_out" in msg and "flux_y_out" in msg, msg
    for get in (lib.lbm_drecord_get, lib.lbm_drecord_ens_get):
        assert get(h, None) == LBM_ERR_ARG
        assert "on_out is NULL" in lib.lbm_last_error().decode()
    for which in (-1, 3, 7):
        assert lib.lbm_drecord_steady_run(h, 8, 4, 1e-3, which) == LBM_ERR_ARG
        assert "which must be 0 (content), 1 (flux_x) or 2 (flux_y)" in lib.lbm_last_error().decode()
    # lbm_dsteady_run's refusals, which it shares
    for bad, word in (((-1, 4, 1e-3), "max_steps"), ((8, 0, 1e-3), "window"), ((8, 4, -1.0), "rel_tol"), ((8, 4, float("nan")), "rel_tol")):
        assert lib.lbm_drecord_steady_run(h, *bad, 1) == LBM_ERR_ARG
        assert word in lib.lbm_last_error().decode()


def test_an_unknown_criterion_names_the_new_ones(lbm):
    """EnsembleDouble.run_until refuses the name before it touches its handle"""
    ens = object.__new__(lbm.EnsembleDouble)
    with pytest.raises(ValueError) as err:
        lbm.EnsembleDouble.run_until(ens, 8, on="scalar_flux_z")
    for name in ("av_vels", "drag", "scalar", "scalar_flux_x", "scalar_flux_y"):
        assert '"%s"' % name in str(err.value)

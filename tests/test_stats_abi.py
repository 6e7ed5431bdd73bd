"""The running-statistics entry points (lbm_dstats_*) as far as they go without a device: header, binding and library agree on the
six names and their argument types, the header holds the six statements that define a sample, consecutive and in order, in a
section behind "Scalar record", NULL handles are refused, and every < 0 and all-NULL outputs are refused before anything of the
handle is read.  The fp32 classes have none of the four methods.  What needs a handle that exists is in tests/test_stats_gpu.py.
This module fails on a library without the feature."""
import ctypes
import os
import re

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = sorted(["lbm_dstats_set", "lbm_dstats_get", "lbm_dstats", "lbm_dstats_ens_set", "lbm_dstats_ens_get", "lbm_dstats_ens"])
METHODS = ("set_stats", "stats_state", "stats_sums", "stats")


def header_text():
    return open(os.path.join(ROOT, "include", "lbm.h")).read()


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    code = " ".join(re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S).split())
    syms = sorted(set(re.findall(r"\b(lbm_dstats[a-z_]*)\s*\(", code)))
    assert syms == NAMES and len(NAMES) == 6
    assert sorted(s for s in lbm.ABI_SYMBOLS if s.startswith("lbm_dstats")) == NAMES
    for s in syms:
        assert hasattr(lib, s), s
    vp, ci, pi = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    assert lib.lbm_dstats_set.argtypes == [vp, ci] and lib.lbm_dstats_ens_set.argtypes == [vp, ci]
    assert lib.lbm_dstats_get.argtypes == [vp, pi, pi, pi] and lib.lbm_dstats_ens_get.argtypes == [vp, pi, pi, pi]
    assert lib.lbm_dstats.argtypes == [vp, vp] and lib.lbm_dstats_ens.argtypes == [vp, vp]
    for proto in ("int lbm_dstats_set(lbm_dp *d, int every);",
                  "int lbm_dstats_get(const lbm_dp *d, int *every_out, int *origin_out, int *samples_out);",
                  "int lbm_dstats(lbm_dp *d, double *sums_out );",
                  "int lbm_dstats_ens_set(lbm_dens *e, int every);",
                  "int lbm_dstats_ens_get(const lbm_dens *e, int *every_out, int *origin_out, int *samples_out);",
                  "int lbm_dstats_ens(lbm_dens *e, double *sums_out );"):
        assert proto in code, proto
    # the error channel stays last
    assert code.index("lbm_dstats_ens(") < code.index("lbm_last_error(") < code.index("lbm_version(")
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in METHODS:
            assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls in (lbm.LBM, lbm.Ensemble):                                        # fp32: gets nothing, said in lbm.h
        assert not any(hasattr(cls, method) for method in METHODS), cls.__name__
    doc = lbm.LBMDouble.stats.__doc__
    assert "loses as many digits as the variance is small against the squared mean" in " ".join(doc.split())


def test_the_definition_is_in_the_header():
    lines = [" ".join(l.lstrip(" *").split()) for l in header_text().splitlines()]
    text = "\n".join(lines)
    block = ["S[0] = S[0] + u_x;",
             "S[1] = S[1] + u_y;",
             "S[2] = S[2] + pressure;",
             "S[3] = S[3] + u_x * u_x;",
             "S[4] = S[4] + u_y * u_y;",
             "S[5] = S[5] + u_x * u_y;"]
    assert "\n".join(block) in text                                            # the statements, consecutive and in order
    at = text.index("\n".join(block))
    order = ["---- Scalar transport", "---- Buoyancy", "---- Scalar record", "---- Running statistics"]
    where = [text.index(s) for s in order]
    assert where == sorted(where)
    assert text.index("lbm_drecord_steady_run(lbm_dens") < text.index("---- Running statistics") < at < text.index("lbm_dstats_set(lbm_dp")
    joined = " ".join(lines)
    for phrase in ("exactly as lbm_dp_final_state", "a blocked cell giving 0, 0, 0, density / 3", "contraction off",
                   "one IEEE operation per written operator", "left-to-right sum", "s = s0 + j * every, j >= 1",
                   "(first, first + nsteps]", "accepted between runs at ANY step count", "Setting again while on starts anew",
                   "every == 0 switches the statistics off and frees the planes",
                   "lbm_dp_upload, lbm_dens_upload and lbm_dp_upload_obstacles keep the setting", "The run is cut at its sample points",
                   "a cut costs one sample launch and one accelerate launch", "Nothing else moves",
                   "the same bits with statistics on as with them off", "Everything is checked before anything changes",
                   "a gated sample kernel, which is out of scope", "ragged ensemble", "48 B per cell",
                   "Out of scope: fp32 contexts and fp32 ensembles", "moments of the scalar", "a per-member every",
                   "statistics fused into a flow kernel", "shifted or Welford accumulation",
                   "loses as many digits as the variance is small against the squared mean"):
        assert phrase in joined, phrase


def test_null_handles(lbm):
    lib = lbm.load_library()
    buf = (ctypes.c_double * 8)(*([7.0] * 8))
    vb = ctypes.cast(buf, ctypes.c_void_p)
    a, b, c = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    calls = {"context": [lambda: lib.lbm_dstats_set(None, 3), lambda: lib.lbm_dstats_set(None, 0),
                         lambda: lib.lbm_dstats_get(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                         lambda: lib.lbm_dstats(None, vb)],
             "ensemble": [lambda: lib.lbm_dstats_ens_set(None, 3), lambda: lib.lbm_dstats_ens_set(None, 0),
                          lambda: lib.lbm_dstats_ens_get(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                          lambda: lib.lbm_dstats_ens(None, vb)]}
    for noun, group in calls.items():
        for call in group:
            assert call() == LBM_ERR_ARG
            msg = lib.lbm_last_error().decode()
            assert "NULL" in msg and noun in msg, msg
    assert list(buf) == [7.0] * 8 and (a.value, b.value, c.value) == (7, 7, 7)


def test_bad_arguments_are_refused_before_the_handle_is_read(lbm):
    """The handle is a block of zero bytes, not a context: the refusal comes before anything of it is read, and without a
    device"""
    lib = lbm.load_library()
    fake = ctypes.create_string_buffer(0)
    h = ctypes.cast(fake, ctypes.c_void_p)
    for setter in (lib.lbm_dstats_set, lib.lbm_dstats_ens_set):
        for bad in (-1, -7, -2 ** 31):
            assert setter(h, bad) == LBM_ERR_ARG, bad
            assert "every must be >= 1, or 0 (off)" in lib.lbm_last_error().decode()
    for getter in (lib.lbm_dstats_get, lib.lbm_dstats_ens_get):
        assert getter(h, None, None, None) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "NULL" in msg and "every_out" in msg and "origin_out" in msg and "samples_out" in msg, msg
    for sums in (lib.lbm_dstats, lib.lbm_dstats_ens):
        assert sums(h, None) == LBM_ERR_ARG
        assert "sums_out is NULL" in lib.lbm_last_error().decode()

"""The body-map entry points (lbm_dbody_*) as far as they go without a device: header, binding and library agree on the five
names, NULL handles and a NULL body_out are refused with LBM_ERR_ARG and a message that names the argument before anything
is dereferenced, run_until refuses an unknown criterion before the library is called, and the header states the contract."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

LBM_ERR_ARG = 1

NAMES = ["lbm_dbody_ens_get", "lbm_dbody_ens_set", "lbm_dbody_get", "lbm_dbody_set", "lbm_dbody_steady_run"]


def header_text():
    return open(os.path.join(ROOT, "include", "lbm.h")).read()


def test_header_binding_and_library_agree(lbm):
    lib = lbm.load_library()
    code = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm_dbody_[a-z_]+)\s*\(", code)))
    assert syms == NAMES
    for s in syms:
        assert s in lbm.ABI_SYMBOLS and hasattr(lib, s), s
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for s in NAMES[:4]:
        assert getattr(lib, s).argtypes == [vp, vp], s
    assert lib.lbm_dbody_steady_run.argtypes == [vp, ci, ci, ctypes.c_double]
    assert lib.lbm_dbody_steady_run.argtypes == lib.lbm_dsteady_run.argtypes
    for cls in (lbm.LBMDouble, lbm.EnsembleDouble):
        for method in ("set_body", "body"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
    for cls in (lbm.LBM, lbm.Ensemble):                                      # fp32: out of scope, said in lbm.h
        assert not hasattr(cls, "set_body") and not hasattr(cls, "body"), cls.__name__


def test_run_until_signatures(lbm):
    sig = inspect.signature(lbm.EnsembleDouble.run_until)
    assert list(sig.parameters) == ["self", "max_steps", "window", "rel_tol", "on"]
    assert (sig.parameters["window"].default, sig.parameters["rel_tol"].default, sig.parameters["on"].default) == (64, 1e-4, "av_vels")
    assert list(inspect.signature(lbm.Ensemble.run_until).parameters) == ["self", "max_steps", "window", "rel_tol"]   # kept


def test_unknown_criterion_is_refused_before_the_library_is_called(lbm):
    """an EnsembleDouble that was never created (no device here): its handle is never touched"""
    ens = lbm.EnsembleDouble.__new__(lbm.EnsembleDouble)
    ens.ens = ctypes.c_void_p()

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)

    ens.lib = NoLibrary()
    for on in ("nonsense", "", None, "Drag"):
        with pytest.raises(ValueError):
            ens.run_until(8, window=4, rel_tol=1e-2, on=on)


def test_null_handles(lbm):
    lib = lbm.load_library()
    out = (ctypes.c_int32 * 16)()
    p = ctypes.cast(out, ctypes.c_void_p)
    calls = {"context": [lambda: lib.lbm_dbody_set(None, p), lambda: lib.lbm_dbody_set(None, None), lambda: lib.lbm_dbody_get(None, p)],
             "ensemble": [lambda: lib.lbm_dbody_ens_set(None, p), lambda: lib.lbm_dbody_ens_set(None, None),
                          lambda: lib.lbm_dbody_ens_get(None, p), lambda: lib.lbm_dbody_steady_run(None, 8, 4, 1e-2)]}
    for noun, group in calls.items():
        for call in group:
            assert call() == LBM_ERR_ARG
            msg = lib.lbm_last_error().decode()
            assert "NULL" in msg and noun in msg, msg


def test_null_output_and_bad_arguments_are_refused_before_the_handle_is_read(lbm):
    """The handle is a block of zero bytes, not a context: the refusal comes before anything of it is read, and without a
    device"""
    lib = lbm.load_library()
    fake = ctypes.create_string_buffer(4096)
    h = ctypes.cast(fake, ctypes.c_void_p)
    for call in (lib.lbm_dbody_get, lib.lbm_dbody_ens_get):
        assert call(h, None) == LBM_ERR_ARG
        msg = lib.lbm_last_error().decode()
        assert "NULL" in msg and "body_out" in msg, msg
    # the argument refusals of lbm_dsteady_run, each naming its argument
    for args, name in (((-1, 4, 1e-2), "max_steps"), ((8, 0, 1e-2), "window"), ((8, 4, -1.0), "rel_tol"),
                       ((8, 4, float("nan")), "rel_tol")):
        assert lib.lbm_dbody_steady_run(h, *args) == LBM_ERR_ARG
        assert name in lib.lbm_last_error().decode()


def test_the_contract_is_in_the_header():
    text = header_text()
    assert "fabs(F(s) - F(s - window)) <= rel_tol * fabs(F(s))" in text                # the criterion line
    assert text.index("---- Drag and lift: the momentum-exchange force") < text.index("---- Drag of a body")
    text = " ".join(re.sub(r"\n \*", " ", text).split())                               # comment lines joined
    for phrase in ("blocked cells of the body only", "in the body or not, gives no link", "every blocked cell counts",
                   "gives exactly +0.0", "refused with LBM_ERR_ARG", "lbm_dbody_get returns 0 and 1 only",
                   "only while steps_done is 0", "one record never mixes two bodies", "A NaN never stops a member",
                   "stops at its first check point", "nothing is multiplied into it", "Out of scope: fp32"):
        assert phrase in text, phrase
    # what the force section no longer says: a steady run can stop on the force now
    assert "not on its force" not in text
    # lbm_dp_upload_obstacles says what it does to the body
    at = text.index("int lbm_dp_upload_obstacles")
    assert "Resets the body map" in text[at - 600:at]

"""CPU-side test of the chunk-table planner (csrc/chunk_schedule.h): tests/cpu/chunk_schedule_test.cpp checks the
invariants of its tables — built once plain and once under AddressSanitizer + UBSan, run as a plain executable — and the
tables recorded under tests/golden/schedule/ (what the library planned before the planner moved into its header, chunk by
chunk also for pairs) are reproduced: all of them by the chunk-by-chunk rule, and by the default rule every table that is
not a pair schedule of several rounds.  Compiled with g++ — no GPU, no HIP."""
import glob
import json
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "chunk_schedule_test.cpp")
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "schedule", "*.json")))
ARGS = ("rows", "allow_bands", "strips", "waves_resident", "cmax", "cmin", "cmax_one", "pairs", "flex_bands", "r0")
DEFAULT_TAPER = 37  # kPairTaper32


def build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp("chunk_schedule") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory, "chunk_schedule_test", [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return build(tmp_path_factory, "chunk_schedule_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def run_invariants(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "chunk_schedule_test: ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


def test_chunk_tables_keep_their_invariants(exe):
    run_invariants(exe)


def test_chunk_tables_keep_their_invariants_under_sanitizers(exe_san):
    run_invariants(exe_san)


def table(exe, rec, taper):
    out = subprocess.run([exe, "--table"] + [str(rec["args"][k]) for k in ARGS] + [str(taper)], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


def test_goldens_cover_the_recorded_shapes():
    names = {os.path.basename(p)[:-5] for p in GOLDEN}
    for grid in ("1024x1024", "2048x2048", "4096x4096", "8192x4096", "6144x6144", "8192x1024_slab_reserve", "8192x8192"):
        assert {"deep_%s_lone" % grid, "deep_%s_pairs" % grid} <= names
    assert {"step3p_1024x1024", "step4p_1024x1024", "twin5_1024x1024"} <= names


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[:-5])
def test_recorded_tables_are_reproduced(exe_san, path):
    with open(path) as f:
        rec = json.load(f)
    want = {k: rec[k] for k in ("nbands", "chunks_per_band", "single_round", "starts")}
    assert rec["pair_taper_applies"] == bool(rec["args"]["pairs"] and not rec["single_round"])
    assert table(exe_san, rec, 0) == want
    got = table(exe_san, rec, DEFAULT_TAPER)
    if not rec["pair_taper_applies"]:
        assert got == want
    else:
        # the pair taper plans these anew: same bands, same rows, another split
        assert got["nbands"] == want["nbands"] and not got["single_round"]
        assert got["starts"][0] == want["starts"][0] and got["starts"][-1] == want["starts"][-1]
        assert got["starts"] != want["starts"]

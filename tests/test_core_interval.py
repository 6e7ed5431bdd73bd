"""CPU-side test of the CORE stretch of a deep-window sweep (csrc/core_interval.h): tests/cpu/core_interval_test.cpp checks
every iteration of every returned interval against the four conditions the kernel's CORE loop relies on, by brute force, and
that no longer run of such iterations exists — grids of 16 to 400 rows, chunks of 1 to 160 rows, both sweep directions, lone
waves and twins, depths 5 to 8, accelerated rows anywhere (none, one, two copies).  Built once plain and once under
AddressSanitizer + UBSan, run as a plain executable.  Compiled with g++ — no GPU, no HIP."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "core_interval_test.cpp")


def build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp("core_interval") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory, "core_interval_test", [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return build(tmp_path_factory, "core_interval_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "core_interval_test: ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


def test_core_intervals_hold_their_conditions(exe):
    run(exe)


def test_core_intervals_hold_their_conditions_under_sanitizers(exe_san):
    run(exe_san)

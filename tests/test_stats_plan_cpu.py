"""Where a run with running statistics is cut (csrc/stats_plan.h), without a device: tests/cpu/stats_plan_test.cpp prints the plan
of every row of its table, built once plain and once under AddressSanitizer + UBSan with g++ and run as a plain executable; every
line is compared with the Python restatement (tests/_stats_ref.py), and the restatement with the properties the header states:
the pieces sum to nsteps, every sample point in (first, first + nsteps] ends a piece, no other piece is marked."""
import os
import subprocess

import pytest

import _stats_ref as ref
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "stats_plan_test.cpp")


def build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp("stats_plan") / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory, "stats_plan_test", [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return build(tmp_path_factory, "stats_plan_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def rows_of(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "stats_plan_test: ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ":" in ln and not ln.startswith("stats_plan_test")]
    return [(tuple(int(v) for v in ln.split(":")[0].split()), ln.rstrip()) for ln in lines]


def check(exe):
    rows = rows_of(exe)
    assert len(rows) >= 20
    for row, line in rows:
        assert line == ref.plan_text(*row), row
    table = [row for row, _ in rows]
    live = [r for r in table if ref.plan(*r) is not None and r[3] > 0 and r[1] > 0]
    # the cases the table must hold
    assert any(r[3] == 1 for r in live)                                                   # every step
    assert any(r[3] > r[1] and not any(m for _, m in ref.plan(*r)) for r in live)         # every larger than the run
    assert any(ref.plan(*r)[-1][1] for r in live)                                         # ends exactly on a sample point
    assert any(r[0] > r[2] and (r[0] - r[2]) % r[3] == 0 for r in live)                   # starts on one
    assert any(r[2] > r[0] and r[3] > 0 and ref.plan(*r) is None for r in table)          # origin beyond first: refused
    assert any(r[1] == 0 and ref.plan(*r) == [] for r in table)                           # no steps
    assert any(r[3] == 0 and ref.plan(*r) == [(r[1], False)] for r in table if r[1] > 0)  # off: one piece
    assert any(r[2] > 0 for r in live)                                                    # an origin behind a transient


def test_the_plan_is_the_restatement(exe):
    check(exe)


def test_the_plan_is_the_restatement_under_sanitizers(exe_san):
    check(exe_san)


def test_the_restatement_holds_the_stated_properties():
    """brute force over small arguments: the pieces sum to nsteps, each is at least one step, the marked ends are exactly the
    sample points of the run, and a run that starts on a sample point does not take it again"""
    count = 0
    for every in range(0, 9):
        for origin in range(0, 7):
            for first in range(origin, origin + 12):
                for nsteps in range(0, 20):
                    pieces = ref.plan(first, nsteps, origin, every)
                    assert pieces is not None
                    assert sum(n for n, _ in pieces) == nsteps and all(n >= 1 for n, _ in pieces)
                    ends, at = [], first
                    for n, mark in pieces:
                        at += n
                        if mark:
                            ends.append(at)
                    want = [s for s in range(first + 1, first + nsteps + 1) if every and s > origin and (s - origin) % every == 0]
                    assert ends == want and first not in ends
                    assert all(mark for _, mark in pieces[:-1])                # only the last piece may end off a sample point
                    count += 1
    assert count > 10000
    # run(10); run(5); run(6) and one run of 21 take the same sample points
    for every in (1, 3, 4, 7):
        split, first = [], 0
        for n in (10, 5, 6):
            split += ref.sample_points(first, n, 0, every)
            first += n
        assert split == ref.sample_points(0, 21, 0, every)
    assert ref.sample_points(0, 21, 0, 7) == [7, 14, 21]
    assert ref.sample_points(5, 10, 5, 3) == [8, 11, 14]


def test_the_accumulation_is_a_left_to_right_sum():
    import numpy as np
    rng = np.random.default_rng(5)
    acc = ref.Sums((3, 4))
    fields = [rng.standard_normal((3, 3, 4)) for _ in range(5)]
    for u_x, u_y, pr in fields:
        acc.add(u_x, u_y, pr)
    want = np.zeros((3, 4))
    for u_x, u_y, _ in fields:
        want = want + u_x * u_y
    assert acc.samples == 5 and np.array_equal(acc.sums()[5], want)
    ens = ref.Sums((2, 3, 4))
    assert ens.sums().shape == (2, 6, 3, 4)

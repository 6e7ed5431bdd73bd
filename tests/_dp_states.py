"""States, parameters and gates of the double-precision families that more than one test module needs: the gates of
tests/test_dp_gpu.py at print precision, the oracle's parameters and tracks, random states, and the members, runs and cases of
tests/test_dp_ensemble_gpu.py.  Nothing here needs a GPU to import."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

PRINT_PRECISION_PCNT = 1e-8       # % (tests/test_oracle_golden.py): the golden files carry 13 significant digits
VEL_ABS = 1e-12                   # u_x, u_y, u: 9x the 1.1e-13 the oracle's forms differ by
PRESSURE_ABS_256 = 1e-12
RE_REL = 1e-10                    # the oracle's forms: <= 8e-13
ORACLE_FORMS_FACTOR = 4.0         # section 3: gate = 4x the largest difference between the oracle's two fp64 forms
MASS_REL = 1e-12                  # the fp64 oracle alone, 256x256 after 1000 steps: 1.8e-13
LDS = 8                           # "multistep" of the LDS-tile form
W = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float64).reshape(9, 1, 1)

FULL = {"128x128": 40000, "128x256": 40000, "256x256": 80000, "1024x1024": 20000}


def max_pcnt(ref, sim):
    diff = ref - sim
    return float(np.max(np.abs(100.0 * diff / (ref - diff))))


def oracle_params(orc, p):
    q = orc.Params()
    q.nx, q.ny, q.max_iters, q.reynolds_dim = p.nx, p.ny, p.max_iters, p.reynolds_dim
    q.density, q.accel, q.omega, q.free_cells_inv = p.density, p.accel, p.omega, p.free_cells_inv
    return q


def build_oracle_nofma(tmp_path_factory):
    """oracle/d2q9_oracle.c in double with pairwise momenta and contraction off, built as test_dp_gpu.oracle_fma builds its
    contracted twin: what the `oracle_nofma` fixtures return"""
    out = str(tmp_path_factory.mktemp("oracle_nofma") / "liboracle_f64_pairwise.so")
    src = os.path.join(ROOT, "oracle", "d2q9_oracle.c")
    subprocess.run(["gcc", "-std=c99", "-O3", "-march=native", "-fPIC", "-DREAL=double", "-DORACLE_PAIRWISE=1",
                    "-ffp-contract=off", "-shared", src, "-o", out, "-lm"], check=True)
    from oracle.oracle import Oracle
    o = Oracle("f64")
    base = o.lib
    o.lib = ctypes.CDLL(out)
    for name in ("oracle_accelerate_flow", "oracle_timestep"):
        f, g = getattr(o.lib, name), getattr(base, name)
        f.argtypes, f.restype = g.argtypes, g.restype
    assert o.lib.oracle_pairwise_momentum() == 1 and o.lib.oracle_real_size() == 8
    return o


def oracle_track(orc, p, ob, cells0, checkpoints):
    """the oracle's cells and av_vels at each checkpoint (cumulative steps)"""
    q = oracle_params(orc, p)
    cells = np.array(cells0, dtype=np.float64, copy=True)
    av_all, out, done = [], [], 0
    with np.errstate(invalid="ignore"):
        for n in checkpoints:
            av_all.append(orc.run(q, cells, ob, n - done))
            done = n
            out.append((cells.copy(), np.concatenate(av_all)))
    return out


def gpu_track(lbm, p, ob, cells0, checkpoints, multistep):
    out, done = [], 0
    with lbm.LBMDouble(p, ob) as sim:
        sim.set_option("multistep", multistep)
        sim.upload(cells0)
        for n in checkpoints:
            sim.run(n - done)
            done = n
            c, av = sim.download()
            out.append((c, av))
    return out


def max_abs(a, b):
    """max |a - b|; a NaN in both at the same place (av_vels of a grid without a free cell: 0 * inf) counts 0"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return math.inf
    return float(np.max(np.abs(a[~na] - b[~nb]), initial=0.0))


def reynolds_ref(size):
    with open(os.path.join(GOLDEN, "transcripts.json")) as f:
        tr = json.load(f)
    if size in tr["reynolds"]:
        return tr["reynolds"][size]
    with open(os.path.join(GOLDEN, "generated", "oracle_f64_scalars.json")) as f:
        return json.load(f)[size]["reynolds"]


def random_state(rng, density, ny, nx):
    return W * density * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5))


# ---- the members, runs and cases of tests/test_dp_ensemble_gpu.py -----------------------------------------------------------

CHECKPOINTS = [1, 2, 11, 1000]
# runs between the checkpoints: 1, 1, 9, then 2..8 (with at most 8 steps a launch: one launch of every depth; with fewer,
# every depth up to that and two-launch splits), 20 (7 + 7 + 6) and the tail
RUNS = [1, 1, 9, 2, 3, 4, 5, 6, 7, 8, 20, 1000 - 11 - 35 - 20]
assert sum(RUNS) == CHECKPOINTS[-1]


def make_members(lbm, nx, ny, n, seed, max_iters=CHECKPOINTS[-1], masks=None):
    """n members that differ in omega, accel, density, obstacle map and initial state"""
    rng = np.random.default_rng(seed)
    params, obs, cells = [], [], []
    for k in range(n):
        ob = masks[k] if masks is not None else (rng.random((ny, nx)) < 0.05 + 0.03 * k).astype(np.int32)
        density = 0.1 * (1.0 + 0.05 * k)
        params.append(lbm.make_dparams(nx, ny, max_iters, density=density, accel=0.005 * (1.0 + 0.2 * k),
                                       omega=1.0 + 0.85 * (k + 1) / n, obstacles=ob))
        obs.append(ob)
        cells.append(random_state(rng, density, ny, nx))
    return params, np.stack(obs), np.stack(cells)


def blocked_and_free_masks(nx, ny):
    rng = np.random.default_rng(99)
    ordinary = [(rng.random((ny, nx)) < 0.1).astype(np.int32) for _ in range(2)]
    return [ordinary[0], np.ones((ny, nx), dtype=np.int32), np.zeros((ny, nx), dtype=np.int32), ordinary[1]]


def one_blocked_cell(n):
    """3x3: member k has cell k blocked (without any obstacle nothing opposes the acceleration on nine cells)"""
    masks = []
    for k in range(n):
        m = np.zeros(9, dtype=np.int32)
        m[k] = 1
        masks.append(m.reshape(3, 3))
    return masks


CASES = {
    "128x128": (128, 128, 5, None),
    "128x256": (128, 256, 3, None),
    "256x256": (256, 256, 3, None),
    "ragged 100x37": (100, 37, 4, None),
    "3x3": (3, 3, 3, one_blocked_cell(3)),
    "near the bound 1024x300": (1024, 300, 2, None),
    "all-blocked and all-free members 64x48": (64, 48, 4, blocked_and_free_masks(64, 48)),
}

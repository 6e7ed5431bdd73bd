"""The CORE form of the deep window kernels' row loop (csrc/d2q9_kernels.h: deep_sweep; option "core_loop"): the rows of a
chunk's interior — every level on one of the chunk's own rows, none on the accelerated row, no row wrap (csrc/core_interval.h)
— run without the per-level tests and with carried row pointers.  Same arithmetic: every cell must equal single steps bit for
bit, with the option on (the default) and off, and av_vels stays within the suite's 2e-6 of single steps.

Grids put the accelerated row ny-2 on a chunk's first row, its last row and within a depth of rows either side of a chunk
boundary; chunk lengths 7 ... 10 give no CORE stretch, then the shortest one; 23 steps end with a launch of depth 7, 6 steps
are one launch of depth 6.  Without obstacles every wave sweeps free (and so runs CORE); with obstacles in a band of rows and
a band of columns free and looking twins share workgroups."""
import numpy as np
import pytest

from test_gpu_parity import SINGLE, max_rel, run_gpu, sparse_obstacles

pytestmark = pytest.mark.gpu

C = 24
GRIDS = [(256, 4 * C + j, C) for j in (0, 1, 2, 7, 8, 9)] + [(512, 300, 40), (1024, 300, 128), (260, 131, 17)] + \
        [(256, 64, c) for c in (7, 8, 9, 10)]
STEPS = {(256, 4 * C + 1, C): (6, 8, 16, 23)}


def start(rng, nx, ny):
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float64).reshape(9, 1, 1) * 0.1
    return (w * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5))).astype(np.float32)


@pytest.mark.parametrize("obstacles", ["none", "sparse"])
@pytest.mark.parametrize("nx,ny,chunk", GRIDS, ids=lambda v: str(v))
def test_core_loop_is_bit_identical_to_single_steps(lbm, nx, ny, chunk, obstacles):
    rng = np.random.default_rng(nx + 3 * ny + chunk)
    ob = sparse_obstacles(rng, nx, ny, 20, 200) if obstacles == "sparse" else np.zeros((ny, nx), np.int32)
    cells0 = start(rng, nx, ny)
    for nsteps in STEPS.get((nx, ny, chunk), (8, 16, 23)):
        p = lbm.make_params(nx, ny, nsteps, obstacles=ob)
        single, av_single = run_gpu(lbm, p, ob, cells0, nsteps, SINGLE)
        for pair in (0, 1):
            for core in (1, 0):
                with lbm.LBM(p, ob) as sim:
                    assert sim.get_option("core_loop") == 1  # on by default
                    opts = {"multistep": 0, "fuse": 8, "nt_stores": 1, "free_sweeps": 1, "chunk_rows": chunk, "pair": pair, "core_loop": core}
                    if pair == 1:
                        opts["twin_steps"] = 8
                    for k, v in opts.items():
                        sim.set_option(k, v)
                    assert sim.get_option("fuse") == 8 and sim.get_option("pair") == pair
                    assert sim.get_option("free_sweeps") == 1 and sim.get_option("core_loop") == core
                    sim.upload(cells0)
                    sim.run(nsteps)
                    got, av = sim.download()
                assert np.array_equal(got, single), (nsteps, pair, core)
                assert max_rel(av, av_single) < 2e-6, (nsteps, pair, core)


def test_core_loop_option_values(lbm):
    nx, ny = 256, 64
    ob = np.zeros((ny, nx), np.int32)
    with lbm.LBM(lbm.make_params(nx, ny, 8, obstacles=ob), ob) as sim:
        for value, back in ((0, 0), (1, 1), (-1, 1)):
            sim.set_option("core_loop", value)
            assert sim.get_option("core_loop") == back
        with pytest.raises(Exception):
            sim.set_option("core_loop", 2)

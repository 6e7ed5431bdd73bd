"""The eight-step chunk pairs (d2q9_deep_twin<8>) on a pair schedule of SEVERAL rounds, tapered over pairs of equal halves
(csrc/chunk_schedule.h): bit-identical to single steps.  512 x 4104 is the smallest grid that gets there on a 256-CU
device: 5 strips and 513 rows per band against about 50 pair slots per band and strip need chunks of 11 rows for one round,
and chunk_rows 8 allows 8."""
import numpy as np
import pytest

from test_gpu_parity import SINGLE, max_rel, random_case, run_gpu, sparse_obstacles

pytestmark = pytest.mark.gpu

OPTS = {"multistep": 0, "fuse": 8, "pair": 1, "twin_steps": 8, "chunk_rows": 8, "chunk_min": 4, "nt_stores": 1}


def tapered_pairs_equal_single_steps(lbm, ob, cells0, nsteps):
    ny, nx = ob.shape
    p = lbm.make_params(nx, ny, nsteps, obstacles=ob)
    single, av_single = run_gpu(lbm, p, ob, cells0, nsteps, SINGLE)
    with lbm.LBM(p, ob) as sim:
        for k, v in OPTS.items():
            sim.set_option(k, v)
        assert sim.get_option("pair") == 1 and sim.get_option("launch_steps") == 8
        # more units than the device has pair slots (four 40-KB pair workgroups per CU): several rounds
        assert sim.get_option("fuse_units") > 4 * sim.get_option("cus")
        sim.upload(cells0)
        sim.run(nsteps)
        got, av = sim.download()
    assert np.array_equal(got, single)
    err = max_rel(av, av_single)
    print("av_vels max rel %.3e" % err)
    assert err < 2e-6


@pytest.mark.parametrize("nx,ny,nsteps", [(512, 4104, 8), (512, 4104, 23), (512, 4101, 8)])
def test_tapered_pair_schedule_equals_single_steps(lbm, nx, ny, nsteps):
    """random obstacles with a band of free rows, so that both collision paths run; 23 steps are launches of 8 + 8 + 7;
    4101 rows leave bands of 513 and 512 rows, odd remainders in the last pairs"""
    rng = np.random.default_rng(6 * nx + ny + nsteps)
    ob, cells0 = random_case(rng, nx, ny)
    ob[ny // 3: 2 * ny // 3, :] = 0
    tapered_pairs_equal_single_steps(lbm, ob, cells0, nsteps)


def test_tapered_pair_schedule_with_free_and_looking_twins(lbm):
    """obstacles in a band of rows and a band of columns only: free and looking twins share workgroups"""
    nx, ny, nsteps = 512, 4104, 8
    rng = np.random.default_rng(nx + 3 * ny + nsteps)
    ob = sparse_obstacles(rng, nx, ny, 20, 200)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=np.float64).reshape(9, 1, 1) * 0.1
    cells0 = (w * (1.0 + 0.2 * (rng.random((9, ny, nx)) - 0.5))).astype(np.float32)
    tapered_pairs_equal_single_steps(lbm, ob, cells0, nsteps)

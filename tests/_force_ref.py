"""The momentum-exchange force of include/lbm.h restated in numpy float64, with the masks, cases and states that
tests/test_force_gpu.py, tests/test_body_gpu.py and the modules on top of them share.

`restatement` is the header's definition, np.roll per speed over the mask, evaluated on a state accelerated with the fp64 oracle's
accelerate_flow (`accelerated`); `body_restatement` is the same with the outer sum over the blocked cells of a body only.
force_mask: a partial wall, a 4x5 block, 3 % random cells, a blocked cell at x = 0 facing fluid at x = nx-1 across the wrap and the
same in y, blocked cells on rows ny-1, ny-2, ny-3 with fluid beside them on ny-2, an isolated blocked cell, a blocked cell with
all eight neighbours blocked, blocked cells at x = 15 | 16 and y = 15 | 16 (tile seams)."""
import numpy as np

from _dp_states import oracle_params, random_state
from _steady_rule import channel

U = 2.0 ** -53
# speed k: c_k = (CX[k], CY[k]); OPP[k] the opposite speed (include/lbm.h)
CX = [0, 1, 0, -1, 0, 1, -1, -1, 1]
CY = [0, 0, 1, 0, -1, 1, 1, -1, -1]
OPP = [0, 3, 4, 1, 2, 7, 8, 5, 6]
SHAPES = [(16, 16), (33, 19), (48, 35), (128, 128), (3, 3)]
SINGLE_STEPS = 12


def force_mask(nx, ny, seed=7):
    """the masks of the module docstring, as far as the grid has room for them"""
    ob = np.zeros((ny, nx), dtype=np.int32)
    if nx == 3 and ny == 3:
        ob[1, 1] = 1
        return ob
    rng = np.random.default_rng(seed)
    ob[:] = rng.random((ny, nx)) < 0.03
    ob[0, : 3 * nx // 4] = 1                                  # a wall on row 0, open at its east end
    ob[ny - 1, :] = 0
    ob[ny - 1, nx // 2:nx // 2 + 3] = 1                       # rows ny-1, ny-2, ny-3, fluid beside them on ny-2
    ob[ny - 2, nx // 2 + 1] = 1
    ob[ny - 2, [nx // 2, nx // 2 + 2]] = 0
    ob[ny - 3, nx // 2:nx // 2 + 2] = 1
    ob[ny // 2 - 2:ny // 2 + 2, nx // 4:nx // 4 + 5] = 1      # a 4x5 block
    ob[ny // 2, 0] = 1                                        # x = 0 facing fluid at x = nx-1 across the wrap
    ob[ny // 2 - 1:ny // 2 + 2, nx - 1] = 0
    ob[0, 1] = 1                                              # y = 0 facing fluid at y = ny-1 (row ny-1 is fluid there)
    if nx >= 16 and ny >= 12:
        y, x = ny - 7, nx - 5                                 # an isolated blocked cell
        ob[y - 1:y + 2, x - 1:x + 2] = 0
        ob[y, x] = 1
        ob[3:6, nx - 7:nx - 4] = 1                            # 3x3: its centre has all eight neighbours blocked
    for y in (15, 16):                                        # tile seams
        for x in (15, 16):
            if x < nx and y < ny - 3:
                ob[y, x] = 1
    if nx > 20 and ny > 20:
        ob[15, 14] = ob[16, 17] = 0
    assert 0 < np.count_nonzero(ob) < ob.size
    return ob


def restatement(f, ob):
    """include/lbm.h's definition on the accelerated state f float64[9, ny, nx]: (F_x, F_y, links, sum of |link terms|)"""
    assert f.dtype == np.float64
    blocked = ob != 0
    fx = fy = 0.0
    links, mag = 0, 0.0
    for k in range(1, 9):
        # at o: the neighbour x = o - c_k (periodic), np.roll(a, s)[i] = a[i - s]
        shift = (CY[k], CX[k])
        counted = blocked & np.roll(~blocked, shift, axis=(0, 1))
        term = (np.roll(f[k], shift, axis=(0, 1)) + f[OPP[k]])[counted]
        fx += CX[k] * float(np.sum(term))
        fy += CY[k] * float(np.sum(term))
        links += int(term.size)
        mag += float(np.sum(np.abs(term)))
    return fx, fy, links, mag


def body_restatement(f, ob, body):
    """restatement with the outer sum over the blocked cells of the body only: counted &= body"""
    assert f.dtype == np.float64
    blocked = ob != 0
    fx = fy = 0.0
    links, mag = 0, 0.0
    for k in range(1, 9):
        shift = (CY[k], CX[k])
        counted = blocked & np.roll(~blocked, shift, axis=(0, 1))
        counted &= body != 0
        term = (np.roll(f[k], shift, axis=(0, 1)) + f[OPP[k]])[counted]
        fx += CX[k] * float(np.sum(term))
        fy += CY[k] * float(np.sum(term))
        links += int(term.size)
        mag += float(np.sum(np.abs(term)))
    return fx, fy, links, mag


def block_body(nx, ny):
    """the 4x4 block of _steady_rule.channel, without the walls"""
    body = np.zeros((ny, nx), dtype=np.int32)
    body[ny // 2 - 2:ny // 2 + 2, nx // 4:nx // 4 + 4] = 1
    ob = channel(nx, ny)
    assert np.count_nonzero(body) == 16 and not np.any(body & (ob == 0)) and np.count_nonzero(ob) == 16 + 2 * nx
    return body


def fluid_momentum(f, ob):
    fluid = ob == 0
    return (sum(CX[k] * float(np.sum(f[k][fluid])) for k in range(1, 9)),
            sum(CY[k] * float(np.sum(f[k][fluid])) for k in range(1, 9)))


def case(lbm, nx, ny, max_iters, seed=11):
    ob = force_mask(nx, ny)
    p = lbm.make_dparams(nx, ny, max_iters, density=0.1, accel=0.005, omega=1.7, obstacles=ob)
    return p, ob, random_state(np.random.default_rng(seed + nx), 0.1, ny, nx)


_single = {}


def single_steps(lbm, nx, ny, multistep):
    """12 steps one at a time: the state before each step and after the last, and the record.  Computed once per case."""
    key = (nx, ny, multistep)
    if key not in _single:
        p, ob, cells0 = case(lbm, nx, ny, SINGLE_STEPS)
        states = []
        with lbm.LBMDouble(p, ob) as sim:
            sim.set_option("multistep", multistep)
            sim.set_option("force", 1)
            assert sim.get_option("force") == 1
            sim.upload(cells0)
            for _ in range(SINGLE_STEPS):
                states.append(sim.download(av_vels=False)[0])
                sim.run(1)
            states.append(sim.download(av_vels=False)[0])
            fx, fy = sim.force_record()
        assert fx.shape == fy.shape == (SINGLE_STEPS,)
        _single[key] = (p, ob, states, fx, fy)
    return _single[key]


def accelerated(orc, p, ob, cells):
    f = np.array(cells, dtype=np.float64, copy=True)
    orc.accelerate_flow(oracle_params(orc, p), f, ob)
    return f

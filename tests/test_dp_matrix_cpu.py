"""The inputs of tests/test_dp_matrix_gpu.py held to what that module needs of them, without a GPU.  A comparison on the GPU
proves only what its inputs can show; every condition here is asserted per shape and per member, on the masks and on the very
states the GPU module uploads (tests/_dp_matrix.py builds both).

  1. matrix_mask keeps its promises: which cells are blocked, which are in the body, that the lips and the column cells of
     different members lie in different rows, that no body cell is in column 0 or nx - 1;
  2. at least 8 counted links have their fluid end in column 0 and at least 8 in column nx - 1, with the body counted and
     with every blocked cell counted; the member with the cell beside column 0's blocked cell has a link toward that blocked
     cell (not counted) and links toward the marked fluid cells above and below it (counted);
  3. taking those links out of _open_ref.force moves F_x or F_y by more than 1000 x the force gate 8 L 2^-53 sum|link terms|: a
     force pass that loses them cannot pass the GPU module's gate.  A condition, not a measurement (the figures are printed:
     2.9e8 to 1.6e11 gates);
  4. with every flag off reference_step is the fp64 oracle's pairwise no-FMA step bit for bit (the link that
     tests/test_trt_restatement_cpu.py holds, on this geometry);
  5. the open and the periodic step of one state differ in columns 0 and nx - 1, and the TRT step is more than 1e-3 relative
     from the BGK step: the flags of reference_step choose other operators (test_open_gpu's and test_trt_gpu's checks)."""
import numpy as np
import pytest

import _dp_matrix as dm
import _open_ref
from _dp_states import build_oracle_nofma, oracle_params

SHAPES = [(33, 19), (17, 16), (48, 35)]
STEADY_SHAPE = (48, 32)


@pytest.fixture(scope="module")
def oracle_nofma(tmp_path_factory):
    return build_oracle_nofma(tmp_path_factory)


@pytest.fixture(scope="module")
def oracle_f64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def members_of(nx, ny):
    return range(4 if (nx, ny) == STEADY_SHAPE else 3)


@pytest.mark.parametrize("nx,ny", SHAPES + [STEADY_SHAPE])
def test_masks_hold_what_they_promise(nx, ny):
    seen = {"lip_west": set(), "lip_east": set(), "cell_west": set(), "cell_east": set()}
    for k in members_of(nx, ny):
        for beside in (False, True):
            ob, body = dm.matrix_mask(nx, ny, k, beside=beside)
            r = dm.matrix_rows(nx, ny, k)
            assert ob.dtype == np.int32 and body.dtype == np.int32 and ob.shape == body.shape == (ny, nx)
            want_body = np.zeros((ny, nx), dtype=bool)
            want_body[ny // 2 - 2:ny // 2 + 2, nx // 4:nx // 4 + 5] = True
            assert np.count_nonzero(want_body) == 20
            for row, x in ((r.lip_west, 1), (r.lip_east, nx - 2)):
                assert 1 <= row and row + 2 <= ny - 2                      # between the walls
                assert not np.any(want_body[row:row + 3, x])               # apart from the block
                want_body[row:row + 3, x] = True
            if beside:
                assert not want_body[r.cell_west, 1]
                want_body[r.cell_west, 1] = True
            assert np.count_nonzero(want_body) == 26 + beside
            want_ob = want_body.copy()
            want_ob[0] = want_ob[ny - 1] = True
            for row, x in ((r.cell_west, 0), (r.cell_east, nx - 1)):
                assert 2 <= row <= ny - 3 and not want_ob[row, x]
                want_ob[row, x] = True
                assert not want_ob[row - 1, x] and not want_ob[row + 1, x]  # fluid above and below it in its column
            assert np.array_equal(ob != 0, want_ob) and np.array_equal(body != 0, want_body)
            assert not np.any(body[:, 0]) and not np.any(body[:, nx - 1])
            assert not np.any(body[0]) and not np.any(body[ny - 1])         # the walls are outside the body
            assert np.count_nonzero(ob[1:ny - 1, 0]) == 1 and np.count_nonzero(ob[1:ny - 1, nx - 1]) == 1
        for name in seen:
            row = getattr(r, name)
            assert row not in seen[name], (name, k)                        # another row than every earlier member's
            seen[name].add(row)
    ob, body = dm.matrix_mask(5, 4)
    assert not np.any(ob) and body is None


@pytest.mark.parametrize("nx,ny", SHAPES + [STEADY_SHAPE])
def test_counted_links_end_in_both_open_columns_and_dropping_them_is_seen(lbm, nx, ny):
    for counted in ("body", "all"):
        case = dm.make_case(lbm, nx, ny, len(members_of(nx, ny)), 1, True, False, True, counted=counted, beside=1)
        for k, m in enumerate(case.members):
            assert (m.body is None) == (counted == "all")
            west, east, dx, dy = dm.column_links(m.cells0, m.ob, m.body)
            fx, fy, links, mag = _open_ref.force(m.cells0, m.ob, m.body)
            gate = 8.0 * links * dm.U * mag
            print("%dx%d member %d, %s counted: %d links, %d end in column 0, %d in column %d; without them F moves by (%.3e, %.3e) = "
                  "(%.1e, %.1e) gates of %.2e" % (nx, ny, k, counted, links, west, east, nx - 1, dx, dy, abs(dx) / gate, abs(dy) / gate,
                                                 gate))
            assert west >= 8 and east >= 8 and links > west + east
            assert gate > 0.0 and max(abs(dx), abs(dy)) > 1000.0 * gate
            # column_links names links of _open_ref.force: with the two columns' fluid cells read as blocked, the force is
            # the rest of the sum
            shut = m.ob.copy()
            shut[:, 0] = shut[:, nx - 1] = 1
            rx, ry, rest, _ = _open_ref.force(m.cells0, shut, m.ob if m.body is None else m.body)
            assert rest == links - west - east
            assert abs((fx - dx) - rx) <= gate and abs((fy - dy) - ry) <= gate


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_the_cell_beside_the_blocked_column_cell_has_both_kinds_of_link(nx, ny):
    k = 1
    ob, body = dm.matrix_mask(nx, ny, k, beside=True)
    r = dm.matrix_rows(nx, ny, k)
    row = r.cell_west
    assert ob[row, 1] and body[row, 1] and _open_ref.counted_cells(ob, body)[row, 1]
    assert ob[row, 0] and not body[row, 0]                                 # its west neighbour: blocked, the link does not count
    assert not ob[row - 1, 0] and not ob[row + 1, 0]                       # its two diagonal neighbours in column 0: fluid, marked
    f = dm.member_state(nx, ny, k)
    with_cell = dm.column_links(f, ob, body)
    plain_ob, plain_body = dm.matrix_mask(nx, ny, k)
    without = dm.column_links(f, plain_ob, plain_body)
    # the cell brings exactly its two diagonal links into column 0 (the lips are not its neighbours)
    assert abs(row - r.lip_west) > 1 and abs(row - (r.lip_west + 2)) > 1
    assert with_cell[0] == without[0] + 2 and with_cell[1] == without[1]


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_with_every_flag_off_the_reference_is_the_oracle_step(lbm, oracle_nofma, nx, ny):
    case = dm.make_case(lbm, nx, ny, 3, 6, False, False, False)
    for k, m in enumerate(case.members):
        q = oracle_params(oracle_nofma, m.p)
        cells = m.cells0
        for t in range(6):
            got, u, force = dm.reference_step(oracle_nofma, m.p, m.ob, m.body, cells, None, None)
            f = np.array(cells, dtype=np.float64, copy=True)
            oracle_nofma.accelerate_flow(q, f, m.ob)
            want = np.empty_like(f)
            oracle_nofma.timestep(q, f, want, m.ob)
            assert np.array_equal(got, want), (k, t)
            assert np.all(u[m.ob != 0] == 0.0) and np.all(u[m.ob == 0] > 0.0)
            assert force[2] > 0 and force[3] > 0.0
            cells = want


@pytest.mark.parametrize("nx,ny", SHAPES + [(5, 4)])
def test_the_flags_choose_other_operators(lbm, oracle_f64, nx, ny):
    case = dm.make_case(lbm, nx, ny, 3, 1, True, True, True)
    for k, m in enumerate(case.members):
        step = {(trt, opened): dm.reference_step(oracle_f64, m.p, m.ob, m.body, m.cells0, m.magic if trt else None,
                                                 m.open if opened else None)
                for trt in (False, True) for opened in (False, True)}
        for trt in (False, True):
            on, off = step[(trt, True)][0], step[(trt, False)][0]
            assert not np.array_equal(on[:, :, 0], off[:, :, 0]) and not np.array_equal(on[:, :, nx - 1], off[:, :, nx - 1]), k
        for opened in (False, True):
            trt, bgk = step[(True, opened)][0], step[(False, opened)][0]
            apart = float(np.max(np.abs(trt - bgk) / np.abs(bgk)))
            print("%dx%d member %d open %d: the TRT step is up to %.2f %% from the BGK step" % (nx, ny, k, opened, 100.0 * apart))
            assert apart > 1e-3, k
        if (nx, ny) == (5, 4):
            assert all(v[2] is None for v in step.values())

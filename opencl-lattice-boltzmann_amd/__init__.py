"""opencl-lattice-boltzmann_amd — MI355X-native D2Q9-BGK lattice-Boltzmann timestep.

Host-side mirror of the C ABI in include/lbm.h (liblbm_hip.so, hand-written HIP for gfx950).
The product's host is the C program `d2q9-bgk` (host/d2q9-bgk.c); this module is the ctypes
binding used by bench.py, __graft_entry__.py and the tests.  There is NO CPU fallback: loading
fails loudly when the HIP library is missing, and every entry point raises LBMError on a non-zero
return code (the reference's checkError() prints and exits, d2q9-bgk.c:858-866).

The directory name contains '-' and is therefore loaded through `lbm_amd.py` at the repo root
(`import lbm_amd`).
"""
import ctypes
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, os.environ.get("LBM_LIB", "liblbm_hip.so"))  # LBM_LIB: A/B of two builds (tools/ab_two_libs.py)

# every symbol include/lbm.h declares
ABI_SYMBOLS = [
    "lbm_create", "lbm_create_rank", "lbm_comm_id_size", "lbm_comm_get_id", "lbm_upload", "lbm_run",
    "lbm_run_timed", "lbm_sync", "lbm_download", "lbm_steps_done", "lbm_row_range", "lbm_final_state",
    "lbm_reynolds", "lbm_set_option", "lbm_get_option", "lbm_copy_bandwidth", "lbm_valu_rate", "lbm_destroy",
    "lbm_last_error", "lbm_version", "lbm_set_default", "lbm_peer_info_size", "lbm_peer_info", "lbm_connect_peers",
    "lbm_run_profiled", "lbm_upload_obstacles", "lbm_disconnect_peers", "lbm_host_alloc", "lbm_host_free",
    "lbm_ens_create", "lbm_ens_upload", "lbm_ens_run", "lbm_ens_run_timed", "lbm_ens_sync", "lbm_ens_download",
    "lbm_ens_final_state", "lbm_ens_reynolds", "lbm_ens_steps_done", "lbm_ens_members", "lbm_ens_destroy",
    "lbm_steady_run", "lbm_steady_steps",
    "lbm_dp_create", "lbm_dp_upload", "lbm_dp_upload_obstacles", "lbm_dp_run", "lbm_dp_run_timed", "lbm_dp_sync",
    "lbm_dp_download", "lbm_dp_final_state", "lbm_dp_reynolds", "lbm_dp_steps_done", "lbm_dp_set_option",
    "lbm_dp_get_option", "lbm_dp_destroy",
    "lbm_dens_create", "lbm_dens_upload", "lbm_dens_run", "lbm_dens_run_timed", "lbm_dens_sync", "lbm_dens_download",
    "lbm_dens_final_state", "lbm_dens_reynolds", "lbm_dens_steps_done", "lbm_dens_members", "lbm_dens_destroy",
    "lbm_dsteady_run", "lbm_dsteady_steps",
    "lbm_dforce_record", "lbm_dforce", "lbm_dforce_ens_set_option", "lbm_dforce_ens_get_option", "lbm_dforce_ens_record",
    "lbm_dforce_ens",
    "lbm_dbody_set", "lbm_dbody_get", "lbm_dbody_ens_set", "lbm_dbody_ens_get", "lbm_dbody_steady_run",
    "lbm_dtrt_set", "lbm_dtrt_get", "lbm_dtrt_ens_set", "lbm_dtrt_ens_get",
    "lbm_dopen_set", "lbm_dopen_get", "lbm_dopen_ens_set", "lbm_dopen_ens_get",
    "lbm_dwall_set", "lbm_dwall_get", "lbm_dwall_ens_set", "lbm_dwall_ens_get",
    "lbm_dles_set", "lbm_dles_get", "lbm_dles_ens_set", "lbm_dles_ens_get",
    "lbm_ddrive_set", "lbm_ddrive_get", "lbm_ddrive_ens_set", "lbm_ddrive_ens_get",
    "lbm_dscalar_set", "lbm_dscalar_get", "lbm_dscalar_field", "lbm_dscalar_download", "lbm_dscalar_upload",
    "lbm_dscalar_ens_set", "lbm_dscalar_ens_get", "lbm_dscalar_ens_field", "lbm_dscalar_ens_download", "lbm_dscalar_ens_upload",
    "lbm_dbuoy_set", "lbm_dbuoy_get", "lbm_dbuoy_ens_set", "lbm_dbuoy_ens_get",
    "lbm_drecord_set", "lbm_drecord_get", "lbm_drecord",
    "lbm_drecord_ens_set", "lbm_drecord_ens_get", "lbm_drecord_ens", "lbm_drecord_steady_run",
    "lbm_dstats_set", "lbm_dstats_get", "lbm_dstats", "lbm_dstats_ens_set", "lbm_dstats_ens_get", "lbm_dstats_ens",
]

TRANSPORTS = {"auto": 0, "rccl": 1, "copy": 2, "peer": 3}


class LBMError(RuntimeError):
    pass


class Params(ctypes.Structure):
    """lbm_params == the reference's t_param (d2q9-bgk.c:81-92)."""
    _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("max_iters", ctypes.c_int),
                ("reynolds_dim", ctypes.c_int), ("density", ctypes.c_float), ("accel", ctypes.c_float),
                ("omega", ctypes.c_float), ("free_cells_inv", ctypes.c_float)]


class DParams(ctypes.Structure):
    """lbm_dparams: the fields of Params with the four reals in double, as the reference's fp64 ancestor held them."""
    _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("max_iters", ctypes.c_int),
                ("reynolds_dim", ctypes.c_int), ("density", ctypes.c_double), ("accel", ctypes.c_double),
                ("omega", ctypes.c_double), ("free_cells_inv", ctypes.c_double)]


def build_library(verbose=False):
    """Compile liblbm_hip.so and the d2q9-bgk host for gfx950 (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.run(["make", "-C", ROOT, "-j4", "all"], check=True, stdout=out)


_lib = None


def load_library():
    """dlopen liblbm_hip.so and declare the prototypes of include/lbm.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LBMError("HIP library %s is missing: run `make` (or __graft_entry__.build()); "
                       "there is no CPU fallback" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, ci, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p
    L.lbm_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(Params), vp, ci, ctypes.POINTER(ci)]
    L.lbm_create_rank.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(Params), vp, ci, ci, ci, vp]
    L.lbm_comm_id_size.restype = ctypes.c_size_t
    L.lbm_comm_get_id.argtypes = [vp]
    L.lbm_upload.argtypes = [vp, vp]
    L.lbm_upload_obstacles.argtypes = [vp, vp]
    L.lbm_run.argtypes = [vp, ci]
    L.lbm_run_timed.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double)]
    L.lbm_run_profiled.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double)]
    L.lbm_sync.argtypes = [vp]
    L.lbm_download.argtypes = [vp, vp, vp]
    L.lbm_steps_done.argtypes = [vp]
    L.lbm_row_range.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.lbm_final_state.argtypes = [vp, vp, vp, vp, vp]
    L.lbm_reynolds.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.lbm_set_option.argtypes = [vp, cp, ctypes.c_long]
    L.lbm_get_option.argtypes = [vp, cp, ctypes.POINTER(ctypes.c_long)]
    L.lbm_copy_bandwidth.argtypes = [ctypes.c_size_t, ci, ctypes.POINTER(ctypes.c_double)]
    L.lbm_valu_rate.argtypes = [ci, ctypes.POINTER(ctypes.c_double)]
    L.lbm_set_default.argtypes = [cp, ctypes.c_long]
    L.lbm_peer_info_size.restype = ctypes.c_size_t
    L.lbm_peer_info.argtypes = [vp, vp]
    L.lbm_connect_peers.argtypes = [vp, vp, vp]
    L.lbm_disconnect_peers.argtypes = [vp]
    L.lbm_host_alloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    L.lbm_host_free.argtypes = [vp]
    L.lbm_destroy.argtypes = [vp]
    L.lbm_destroy.restype = None
    L.lbm_ens_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(Params), vp, ci]
    L.lbm_ens_upload.argtypes = [vp, vp]
    L.lbm_ens_run.argtypes = [vp, ci]
    L.lbm_ens_run_timed.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double)]
    L.lbm_ens_sync.argtypes = [vp]
    L.lbm_ens_download.argtypes = [vp, vp, vp]
    L.lbm_ens_final_state.argtypes = [vp, vp, vp, vp, vp]
    L.lbm_ens_reynolds.argtypes = [vp, vp]
    L.lbm_ens_steps_done.argtypes = [vp]
    L.lbm_ens_members.argtypes = [vp]
    L.lbm_ens_destroy.argtypes = [vp]
    L.lbm_ens_destroy.restype = None
    L.lbm_steady_run.argtypes = [vp, ci, ci, ctypes.c_double]
    L.lbm_steady_steps.argtypes = [vp, vp, vp]
    L.lbm_dp_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(DParams), vp]
    L.lbm_dp_upload.argtypes = [vp, vp]
    L.lbm_dp_upload_obstacles.argtypes = [vp, vp]
    L.lbm_dp_run.argtypes = [vp, ci]
    L.lbm_dp_run_timed.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double)]
    L.lbm_dp_sync.argtypes = [vp]
    L.lbm_dp_download.argtypes = [vp, vp, vp]
    L.lbm_dp_final_state.argtypes = [vp, vp, vp, vp, vp]
    L.lbm_dp_reynolds.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.lbm_dp_steps_done.argtypes = [vp]
    L.lbm_dp_set_option.argtypes = [vp, cp, ctypes.c_long]
    L.lbm_dp_get_option.argtypes = [vp, cp, ctypes.POINTER(ctypes.c_long)]
    L.lbm_dp_destroy.argtypes = [vp]
    L.lbm_dp_destroy.restype = None
    L.lbm_dens_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(DParams), vp, ci]
    L.lbm_dens_upload.argtypes = [vp, vp]
    L.lbm_dens_run.argtypes = [vp, ci]
    L.lbm_dens_run_timed.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double)]
    L.lbm_dens_sync.argtypes = [vp]
    L.lbm_dens_download.argtypes = [vp, vp, vp]
    L.lbm_dens_final_state.argtypes = [vp, vp, vp, vp, vp]
    L.lbm_dens_reynolds.argtypes = [vp, vp]
    L.lbm_dens_steps_done.argtypes = [vp]
    L.lbm_dens_members.argtypes = [vp]
    L.lbm_dens_destroy.argtypes = [vp]
    L.lbm_dens_destroy.restype = None
    L.lbm_dsteady_run.argtypes = [vp, ci, ci, ctypes.c_double]
    L.lbm_dsteady_steps.argtypes = [vp, vp, vp]
    L.lbm_dforce_record.argtypes = [vp, vp, vp]
    L.lbm_dforce.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.lbm_dforce_ens_set_option.argtypes = [vp, cp, ctypes.c_long]
    L.lbm_dforce_ens_get_option.argtypes = [vp, cp, ctypes.POINTER(ctypes.c_long)]
    L.lbm_dforce_ens_record.argtypes = [vp, vp, vp]
    L.lbm_dforce_ens.argtypes = [vp, vp, vp]
    L.lbm_dbody_set.argtypes = [vp, vp]
    L.lbm_dbody_get.argtypes = [vp, vp]
    L.lbm_dbody_ens_set.argtypes = [vp, vp]
    L.lbm_dbody_ens_get.argtypes = [vp, vp]
    L.lbm_dbody_steady_run.argtypes = [vp, ci, ci, ctypes.c_double]
    L.lbm_dtrt_set.argtypes = [vp, ctypes.c_double]
    L.lbm_dtrt_get.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.lbm_dtrt_ens_set.argtypes = [vp, vp]
    L.lbm_dtrt_ens_get.argtypes = [vp, vp, vp]
    L.lbm_dopen_set.argtypes = [vp, vp, ctypes.c_double]
    L.lbm_dopen_get.argtypes = [vp, ctypes.POINTER(ci), vp, ctypes.POINTER(ctypes.c_double)]
    L.lbm_dopen_ens_set.argtypes = [vp, vp, vp]
    L.lbm_dopen_ens_get.argtypes = [vp, ctypes.POINTER(ci), vp, vp]
    L.lbm_dwall_set.argtypes = [vp, vp, vp, ctypes.c_double]
    L.lbm_dwall_get.argtypes = [vp, ctypes.POINTER(ci), vp, vp, ctypes.POINTER(ctypes.c_double)]
    L.lbm_dwall_ens_set.argtypes = [vp, vp, vp, vp]
    L.lbm_dwall_ens_get.argtypes = [vp, ctypes.POINTER(ci), vp, vp, vp]
    L.lbm_dles_set.argtypes = [vp, ctypes.c_double]
    L.lbm_dles_get.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.lbm_dles_ens_set.argtypes = [vp, vp]
    L.lbm_dles_ens_get.argtypes = [vp, vp, vp]
    L.lbm_ddrive_set.argtypes = [vp, ctypes.c_double, ctypes.c_double]
    L.lbm_ddrive_get.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.lbm_ddrive_ens_set.argtypes = [vp, vp]
    L.lbm_ddrive_ens_get.argtypes = [vp, ctypes.POINTER(ci), vp]
    L.lbm_dscalar_set.argtypes = [vp, ctypes.c_double, vp, vp, vp]
    L.lbm_dscalar_get.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.lbm_dscalar_field.argtypes = [vp, vp]
    L.lbm_dscalar_download.argtypes = [vp, vp]
    L.lbm_dscalar_upload.argtypes = [vp, vp]
    L.lbm_dscalar_ens_set.argtypes = [vp, vp, vp, vp, vp]
    L.lbm_dscalar_ens_get.argtypes = [vp, ctypes.POINTER(ci), vp, vp]
    L.lbm_dscalar_ens_field.argtypes = [vp, vp]
    L.lbm_dscalar_ens_download.argtypes = [vp, vp]
    L.lbm_dscalar_ens_upload.argtypes = [vp, vp]
    L.lbm_dbuoy_set.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    L.lbm_dbuoy_get.argtypes = [vp, ctypes.POINTER(ci), vp, ctypes.POINTER(ctypes.c_double)]
    L.lbm_dbuoy_ens_set.argtypes = [vp, vp]
    L.lbm_dbuoy_ens_get.argtypes = [vp, ctypes.POINTER(ci), vp]
    L.lbm_drecord_set.argtypes = [vp, ci]
    L.lbm_drecord_get.argtypes = [vp, ctypes.POINTER(ci)]
    L.lbm_drecord.argtypes = [vp, vp, vp, vp]
    L.lbm_drecord_ens_set.argtypes = [vp, ci]
    L.lbm_drecord_ens_get.argtypes = [vp, ctypes.POINTER(ci)]
    L.lbm_drecord_ens.argtypes = [vp, vp, vp, vp]
    L.lbm_drecord_steady_run.argtypes = [vp, ci, ci, ctypes.c_double, ci]
    L.lbm_dstats_set.argtypes = [vp, ci]
    L.lbm_dstats_get.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.lbm_dstats.argtypes = [vp, vp]
    L.lbm_dstats_ens_set.argtypes = [vp, ci]
    L.lbm_dstats_ens_get.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.lbm_dstats_ens.argtypes = [vp, vp]
    L.lbm_last_error.restype = cp
    L.lbm_version.restype = cp
    _lib = L
    return L


def _check(rc, what):
    if rc != 0:
        raise LBMError("%s failed (code %d): %s" % (what, rc, load_library().lbm_last_error().decode()))


def _make_params(ptype, real, nx, ny, max_iters, reynolds_dim, density, accel, omega, obstacles):
    """a `ptype` (Params / DParams) of these run constants; free_cells_inv = 1 / free_cells in `real`, the numpy type of
    ptype's reals (inf for a grid without a free cell, as the reference's division gives)"""
    p = ptype()
    p.nx, p.ny, p.max_iters, p.reynolds_dim = nx, ny, max_iters, reynolds_dim
    p.density, p.accel, p.omega = float(density), float(accel), float(omega)
    free_cells = nx * ny if obstacles is None else int(obstacles.size - np.count_nonzero(obstacles))
    with np.errstate(divide="ignore"):
        p.free_cells_inv = real(1.0) / real(free_cells)
    return p


def make_params(nx, ny, max_iters, reynolds_dim=10, density=0.1, accel=0.005, omega=1.85, obstacles=None):
    """Run constants; free_cells_inv from the mask as in d2q9-bgk.c:583-591."""
    return _make_params(Params, np.float32, nx, ny, max_iters, reynolds_dim, density, accel, omega, obstacles)


def _parse_inputs(paramfile, obstaclefile):
    """the reference's two input files (d2q9-bgk.c:466-492, 553-591): (nx, ny, max_iters, reynolds_dim), the three reals as
    Python floats (double), and the mask"""
    with open(paramfile) as f:
        tok = f.read().split()
    if len(tok) < 7:
        raise ValueError("could not read param file: %s" %
                         ["nx", "ny", "maxIters", "reynolds_dim", "density", "accel", "omega"][len(tok)])
    nx, ny, max_iters, reynolds_dim = (int(t) for t in tok[:4])
    density, accel, omega = (float(t) for t in tok[4:7])
    obstacles = np.zeros((ny, nx), dtype=np.int32)
    with open(obstaclefile) as f:
        vals = f.read().split()
    if len(vals) % 3:
        raise ValueError("expected 3 values per line in obstacle file")
    if vals:
        tri = np.array(vals, dtype=np.int64).reshape(-1, 3)
        if np.any(tri[:, 0] < 0) or np.any(tri[:, 0] > nx - 1):
            raise ValueError("obstacle x-coord out of range")
        if np.any(tri[:, 1] < 0) or np.any(tri[:, 1] > ny - 1):
            raise ValueError("obstacle y-coord out of range")
        if np.any(tri[:, 2] != 1):
            raise ValueError("obstacle blocked value should be 1")
        obstacles[tri[:, 1], tri[:, 0]] = 1
    return (nx, ny, max_iters, reynolds_dim), (density, accel, omega), obstacles


def read_inputs(paramfile, obstaclefile):
    """Parse the reference's two input files (d2q9-bgk.c:466-492, 553-591) into (Params, mask)."""
    ints, reals, obstacles = _parse_inputs(paramfile, obstaclefile)
    return make_params(*ints, *reals, obstacles), obstacles


def make_dparams(nx, ny, max_iters, reynolds_dim=10, density=0.1, accel=0.005, omega=1.85, obstacles=None):
    """Run constants of a double-precision context: the reals as given (the fp64 literals, never widened floats),
    free_cells_inv = 1.0 / free_cells in double (inf for a grid without a free cell, as the reference's division gives)."""
    return _make_params(DParams, np.float64, nx, ny, max_iters, reynolds_dim, density, accel, omega, obstacles)


def read_inputs_double(paramfile, obstaclefile):
    """The reference's two input files as its fp64 ancestor read them: (DParams, mask) with density, accel and omega parsed
    as double and free_cells_inv = 1.0 / free_cells in double."""
    ints, reals, obstacles = _parse_inputs(paramfile, obstaclefile)
    return make_dparams(*ints, *reals, obstacles), obstacles


def _write_values(final_state_path, av_vels_path, obstacles, fields, av):
    """final_state.dat and av_vels.dat in the reference's formats (d2q9-bgk.c:835, 848-851)"""
    ny, nx = obstacles.shape
    ux, uy, u, pr = fields
    yy, xx = np.mgrid[0:ny, 0:nx]
    cols = np.stack([xx.ravel(), yy.ravel(), ux.ravel(), uy.ravel(), u.ravel(), pr.ravel(), obstacles.ravel()], axis=1)
    np.savetxt(final_state_path, cols, fmt=["%d", "%d", "%.12E", "%.12E", "%.12E", "%.12E", "%d"])
    with open(av_vels_path, "w") as f:
        for i, v in enumerate(av):
            f.write("%d:\t%.12E\n" % (i, v))


# ---- row partition: the host-side geometry of csrc/lbm_hip.cpp (split_rows, build_slab, exchange_halos) ----

# distributions that cross a slab edge in the pull scheme: a cell reads f2,f5,f6 from the row below and
# f4,f7,f8 from the row above (kernels.cl:104-112), so a slab sends its top row's 2,5,6 north and its
# bottom row's 4,7,8 south
HALO_PLANES = {"to_north": [2, 5, 6], "to_south": [4, 7, 8]}


def slab_rows(ny, nslabs, index):
    """(first global row, row count) of slab `index` of `nslabs`: contiguous rows, sizes differ by <= 1."""
    base, rem = divmod(ny, nslabs)
    return index * base + min(index, rem), base + (1 if index < rem else 0)


def ring_neighbours(nslabs, index):
    """(south, north) neighbours on the periodic ring of slabs (the grid wraps in y, kernels.cl:91-93)."""
    return (index + nslabs - 1) % nslabs, (index + 1) % nslabs


def accel_row_local(ny, y0, rows):
    """local index of the accelerated global row ny-2 (kernels.cl:18) inside a slab, or -1."""
    ar = ny - 2
    return ar - y0 if y0 <= ar < y0 + rows else -1


def valu_rate_tera(launches=40):
    """issue rate of packed fp32 FMAs in 1e12 lane-instructions per second (the roofline of the issue-bound kernels)"""
    g = ctypes.c_double(0.0)
    _check(load_library().lbm_valu_rate(launches, ctypes.byref(g)), "lbm_valu_rate")
    return g.value


def copy_bandwidth_gbps(nbytes=1 << 30, iters=20):
    """Measured float4 streaming-copy rate (read + write bytes per second) — the roofline denominator."""
    g = ctypes.c_double()
    _check(load_library().lbm_copy_bandwidth(nbytes, iters, ctypes.byref(g)), "lbm_copy_bandwidth")
    return g.value


def set_default(key, value):
    """Process-wide default for contexts created afterwards (lbm_set_default): force_halo, halo_depth, transport
    (number or one of TRANSPORTS), lanes_out."""
    if key == "transport" and isinstance(value, str):
        value = TRANSPORTS[value]
    _check(load_library().lbm_set_default(key.encode(), int(value)), "lbm_set_default(%s)" % key)


class HostBuffer:
    """Page-locked host memory from lbm_host_alloc, seen as a numpy array (`.array`): a read-back target that device -> host
    copies fill at the PCIe rate.  Free with close() (or leave it to the garbage collector)."""

    def __init__(self, shape, dtype=np.float32):
        self.lib = load_library()
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = ctypes.c_void_p()
        _check(self.lib.lbm_host_alloc(ctypes.byref(self.ptr), nbytes), "lbm_host_alloc")
        raw = (ctypes.c_char * nbytes).from_address(self.ptr.value)
        self.array = np.frombuffer(raw, dtype=dtype).reshape(shape)

    def close(self):
        if self.ptr:
            self.array = None
            self.lib.lbm_host_free(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_id():
    """RCCL unique id blob for lbm_create_rank (produce on one rank, broadcast to the others)."""
    L = load_library()
    buf = ctypes.create_string_buffer(L.lbm_comm_id_size())
    _check(L.lbm_comm_get_id(buf), "lbm_comm_get_id")
    return buf.raw


class _Handle:
    """What the four families of include/lbm.h have in common beyond their names: a handle that `<prefix>_destroy` frees, and
    `<prefix>_run`, `_run_timed`, `_sync` and `_steps_done` on it.  A class names its family in `_prefix` and the attribute
    that holds its handle in `_handle` (contexts keep theirs in `ctx`, ensembles in `ens`)."""
    _prefix = None
    _handle = None

    def _call(self, name, *args):
        """<prefix>_<name>(handle, *args), raising LBMError on a non-zero return code"""
        symbol = "%s_%s" % (self._prefix, name)
        _check(getattr(self.lib, symbol)(getattr(self, self._handle), *args), symbol)

    def run(self, nsteps):
        self._call("run", nsteps)

    def run_timed(self, nsteps):
        """Runs nsteps and returns the HIP-event time of the step loop in milliseconds."""
        ms = ctypes.c_double()
        self._call("run_timed", nsteps, ctypes.byref(ms))
        return ms.value

    def sync(self):
        self._call("sync")

    @property
    def steps_done(self):
        return getattr(self.lib, self._prefix + "_steps_done")(getattr(self, self._handle))

    def close(self):
        if getattr(self, self._handle):
            getattr(self.lib, self._prefix + "_destroy")(getattr(self, self._handle))
            setattr(self, self._handle, ctypes.c_void_p())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LBM(_Handle):
    """A simulation context (lbm_ctx).  Mirrors the call sequence of the reference's main()
    (d2q9-bgk.c:194-277): create -> upload -> run -> sync -> download -> destroy."""
    _prefix, _handle = "lbm", "ctx"

    def __init__(self, params, obstacles, devices=None, rank=None, nranks=None, device=0, comm=None):
        self.lib = load_library()
        self.params = params
        self.nx, self.ny = params.nx, params.ny
        obst = np.ascontiguousarray(obstacles, dtype=np.int32)
        assert obst.shape == (params.ny, params.nx)
        self.obstacles = obst
        self.ctx = ctypes.c_void_p()
        if rank is not None:
            cid = ctypes.create_string_buffer(comm, len(comm)) if comm is not None else None
            _check(self.lib.lbm_create_rank(ctypes.byref(self.ctx), ctypes.byref(params), obst.ctypes.data,
                                            rank, nranks, device, cid), "lbm_create_rank")
        elif devices is None:
            _check(self.lib.lbm_create(ctypes.byref(self.ctx), ctypes.byref(params), obst.ctypes.data, 1, None),
                   "lbm_create")
        else:
            arr = (ctypes.c_int * len(devices))(*devices)
            _check(self.lib.lbm_create(ctypes.byref(self.ctx), ctypes.byref(params), obst.ctypes.data,
                                       len(devices), arr), "lbm_create")

    def upload(self, cells=None):
        if cells is None:
            _check(self.lib.lbm_upload(self.ctx, None), "lbm_upload")
        else:
            c = np.ascontiguousarray(cells, dtype=np.float32)
            assert c.shape == (9, self.ny, self.nx)
            _check(self.lib.lbm_upload(self.ctx, c.ctypes.data), "lbm_upload")

    def upload_obstacles(self, obstacles):
        """the obstacle map once more (d2q9-bgk.c:205-209); same shape as at creation"""
        ob = np.ascontiguousarray(obstacles, dtype=np.int32)
        assert ob.shape == (self.ny, self.nx)
        _check(self.lib.lbm_upload_obstacles(self.ctx, ob.ctypes.data), "lbm_upload_obstacles")
        self.obstacles = ob

    def run_profiled(self, nsteps):
        """Runs nsteps with timing events around every launch of the first slab; dict of mean microseconds."""
        st = (ctypes.c_double * 8)()
        _check(self.lib.lbm_run_profiled(self.ctx, nsteps, st), "lbm_run_profiled")
        return {"sets": int(st[0]), "steps_per_set": st[1], "edge_us": st[2], "exchange_us": st[3], "interior_us": st[4],
                "set_period_us": st[5], "interior_start_lag_us": st[6],
                "transport": {0: "none", 1: "rccl", 2: "copy", 3: "peer"}.get(int(st[7]), "?")}

    def row_range(self):
        y0, y1 = ctypes.c_int(), ctypes.c_int()
        _check(self.lib.lbm_row_range(self.ctx, ctypes.byref(y0), ctypes.byref(y1)), "lbm_row_range")
        return y0.value, y1.value

    def download(self, cells=True, av_vels=True):
        """Returns (cells float32[9,ny,nx] or None, av_vels float32[steps_done] or None)."""
        c = np.zeros((9, self.ny, self.nx), dtype=np.float32) if cells else None
        a = np.zeros(max(self.steps_done, 1), dtype=np.float32) if av_vels else None
        _check(self.lib.lbm_download(self.ctx, c.ctypes.data if cells else None,
                                     a.ctypes.data if av_vels else None), "lbm_download")
        return c, (a[:self.steps_done] if av_vels else None)

    def final_state(self, out=None):
        """(u_x, u_y, u, pressure), each float32[ny,nx] — the columns of final_state.dat.  `out`: a float32[4,ny,nx] array
        to fill instead of fresh ones (e.g. HostBuffer((4, ny, nx)).array: page-locked)."""
        if out is not None:
            assert out.shape == (4, self.ny, self.nx) and out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
            outs = [out[i] for i in range(4)]
        else:
            outs = [np.zeros((self.ny, self.nx), dtype=np.float32) for _ in range(4)]
        _check(self.lib.lbm_final_state(self.ctx, *[o.ctypes.data for o in outs]), "lbm_final_state")
        return outs

    def reynolds(self):
        r = ctypes.c_float()
        _check(self.lib.lbm_reynolds(self.ctx, ctypes.byref(r)), "lbm_reynolds")
        return r.value

    def peer_info(self):
        """This rank's peer descriptor (bytes) for lbm_connect_peers on its ring neighbours."""
        buf = ctypes.create_string_buffer(self.lib.lbm_peer_info_size())
        _check(self.lib.lbm_peer_info(self.ctx, buf), "lbm_peer_info")
        return buf.raw

    def connect_peers(self, south_info, north_info):
        """Descriptors of ranks (rank-1) and (rank+1) mod nranks: switches the halo transport to peer stores."""
        so = ctypes.create_string_buffer(south_info, len(south_info))
        no = ctypes.create_string_buffer(north_info, len(north_info))
        _check(self.lib.lbm_connect_peers(self.ctx, so, no), "lbm_connect_peers")

    def disconnect_peers(self):
        """Unmap the neighbours' grids.  Between processes: every rank calls this, then a barrier, then close() — memory that
        another process still has mapped must not be freed."""
        _check(self.lib.lbm_disconnect_peers(self.ctx), "lbm_disconnect_peers")

    def set_option(self, key, value):
        _check(self.lib.lbm_set_option(self.ctx, key.encode(), int(value)), "lbm_set_option(%s)" % key)

    def get_option(self, key):
        v = ctypes.c_long()
        _check(self.lib.lbm_get_option(self.ctx, key.encode(), ctypes.byref(v)), "lbm_get_option(%s)" % key)
        return v.value

    def write_values(self, final_state_path="final_state.dat", av_vels_path="av_vels.dat"):
        """The two output files in the reference's format (d2q9-bgk.c:835,848-851)."""
        ux, uy, u, pr = self.final_state()
        _, av = self.download(cells=False)
        yy, xx = np.mgrid[0:self.ny, 0:self.nx]
        cols = np.stack([xx.ravel(), yy.ravel(), ux.ravel(), uy.ravel(), u.ravel(), pr.ravel(),
                         self.obstacles.ravel()], axis=1)
        np.savetxt(final_state_path, cols, fmt=["%d", "%d", "%.12E", "%.12E", "%.12E", "%.12E", "%d"])
        with open(av_vels_path, "w") as f:
            for i, v in enumerate(av):
                f.write("%d:\t%.12E\n" % (i, v))


class _Stats:
    """The running statistics of the double-precision families (include/lbm.h, "Running statistics"): the four methods LBMDouble
    and EnsembleDouble share.  A class names its entry points' prefix in `_stats` and the leading axes of its arrays in
    `_stats_lead()`."""

    def set_stats(self, every):
        """Statistics on (lbm_dstats_set / lbm_dstats_ens_set): a sample of u_x, u_y, pressure and their three products per cell
        every `every` steps, counted from the step count as it stands; 0 = off.  Accepted between runs at any step count; setting
        again starts anew.  The uploads keep the setting and start anew; steady runs are refused while it is on."""
        _check(getattr(self.lib, self._stats + "_set")(getattr(self, self._handle), int(every)), self._stats + "_set")

    def stats_state(self):
        """(every, origin, samples), or None while the statistics are off"""
        every, origin, samples = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(getattr(self.lib, self._stats + "_get")(getattr(self, self._handle), ctypes.byref(every), ctypes.byref(origin),
                                                       ctypes.byref(samples)), self._stats + "_get")
        return (every.value, origin.value, samples.value) if every.value else None

    def stats_sums(self):
        """The raw sums, float64[6, ny, nx] (an ensemble: [n, 6, ny, nx]): S[0..5] of u_x, u_y, pressure, u_x u_x, u_y u_y, u_x u_y"""
        sums = np.zeros(self._stats_lead() + (6, self.ny, self.nx), dtype=np.float64)
        _check(getattr(self.lib, self._stats)(getattr(self, self._handle), sums.ctypes.data), self._stats)
        return sums

    def stats(self):
        """{"samples", "u_x", "u_y", "pressure", "uxux", "uyuy", "uxuy"}: the count, the time means S[v] / samples and the
        covariances (Reynolds stresses) S[3] / samples - u_x * u_x and so on, float64[ny, nx] each (an ensemble: [n, ny, nx]),
        formed here in numpy from stats_sums().  Zero samples: LBMError.

        The caveat of raw sums: a covariance loses as many digits as the variance is small against the squared mean.  In fp64 this
        leaves about 10 digits for fluctuations of 1e-3 on a mean of 0.1; a variance may round below zero, by rounding alone."""
        state = self.stats_state()
        if state is None or state[2] == 0:
            raise LBMError("stats(): no samples yet (set_stats(every), then run past a sample point)")
        samples = state[2]
        S = np.moveaxis(self.stats_sums(), -3, 0)
        u_x = S[0] / samples
        u_y = S[1] / samples
        pressure = S[2] / samples
        uxux = S[3] / samples - u_x * u_x
        uyuy = S[4] / samples - u_y * u_y
        uxuy = S[5] / samples - u_x * u_y
        return {"samples": samples, "u_x": u_x, "u_y": u_y, "pressure": pressure, "uxux": uxux, "uyuy": uyuy, "uxuy": uxuy}


class LBMDouble(_Handle, _Stats):
    """A double-precision context (lbm_dp): one grid on the current device in fp64, the precision of the reference's golden
    files.  Mirrors LBM with double in place of float: create -> upload -> run -> sync -> download -> destroy.  `params`:
    DParams (make_dparams, read_inputs_double); `obstacles`: int32[ny, nx]."""
    _prefix, _handle = "lbm_dp", "ctx"
    _stats = "lbm_dstats"

    def _stats_lead(self):
        return ()

    def __init__(self, params, obstacles):
        self.lib = load_library()
        if not isinstance(params, DParams):
            raise LBMError("LBMDouble takes DParams (make_dparams / read_inputs_double), not %s" % type(params).__name__)
        self.params = params
        self.nx, self.ny = params.nx, params.ny
        obst = np.ascontiguousarray(obstacles, dtype=np.int32)
        assert obst.shape == (params.ny, params.nx)
        self.obstacles = obst
        self.ctx = ctypes.c_void_p()
        _check(self.lib.lbm_dp_create(ctypes.byref(self.ctx), ctypes.byref(params), obst.ctypes.data), "lbm_dp_create")

    def upload(self, cells=None):
        """cells float64[9, ny, nx]; None = the rest state from params.density, on the device"""
        if cells is None:
            _check(self.lib.lbm_dp_upload(self.ctx, None), "lbm_dp_upload")
        else:
            c = np.ascontiguousarray(cells, dtype=np.float64)
            assert c.shape == (9, self.ny, self.nx)
            _check(self.lib.lbm_dp_upload(self.ctx, c.ctypes.data), "lbm_dp_upload")

    def upload_obstacles(self, obstacles):
        """the obstacle map once more (d2q9-bgk.c:205-209); same shape as at creation"""
        ob = np.ascontiguousarray(obstacles, dtype=np.int32)
        assert ob.shape == (self.ny, self.nx)
        _check(self.lib.lbm_dp_upload_obstacles(self.ctx, ob.ctypes.data), "lbm_dp_upload_obstacles")
        self.obstacles = ob

    def download(self, cells=True, av_vels=True):
        """Returns (cells float64[9,ny,nx] or None, av_vels float64[steps_done] or None)."""
        steps = self.steps_done
        c = np.zeros((9, self.ny, self.nx), dtype=np.float64) if cells else None
        a = np.zeros(max(steps, 1), dtype=np.float64) if av_vels else None
        _check(self.lib.lbm_dp_download(self.ctx, c.ctypes.data if cells else None,
                                        a.ctypes.data if av_vels else None), "lbm_dp_download")
        return c, (a[:steps] if av_vels else None)

    def final_state(self):
        """(u_x, u_y, u, pressure), each float64[ny,nx] — the columns of final_state.dat."""
        outs = [np.zeros((self.ny, self.nx), dtype=np.float64) for _ in range(4)]
        _check(self.lib.lbm_dp_final_state(self.ctx, *[o.ctypes.data for o in outs]), "lbm_dp_final_state")
        return outs

    def reynolds(self):
        r = ctypes.c_double()
        _check(self.lib.lbm_dp_reynolds(self.ctx, ctypes.byref(r)), "lbm_dp_reynolds")
        return r.value

    def set_option(self, key, value):
        _check(self.lib.lbm_dp_set_option(self.ctx, key.encode(), int(value)), "lbm_dp_set_option(%s)" % key)

    def get_option(self, key):
        v = ctypes.c_long()
        _check(self.lib.lbm_dp_get_option(self.ctx, key.encode(), ctypes.byref(v)), "lbm_dp_get_option(%s)" % key)
        return v.value

    def force(self):
        """(F_x, F_y): the momentum-exchange force on the blocked cells of the current state as the next step would stream
        it (lbm_dforce), in lattice units per step.  The state is not modified."""
        fx, fy = ctypes.c_double(), ctypes.c_double()
        _check(self.lib.lbm_dforce(self.ctx, ctypes.byref(fx), ctypes.byref(fy)), "lbm_dforce")
        return fx.value, fy.value

    def set_body(self, body):
        """The blocked cells whose links count in the force (lbm_dbody_set): int32[ny, nx], non-zero = counts; None = every
        blocked cell again.  With "force" on only before the first step."""
        if body is None:
            _check(self.lib.lbm_dbody_set(self.ctx, None), "lbm_dbody_set")
        else:
            b = np.ascontiguousarray(body, dtype=np.int32)
            assert b.shape == (self.ny, self.nx)
            _check(self.lib.lbm_dbody_set(self.ctx, b.ctypes.data), "lbm_dbody_set")

    def body(self):
        """int32[ny, nx]: 1 where a blocked cell counts in the force, else 0 (lbm_dbody_get)"""
        b = np.zeros((self.ny, self.nx), dtype=np.int32)
        _check(self.lib.lbm_dbody_get(self.ctx, b.ctypes.data), "lbm_dbody_get")
        return b

    def set_trt(self, magic):
        """The collision operator (lbm_dtrt_set): magic > 0 = two relaxation times with that magic parameter (3/16: a straight
        bounce-back wall exactly half-way, 1/4: the most stable), 0.0 = BGK, the default.  Only before the first step."""
        _check(self.lib.lbm_dtrt_set(self.ctx, float(magic)), "lbm_dtrt_set")

    def trt(self):
        """(magic, omega_minus): the magic parameter in force (0.0: BGK) and the second relaxation rate, omega itself under
        BGK (lbm_dtrt_get)"""
        magic, om = ctypes.c_double(), ctypes.c_double()
        _check(self.lib.lbm_dtrt_get(self.ctx, ctypes.byref(magic), ctypes.byref(om)), "lbm_dtrt_get")
        return magic.value, om.value

    def set_open(self, u_in, rho_out=None):
        """Open boundaries (lbm_dopen_set): u_in float64[ny], the inlet velocity of every row on column 0, and rho_out, the
        outlet density on column nx - 1; set_open(None) = periodic and accelerated, the default.  Only before the first step."""
        if u_in is None:
            _check(self.lib.lbm_dopen_set(self.ctx, None, 0.0), "lbm_dopen_set")
            return
        u = np.ascontiguousarray(u_in, dtype=np.float64)
        assert u.shape == (self.ny,)
        _check(self.lib.lbm_dopen_set(self.ctx, u.ctypes.data, float(rho_out)), "lbm_dopen_set")

    def open(self):
        """(u_in float64[ny], rho_out) while open boundaries are on, None while they are off (lbm_dopen_get)"""
        on, rho = ctypes.c_int(), ctypes.c_double()
        u = np.zeros(self.ny, dtype=np.float64)
        _check(self.lib.lbm_dopen_get(self.ctx, ctypes.byref(on), u.ctypes.data, ctypes.byref(rho)), "lbm_dopen_get")
        return (u, rho.value) if on.value else None

    def set_wall(self, u_x, u_y, rho_wall=None):
        """Moving walls (lbm_dwall_set): u_x, u_y float64[ny, nx], the wall velocity of every blocked cell (zero on fluid cells),
        and rho_wall, the wall density (None: params.density); set_wall(None, None) = every wall at rest, the default.  Only
        before the first step."""
        if u_x is None and u_y is None:
            _check(self.lib.lbm_dwall_set(self.ctx, None, None, 0.0), "lbm_dwall_set")
            return
        ux = None if u_x is None else np.ascontiguousarray(u_x, dtype=np.float64)
        uy = None if u_y is None else np.ascontiguousarray(u_y, dtype=np.float64)
        assert all(u is None or u.shape == (self.ny, self.nx) for u in (ux, uy))
        rho = self.params.density if rho_wall is None else float(rho_wall)
        _check(self.lib.lbm_dwall_set(self.ctx, None if ux is None else ux.ctypes.data, None if uy is None else uy.ctypes.data, rho),
               "lbm_dwall_set")

    def wall(self):
        """(u_x float64[ny, nx], u_y float64[ny, nx], rho_wall) while wall velocities are on, None while they are off
        (lbm_dwall_get)"""
        on, rho = ctypes.c_int(), ctypes.c_double()
        ux, uy = (np.zeros((self.ny, self.nx), dtype=np.float64) for _ in range(2))
        _check(self.lib.lbm_dwall_get(self.ctx, ctypes.byref(on), ux.ctypes.data, uy.ctypes.data, ctypes.byref(rho)), "lbm_dwall_get")
        return (ux, uy, rho.value) if on.value else None

    def set_les(self, c):
        """Subgrid viscosity (lbm_dles_set): c > 0 = the Smagorinsky model with that constant (0.1 .. 0.2 is usual), every fluid
        cell relaxes with its own rate; 0.0 = off, the default.  Only before the first step."""
        _check(self.lib.lbm_dles_set(self.ctx, float(c)), "lbm_dles_set")

    def les(self):
        """(c, les_k): the Smagorinsky constant in force (0.0: off) and (18 sqrt 2) c^2 as the library computes it
        (lbm_dles_get)"""
        c, k = ctypes.c_double(), ctypes.c_double()
        _check(self.lib.lbm_dles_get(self.ctx, ctypes.byref(c), ctypes.byref(k)), "lbm_dles_get")
        return c.value, k.value

    def set_drive(self, f):
        """Body force (lbm_ddrive_set): f = (F_x, F_y), a constant force density per cell volume that every fluid cell takes up
        by Guo forcing; (0, 0) = off, the default.  Only before the first step."""
        f_x, f_y = f
        _check(self.lib.lbm_ddrive_set(self.ctx, float(f_x), float(f_y)), "lbm_ddrive_set")

    def drive(self):
        """(F_x, F_y): the body force in force, (0.0, 0.0) while it is off (lbm_ddrive_get)"""
        f_x, f_y = ctypes.c_double(), ctypes.c_double()
        _check(self.lib.lbm_ddrive_get(self.ctx, ctypes.byref(f_x), ctypes.byref(f_y)), "lbm_ddrive_get")
        return f_x.value, f_y.value

    def set_scalar(self, D, c0=0.0, wall=None, inlet=None):
        """Passive scalar (lbm_dscalar_set): D > 0 = a scalar of that diffusivity, started from the field c0 (float64[ny, nx] or one
        value); wall float64[ny, nx], the value a blocked cell is held at, NaN = insulating (None: all insulating); inlet
        float64[ny] or one value, the inlet value with open boundaries on (None: zeros).  set_scalar(None) or 0.0 = off, the
        default.  Between runs at any step count."""
        if D is None or float(D) == 0.0:
            _check(self.lib.lbm_dscalar_set(self.ctx, 0.0, None, None, None), "lbm_dscalar_set")
            return
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(c0, dtype=np.float64), (self.ny, self.nx)))
        w = None if wall is None else np.ascontiguousarray(np.broadcast_to(np.asarray(wall, dtype=np.float64), (self.ny, self.nx)))
        i = None if inlet is None else np.ascontiguousarray(np.broadcast_to(np.asarray(inlet, dtype=np.float64), (self.ny,)))
        _check(self.lib.lbm_dscalar_set(self.ctx, float(D), c.ctypes.data, None if w is None else w.ctypes.data,
                                        None if i is None else i.ctypes.data), "lbm_dscalar_set")

    def scalar(self):
        """(D, omega_s) while a scalar is on, None while it is off (lbm_dscalar_get)"""
        on, D, om = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        _check(self.lib.lbm_dscalar_get(self.ctx, ctypes.byref(on), ctypes.byref(D), ctypes.byref(om)), "lbm_dscalar_get")
        return (D.value, om.value) if on.value else None

    def scalar_field(self):
        """float64[ny, nx]: the scalar of every fluid cell, 0.0 on blocked cells (lbm_dscalar_field)"""
        c = np.zeros((self.ny, self.nx), dtype=np.float64)
        _check(self.lib.lbm_dscalar_field(self.ctx, c.ctypes.data), "lbm_dscalar_field")
        return c

    def scalar_cells(self):
        """float64[5, ny, nx]: the scalar's five populations (lbm_dscalar_download)"""
        g = np.zeros((5, self.ny, self.nx), dtype=np.float64)
        _check(self.lib.lbm_dscalar_download(self.ctx, g.ctypes.data), "lbm_dscalar_download")
        return g

    def upload_scalar(self, g):
        """the scalar's five populations, float64[5, ny, nx] (lbm_dscalar_upload); the scalar is on"""
        a = np.ascontiguousarray(g, dtype=np.float64)
        assert a.shape == (5, self.ny, self.nx)
        _check(self.lib.lbm_dscalar_upload(self.ctx, a.ctypes.data), "lbm_dscalar_upload")

    def set_buoyancy(self, b, c_ref=0.0):
        """Buoyancy (lbm_dbuoy_set): b = (b_x, b_y); every fluid cell takes the force density F0 + b (C - c_ref), C its scalar
        value and F0 the body force of set_drive.  (0, 0) or None = off, the default.  Needs a scalar on; only before the first
        step."""
        b_x, b_y = (0.0, 0.0) if b is None else b
        _check(self.lib.lbm_dbuoy_set(self.ctx, float(b_x), float(b_y), float(c_ref)), "lbm_dbuoy_set")

    def buoyancy(self):
        """((b_x, b_y), c_ref) while buoyancy is on, None while it is off (lbm_dbuoy_get)"""
        on, c_ref = ctypes.c_int(), ctypes.c_double()
        b = np.zeros(2, dtype=np.float64)
        _check(self.lib.lbm_dbuoy_get(self.ctx, ctypes.byref(on), b.ctypes.data, ctypes.byref(c_ref)), "lbm_dbuoy_get")
        return ((float(b[0]), float(b[1])), c_ref.value) if on.value else None

    def set_scalar_record(self, on):
        """The scalar's record (lbm_drecord_set): per step the sums of c, c u_x and c u_y over the fluid cells.  Off by
        default.  Needs a scalar on; only before the first step."""
        _check(self.lib.lbm_drecord_set(self.ctx, 1 if on else 0), "lbm_drecord_set")

    def scalar_record_on(self):
        """True while the scalar's record is on (lbm_drecord_get)"""
        on = ctypes.c_int()
        _check(self.lib.lbm_drecord_get(self.ctx, ctypes.byref(on)), "lbm_drecord_get")
        return bool(on.value)

    def scalar_record(self):
        """(content, flux_x, flux_y), float64[steps_done] each: the scalar's record of every step since the upload
        (lbm_drecord); needs set_scalar_record(True) before the first step."""
        steps = self.steps_done
        c, fx, fy = (np.zeros(max(steps, 1), dtype=np.float64) for _ in range(3))
        _check(self.lib.lbm_drecord(self.ctx, c.ctypes.data, fx.ctypes.data, fy.ctypes.data), "lbm_drecord")
        return c[:steps], fx[:steps], fy[:steps]

    def force_record(self):
        """(F_x float64[steps_done], F_y float64[steps_done]): the force of every step since the upload; needs
        set_option("force", 1) before the first step."""
        steps = self.steps_done
        fx, fy = np.zeros(max(steps, 1), dtype=np.float64), np.zeros(max(steps, 1), dtype=np.float64)
        _check(self.lib.lbm_dforce_record(self.ctx, fx.ctypes.data, fy.ctypes.data), "lbm_dforce_record")
        return fx[:steps], fy[:steps]

    def write_values(self, final_state_path="final_state.dat", av_vels_path="av_vels.dat"):
        """The two output files in the reference's %.12E formats (d2q9-bgk.c:835,848-851), as check/check.py reads them."""
        fields = self.final_state()
        _, av = self.download(cells=False)
        _write_values(final_state_path, av_vels_path, self.obstacles, fields, av)


def _sweep(ptype, base, omega, accel):
    """copies of `base` as `ptype` (Params / DParams) with omega and / or accel replaced, each given as a Python float"""
    count = len(omega if omega is not None else accel)
    members = []
    for i in range(count):
        p = ptype.from_buffer_copy(base)
        if omega is not None:
            p.omega = float(omega[i])
        if accel is not None:
            p.accel = float(accel[i])
        members.append(p)
    return members


def sweep_params(base, omega=None, accel=None):
    """The members of a parameter sweep: copies of `base` with omega and / or accel replaced from lists of equal length."""
    return _sweep(Params, base, omega, accel)


def sweep_dparams(base, omega=None, accel=None):
    """The members of a double-precision parameter sweep: copies of the DParams `base` with omega and / or accel replaced
    from lists of equal length, as Python floats (the fp64 literals, never widened floats)."""
    return _sweep(DParams, base, omega, accel)


class _EnsembleOf(_Handle):
    """The body of Ensemble and EnsembleDouble.  A class names its family in `_prefix`, the numpy type of its arrays in
    `_dtype`, the ctypes type of its members' parameters in `_ptype` and the prefix of its steady-run entry points in
    `_steady`."""
    _handle = "ens"
    _dtype = None
    _ptype = None
    _steady = None

    def __init__(self, params, obstacles):
        self.lib = load_library()
        self.params = list(params)
        self.n = len(self.params)
        if self.n < 1:
            raise LBMError("an ensemble needs at least one member")
        self.nx, self.ny = self.params[0].nx, self.params[0].ny
        obst = np.asarray(obstacles, dtype=np.int32)
        if obst.ndim == 2:
            obst = np.broadcast_to(obst, (self.n,) + obst.shape)
        obst = np.ascontiguousarray(obst)
        assert obst.shape == (self.n, self.ny, self.nx)
        self.obstacles = obst
        self._params = (self._ptype * self.n)(*self.params)
        self.ens = ctypes.c_void_p()
        create = self._prefix + "_create"
        _check(getattr(self.lib, create)(ctypes.byref(self.ens), self._params, obst.ctypes.data, self.n), create)

    def upload(self, cells=None):
        """cells float32[n, 9, ny, nx] (an EnsembleDouble: float64); None = every member's rest state from its own density, on
        the device"""
        if cells is None:
            self._call("upload", None)
        else:
            c = np.ascontiguousarray(cells, dtype=self._dtype)
            assert c.shape == (self.n, 9, self.ny, self.nx)
            self._call("upload", c.ctypes.data)

    def download(self, cells=True, av_vels=True):
        """Returns (cells float32[n,9,ny,nx] or None, av_vels float32[n,steps_done] or None); an EnsembleDouble: float64."""
        steps = self.steps_done
        c = np.zeros((self.n, 9, self.ny, self.nx), dtype=self._dtype) if cells else None
        a = np.zeros((self.n, steps), dtype=self._dtype) if av_vels else None
        self._call("download", c.ctypes.data if cells else None, a.ctypes.data if av_vels and steps else None)
        return c, a

    def final_state(self):
        """(u_x, u_y, u, pressure), each float32[n,ny,nx] (an EnsembleDouble: float64) — per member the columns of
        final_state.dat."""
        outs = [np.zeros((self.n, self.ny, self.nx), dtype=self._dtype) for _ in range(4)]
        self._call("final_state", *[o.ctypes.data for o in outs])
        return outs

    def reynolds(self):
        """float32[n] (an EnsembleDouble: float64[n]): every member's Reynolds number of the current state"""
        r = np.zeros(self.n, dtype=self._dtype)
        self._call("reynolds", r.ctypes.data)
        return r

    def run_until(self, max_steps, window=64, rel_tol=1e-4):
        """Every member to its own steady state (lbm_steady_run; an EnsembleDouble: lbm_dsteady_run): legs of `window` steps,
        a member stops at the first check point s where |A(s) - A(s - window)| <= rel_tol |A(s)| on its own av_vels record, at
        most max_steps steps.  Returns (steps int32[n], converged bool[n]).  Members that stopped at different counts leave
        the ensemble ragged: download(), final_state() and reynolds() return every member's own last state, run() is refused
        until the next upload()."""
        symbol = self._steady + "_run"
        _check(getattr(self.lib, symbol)(self.ens, max_steps, window, rel_tol), symbol)
        return self.member_steps()

    def member_steps(self):
        """(steps int32[n], converged bool[n]): per member the steps applied since the last upload, and whether it met the
        criterion of the last run_until since then"""
        steps = np.zeros(self.n, dtype=np.int32)
        conv = np.zeros(self.n, dtype=np.int32)
        symbol = self._steady + "_steps"
        _check(getattr(self.lib, symbol)(self.ens, steps.ctypes.data, conv.ctypes.data), symbol)
        return steps, conv.astype(bool)


class Ensemble(_EnsembleOf):
    """N independent simulations of one grid size, advanced together (lbm_ens): one launch per (up to) eight timesteps for
    all members.  Mirrors LBM with the member index as the first axis of every array.  `params`: a list of Params that share
    nx, ny and max_iters; `obstacles`: int32[n, ny, nx], or one [ny, nx] map for all members."""
    _prefix, _dtype, _ptype, _steady = "lbm_ens", np.float32, Params, "lbm_steady"


class EnsembleDouble(_EnsembleOf, _Stats):
    """N independent double-precision simulations of one grid size, advanced together (lbm_dens): one launch per several
    timesteps for all members, every member bit-identical to an LBMDouble on the same inputs.  Mirrors Ensemble with double
    in place of float.  `params`: a list of DParams that share nx, ny and max_iters (sweep_dparams); `obstacles`:
    int32[n, ny, nx], or one [ny, nx] map for all members.  run_until() stops a member where an LBMDouble run to the same
    count would be, bit for bit, av_vels included."""
    _prefix, _dtype, _ptype, _steady = "lbm_dens", np.float64, DParams, "lbm_dsteady"
    _stats = "lbm_dstats_ens"

    def _stats_lead(self):
        return (self.n,)

    def __init__(self, params, obstacles):
        params = list(params)
        if not all(isinstance(p, DParams) for p in params):
            raise LBMError("EnsembleDouble takes DParams (make_dparams / read_inputs_double / sweep_dparams)")
        super().__init__(params, obstacles)

    def set_option(self, key, value):
        """one key, "force": 1 = record every member's force per step (before the first step)"""
        _check(self.lib.lbm_dforce_ens_set_option(self.ens, key.encode(), int(value)), "lbm_dforce_ens_set_option(%s)" % key)

    def get_option(self, key):
        v = ctypes.c_long()
        _check(self.lib.lbm_dforce_ens_get_option(self.ens, key.encode(), ctypes.byref(v)), "lbm_dforce_ens_get_option(%s)" % key)
        return v.value

    def set_body(self, body):
        """Per member the blocked cells whose links count in the force (lbm_dbody_ens_set): int32[n, ny, nx], or one [ny, nx]
        map for all members; non-zero = counts; None = every blocked cell again.  With "force" on only before the first
        step."""
        if body is None:
            _check(self.lib.lbm_dbody_ens_set(self.ens, None), "lbm_dbody_ens_set")
            return
        b = np.asarray(body, dtype=np.int32)
        if b.ndim == 2:
            b = np.broadcast_to(b, (self.n,) + b.shape)
        b = np.ascontiguousarray(b)
        assert b.shape == (self.n, self.ny, self.nx)
        _check(self.lib.lbm_dbody_ens_set(self.ens, b.ctypes.data), "lbm_dbody_ens_set")

    def body(self):
        """int32[n, ny, nx]: 1 where a blocked cell counts in the force, else 0 (lbm_dbody_ens_get)"""
        b = np.zeros((self.n, self.ny, self.nx), dtype=np.int32)
        _check(self.lib.lbm_dbody_ens_get(self.ens, b.ctypes.data), "lbm_dbody_ens_get")
        return b

    def set_trt(self, magic):
        """The collision operator of all members (lbm_dtrt_ens_set): one magic parameter for all, or an array-like of n, every
        entry > 0 = two relaxation times; None = BGK, the default.  Only before the first step."""
        if magic is None:
            _check(self.lib.lbm_dtrt_ens_set(self.ens, None), "lbm_dtrt_ens_set")
            return
        m = np.asarray(magic, dtype=np.float64)
        if m.ndim == 0:
            m = np.full(self.n, float(m), dtype=np.float64)
        m = np.ascontiguousarray(m)
        assert m.shape == (self.n,)
        _check(self.lib.lbm_dtrt_ens_set(self.ens, m.ctypes.data), "lbm_dtrt_ens_set")

    def trt(self):
        """(magic float64[n], omega_minus float64[n]): per member the magic parameter in force (0.0: BGK) and the second
        relaxation rate, the member's omega under BGK (lbm_dtrt_ens_get)"""
        magic, om = np.zeros(self.n, dtype=np.float64), np.zeros(self.n, dtype=np.float64)
        _check(self.lib.lbm_dtrt_ens_get(self.ens, magic.ctypes.data, om.ctypes.data), "lbm_dtrt_ens_get")
        return magic, om

    def set_open(self, u_in, rho_out=None):
        """Open boundaries of all members (lbm_dopen_ens_set): u_in float64[n, ny] (or one [ny] profile for all), rho_out
        float64[n] (or one value for all); set_open(None) = periodic and accelerated, the default.  Only before the first
        step."""
        if u_in is None:
            _check(self.lib.lbm_dopen_ens_set(self.ens, None, None), "lbm_dopen_ens_set")
            return
        u = np.asarray(u_in, dtype=np.float64)
        if u.ndim == 1:
            u = np.broadcast_to(u, (self.n,) + u.shape)
        u = np.ascontiguousarray(u)
        r = np.asarray(rho_out, dtype=np.float64)
        if r.ndim == 0:
            r = np.full(self.n, float(r), dtype=np.float64)
        r = np.ascontiguousarray(r)
        assert u.shape == (self.n, self.ny) and r.shape == (self.n,)
        _check(self.lib.lbm_dopen_ens_set(self.ens, u.ctypes.data, r.ctypes.data), "lbm_dopen_ens_set")

    def open(self):
        """(u_in float64[n, ny], rho_out float64[n]) while open boundaries are on, None while they are off
        (lbm_dopen_ens_get)"""
        on = ctypes.c_int()
        u, r = np.zeros((self.n, self.ny), dtype=np.float64), np.zeros(self.n, dtype=np.float64)
        _check(self.lib.lbm_dopen_ens_get(self.ens, ctypes.byref(on), u.ctypes.data, r.ctypes.data), "lbm_dopen_ens_get")
        return (u, r) if on.value else None

    def set_wall(self, u_x, u_y, rho_wall=None):
        """Moving walls of all members (lbm_dwall_ens_set): u_x, u_y float64[n, ny, nx] (or one [ny, nx] map for all), the wall
        velocity of every blocked cell (zero on fluid cells); rho_wall float64[n], one value for all, or None: each member's
        density from its params.  set_wall(None, None) = every wall at rest, the default.  Only before the first step."""
        if u_x is None and u_y is None:
            _check(self.lib.lbm_dwall_ens_set(self.ens, None, None, None), "lbm_dwall_ens_set")
            return
        maps = []
        for u in (u_x, u_y):
            if u is not None:
                u = np.asarray(u, dtype=np.float64)
                if u.ndim == 2:
                    u = np.broadcast_to(u, (self.n,) + u.shape)
                u = np.ascontiguousarray(u)
                assert u.shape == (self.n, self.ny, self.nx)
            maps.append(u)
        r = np.array([p.density for p in self.params] if rho_wall is None else rho_wall, dtype=np.float64)
        if r.ndim == 0:
            r = np.full(self.n, float(r), dtype=np.float64)
        r = np.ascontiguousarray(r)
        assert r.shape == (self.n,)
        _check(self.lib.lbm_dwall_ens_set(self.ens, *[None if u is None else u.ctypes.data for u in maps], r.ctypes.data),
               "lbm_dwall_ens_set")

    def wall(self):
        """(u_x float64[n, ny, nx], u_y float64[n, ny, nx], rho_wall float64[n]) while wall velocities are on, None while they
        are off (lbm_dwall_ens_get)"""
        on = ctypes.c_int()
        ux, uy = (np.zeros((self.n, self.ny, self.nx), dtype=np.float64) for _ in range(2))
        r = np.zeros(self.n, dtype=np.float64)
        _check(self.lib.lbm_dwall_ens_get(self.ens, ctypes.byref(on), ux.ctypes.data, uy.ctypes.data, r.ctypes.data),
               "lbm_dwall_ens_get")
        return (ux, uy, r) if on.value else None

    def set_les(self, c):
        """Subgrid viscosity of all members (lbm_dles_ens_set): one Smagorinsky constant for all, or an array-like of n, every
        entry > 0; None or 0.0 = off, the default.  Only before the first step."""
        if c is None or (np.ndim(c) == 0 and float(c) == 0.0):
            _check(self.lib.lbm_dles_ens_set(self.ens, None), "lbm_dles_ens_set")
            return
        v = np.asarray(c, dtype=np.float64)
        if v.ndim == 0:
            v = np.full(self.n, float(v), dtype=np.float64)
        v = np.ascontiguousarray(v)
        assert v.shape == (self.n,)
        _check(self.lib.lbm_dles_ens_set(self.ens, v.ctypes.data), "lbm_dles_ens_set")

    def les(self):
        """(c float64[n], les_k float64[n]): per member the Smagorinsky constant in force (0.0: off) and (18 sqrt 2) c^2 as the
        library computes it (lbm_dles_ens_get)"""
        c, k = np.zeros(self.n, dtype=np.float64), np.zeros(self.n, dtype=np.float64)
        _check(self.lib.lbm_dles_ens_get(self.ens, c.ctypes.data, k.ctypes.data), "lbm_dles_ens_get")
        return c, k

    def set_drive(self, f):
        """Body force of all members (lbm_ddrive_ens_set): one pair (F_x, F_y) for all, or an array-like [n, 2], no member (0, 0);
        None = off, the default.  Only before the first step."""
        if f is None:
            _check(self.lib.lbm_ddrive_ens_set(self.ens, None), "lbm_ddrive_ens_set")
            return
        v = np.asarray(f, dtype=np.float64)
        if v.ndim == 1:
            v = np.broadcast_to(v, (self.n, 2))
        v = np.ascontiguousarray(v)
        assert v.shape == (self.n, 2)
        _check(self.lib.lbm_ddrive_ens_set(self.ens, v.ctypes.data), "lbm_ddrive_ens_set")

    def drive(self):
        """float64[n, 2]: per member the body force in force, zeros while it is off (lbm_ddrive_ens_get)"""
        on = ctypes.c_int()
        f = np.zeros((self.n, 2), dtype=np.float64)
        _check(self.lib.lbm_ddrive_ens_get(self.ens, ctypes.byref(on), f.ctypes.data), "lbm_ddrive_ens_get")
        return f

    def _per_member(self, a, shape):
        """`a` as a contiguous float64 array with a leading member axis: given with it, or broadcast over the members"""
        return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (self.n,) + shape))

    def set_scalar(self, D, c0=0.0, wall=None, inlet=None):
        """Passive scalars of all members (lbm_dscalar_ens_set): D one diffusivity for all or an array-like of n, every entry > 0;
        c0 float64[n, ny, nx], wall float64[n, ny, nx] (NaN = insulating; None: all insulating) and inlet float64[n, ny] (None:
        zeros) with the member axis or broadcast over it.  set_scalar(None) = off, the default.  Between runs at any step count."""
        if D is None:
            _check(self.lib.lbm_dscalar_ens_set(self.ens, None, None, None, None), "lbm_dscalar_ens_set")
            return
        d = self._per_member(D, ())
        c = self._per_member(c0, (self.ny, self.nx))
        w = None if wall is None else self._per_member(wall, (self.ny, self.nx))
        i = None if inlet is None else self._per_member(inlet, (self.ny,))
        _check(self.lib.lbm_dscalar_ens_set(self.ens, d.ctypes.data, c.ctypes.data, None if w is None else w.ctypes.data,
                                            None if i is None else i.ctypes.data), "lbm_dscalar_ens_set")

    def scalar(self):
        """(D float64[n], omega_s float64[n]) while the scalars are on, None while they are off (lbm_dscalar_ens_get)"""
        on = ctypes.c_int()
        D, om = np.zeros(self.n, dtype=np.float64), np.zeros(self.n, dtype=np.float64)
        _check(self.lib.lbm_dscalar_ens_get(self.ens, ctypes.byref(on), D.ctypes.data, om.ctypes.data), "lbm_dscalar_ens_get")
        return (D, om) if on.value else None

    def scalar_field(self):
        """float64[n, ny, nx]: every member's scalar on its fluid cells, 0.0 on blocked cells (lbm_dscalar_ens_field)"""
        c = np.zeros((self.n, self.ny, self.nx), dtype=np.float64)
        _check(self.lib.lbm_dscalar_ens_field(self.ens, c.ctypes.data), "lbm_dscalar_ens_field")
        return c

    def scalar_cells(self):
        """float64[n, 5, ny, nx]: every member's five populations (lbm_dscalar_ens_download)"""
        g = np.zeros((self.n, 5, self.ny, self.nx), dtype=np.float64)
        _check(self.lib.lbm_dscalar_ens_download(self.ens, g.ctypes.data), "lbm_dscalar_ens_download")
        return g

    def upload_scalar(self, g):
        """every member's five populations, float64[n, 5, ny, nx] (lbm_dscalar_ens_upload); the scalars are on"""
        a = np.ascontiguousarray(g, dtype=np.float64)
        assert a.shape == (self.n, 5, self.ny, self.nx)
        _check(self.lib.lbm_dscalar_ens_upload(self.ens, a.ctypes.data), "lbm_dscalar_ens_upload")

    def set_buoyancy(self, b, c_ref=0.0):
        """Buoyancy of all members (lbm_dbuoy_ens_set): b one pair (b_x, b_y) for all or an array-like [n, 2], no member (0, 0);
        c_ref one value for all or an array-like of n.  None = off, the default.  Needs the scalars on; only before the first
        step."""
        if b is None:
            _check(self.lib.lbm_dbuoy_ens_set(self.ens, None), "lbm_dbuoy_ens_set")
            return
        v = np.empty((self.n, 3), dtype=np.float64)
        v[:, :2] = np.asarray(b, dtype=np.float64)
        v[:, 2] = np.asarray(c_ref, dtype=np.float64)
        _check(self.lib.lbm_dbuoy_ens_set(self.ens, v.ctypes.data), "lbm_dbuoy_ens_set")

    def buoyancy(self):
        """float64[n, 3], per member b_x, b_y, c_ref, while buoyancy is on, None while it is off (lbm_dbuoy_ens_get)"""
        on = ctypes.c_int()
        b = np.zeros((self.n, 3), dtype=np.float64)
        _check(self.lib.lbm_dbuoy_ens_get(self.ens, ctypes.byref(on), b.ctypes.data), "lbm_dbuoy_ens_get")
        return b if on.value else None

    def set_scalar_record(self, on):
        """The scalars' record of all members (lbm_drecord_ens_set): per step and member the sums of c, c u_x and c u_y
        over the fluid cells.  Off by default.  Needs the scalars on; only before the first step."""
        _check(self.lib.lbm_drecord_ens_set(self.ens, 1 if on else 0), "lbm_drecord_ens_set")

    def scalar_record_on(self):
        """True while the scalars' record is on (lbm_drecord_ens_get)"""
        on = ctypes.c_int()
        _check(self.lib.lbm_drecord_ens_get(self.ens, ctypes.byref(on)), "lbm_drecord_ens_get")
        return bool(on.value)

    def scalar_record(self):
        """(content, flux_x, flux_y), float64[n, steps_done] each: every member's record of every step since the upload, +0.0 at
        and beyond the count of a member that run_until() stopped earlier (lbm_drecord_ens); needs
        set_scalar_record(True) before the first step."""
        steps = self.steps_done
        c, fx, fy = (np.zeros((self.n, max(steps, 1)), dtype=np.float64) for _ in range(3))
        _check(self.lib.lbm_drecord_ens(self.ens, c.ctypes.data, fx.ctypes.data, fy.ctypes.data), "lbm_drecord_ens")
        return c[:, :steps].copy(), fx[:, :steps].copy(), fy[:, :steps].copy()

    SCALAR_CRITERIA = {"scalar": 0, "scalar_flux_x": 1, "scalar_flux_y": 2}

    def run_until(self, max_steps, window=64, rel_tol=1e-4, on="av_vels"):
        """_EnsembleOf.run_until with a choice of criterion: on="av_vels" (lbm_dsteady_run), or on="drag"
        (lbm_dbody_steady_run): |F(s) - F(s - window)| <= rel_tol |F(s)| on the member's own F_x record, the force on its body
        (set_body); needs set_option("force", 1) before the first step.  on="scalar", "scalar_flux_x" or "scalar_flux_y"
        (lbm_drecord_steady_run): the same rule on the member's own content, flux_x or flux_y record of its scalar; needs
        set_scalar_record(True) before the first step."""
        if on == "av_vels":
            return super().run_until(max_steps, window=window, rel_tol=rel_tol)
        if on in self.SCALAR_CRITERIA:
            _check(self.lib.lbm_drecord_steady_run(self.ens, max_steps, window, rel_tol, self.SCALAR_CRITERIA[on]),
                   "lbm_drecord_steady_run")
            return self.member_steps()
        if on != "drag":
            raise ValueError("run_until(on=%r): the criteria are \"av_vels\", \"drag\", \"scalar\", \"scalar_flux_x\" and "
                             "\"scalar_flux_y\"" % (on,))
        _check(self.lib.lbm_dbody_steady_run(self.ens, max_steps, window, rel_tol), "lbm_dbody_steady_run")
        return self.member_steps()

    def force(self):
        """(F_x float64[n], F_y float64[n]): every member's momentum-exchange force of its current state as the next step
        would stream it (lbm_dforce_ens).  The states are not modified."""
        fx, fy = np.zeros(self.n, dtype=np.float64), np.zeros(self.n, dtype=np.float64)
        _check(self.lib.lbm_dforce_ens(self.ens, fx.ctypes.data, fy.ctypes.data), "lbm_dforce_ens")
        return fx, fy

    def force_record(self):
        """(F_x float64[n, steps_done], F_y float64[n, steps_done]): every member's force of every step since the upload,
        +0.0 at and beyond the count of a member that run_until() stopped earlier; needs set_option("force", 1) before the
        first step."""
        steps = self.steps_done
        fx, fy = (np.zeros((self.n, max(steps, 1)), dtype=np.float64) for _ in range(2))
        _check(self.lib.lbm_dforce_ens_record(self.ens, fx.ctypes.data, fy.ctypes.data), "lbm_dforce_ens_record")
        return fx[:, :steps].copy(), fy[:, :steps].copy()

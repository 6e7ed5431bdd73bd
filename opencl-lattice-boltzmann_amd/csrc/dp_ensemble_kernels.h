// Device side of a DOUBLE-PRECISION ENSEMBLE (include/lbm.h: lbm_dens_*): N independent fp64 grids of one size, each with
// its own run constants, obstacle map and state, advanced by one launch per (up to) TMAX timesteps.
//
// d2q9_dp_ensemble is d2q9_dp_multi (dp_kernels.h) with a member axis, the way d2q9_ensemble (ensemble_kernels.h) is
// d2q9_multi's, and here the two are one body (dp_tile, dp_tile.h) on two Grids: nothing is mirrored by hand.
// member = blockIdx.y, tile = blockIdx.x; a member's two grids, mask and segment sums lie a member stride
// apart, in the layout of dp_kernels.h (row-interleaved SoA in double, planes padded to 32 doubles).  x and y wrap inside
// the member: members never interact.  The per-cell arithmetic is dp_collide_cell / dp_accelerate_cell of dp_kernels.h, so a
// member's cells are bit-identical to an lbm_dp context on the same inputs; the velocity sum keeps that header's scheme
// (every 16-cell row segment in one fixed tree, a step's segments added per member by dens_reduce in dp_reduce's order), so
// a member's av_vels are bit-identical too.
#pragma once
#include "dp_kernels.h"

namespace lbm {

// What differs from member to member, in device memory, read by member index (a wave-uniform load), as EnsMember
struct DensMember {
  double omega, aw1, aw2;  // aw1 = density*accel/9, aw2 = density*accel/36 (kernels.cl:14-15), in double
  double density;
  double w0, w1, w2;       // rest state (d2q9-bgk.c:529-531)
  union {
    double omega_m;        // the second relaxation rate of the TRT instances (dp_trt_omega_minus); omega where the member is BGK
    double pad;            // the name under which member_constants (host_common.h) zeroes the table's last slot
  };
};
static_assert(sizeof(DensMember) == 64, "a member's constants are one 64-B line");

struct DensArgs {
  const double *src;         // member m: src + m * member_stride
  double *dst;
  const uint8_t *mask;       // member m: mask + m * nx * ny
  const DensMember *members; // [members], and behind them the open-boundary table (OPEN: dens_open_table)
  double *seg;               // [T][members][ny][nseg]: the segment sums of each of the T steps; FORCE:
                             // [T][3][members][ny][nseg], |u|, F_x, F_y
  unsigned long long plane_stride, member_stride;   // row_stride = 9 * plane_stride
  unsigned long long seg_step;                      // = members * ny * nseg; FORCE: three times that
  int nx, ny, nseg;
  int tiles_x;
  int T;                     // steps in this launch
  int accel_next;            // apply the following step's accelerate_flow to the final state
};
// What a WALL instance takes beyond that: the members' wall velocities, [2][members][ny][nx], u_x then u_y (lbm_dwall_ens_set;
// one address: the kernel is short of SGPRs).  The WALL = false instances keep the argument struct of a library without moving
// walls.
struct DensWallArgs : DensArgs {
  const double *wall_u;
};
template <bool WALL>
using DensArgsOf = std::conditional_t<WALL, DensWallArgs, DensArgs>;

// Open boundaries: member m's inlet profile u_in[ny] and, behind it, its rho_out lie m * (ny + 1) doubles into a second table,
// which starts where the table of DensMember ends: one allocation, and DensArgs is the struct of a library without it.
__host__ __device__ inline const double *dens_open_table(const DensMember *members, int n) {
  return reinterpret_cast<const double *>(members + n);
}
// Moving walls: member m's rho_wall is entry m of a third table, behind the open-boundary table
__host__ __device__ inline const double *dens_wall_table(const DensMember *members, int n, int ny) {
  return dens_open_table(members, n) + (size_t)n * (ny + 1);
}

// Member blockIdx.y as dp_tile takes it (dp_tile.h): its arrays a member stride into the ensemble's, its constants from the
// DensMember load, its profile, rho_out and rho_wall from the tables behind the members
template <bool WALL>
struct DensGrid {
  static constexpr bool kStageRhoOut = true;   // rho_out lies in a table in global memory: no load under the outlet's branch
  const DensArgsOf<WALL> &a;
  int member;
  size_t cells, cell0;   // nx * ny, and this member's cell (0,0) among all members' cells: mask and wall velocities
  const double *src;
  double *dst;
  const uint8_t *mask;
  double *seg_out;
  double omega, omega_m, aw1, aw2;
  __device__ __forceinline__ explicit DensGrid(const DensArgsOf<WALL> &a_) : a(a_), member(blockIdx.y) {
    src = a.src + (size_t)member * a.member_stride;
    dst = a.dst + (size_t)member * a.member_stride;
    cells = (size_t)a.nx * a.ny;
    cell0 = (size_t)member * cells;
    mask = a.mask + cell0;
    seg_out = a.seg + (size_t)member * ((size_t)a.ny * a.nseg);
    const DensMember mc = a.members[member];
    omega = mc.omega, omega_m = mc.omega_m, aw1 = mc.aw1, aw2 = mc.aw2;
  }
  __device__ __forceinline__ unsigned comp() const { return gridDim.y * (unsigned)(a.ny * a.nseg); }   // members * ny * nseg < 2^31 (lbm_dens_create's bounds)
  __device__ __forceinline__ const double *u_in() const { return dens_open_table(a.members, (int)gridDim.y) + (size_t)member * (a.ny + 1); }
  __device__ __forceinline__ double rho_out() const { return u_in()[a.ny]; }
  // wall_u is [2][members][ny][nx], u_x then u_y
  __device__ __forceinline__ size_t wall_cell0() const { return cell0; }
  __device__ __forceinline__ const double *wall_u_x() const { return a.wall_u; }
  __device__ __forceinline__ const double *wall_u_y() const { return a.wall_u + (size_t)gridDim.y * cells; }
  __device__ __forceinline__ double rho_wall() const { return dens_wall_table(a.members, (int)gridDim.y, a.ny)[member]; }
};

// grid = (tiles per member, members), NT threads: dp_tile (dp_tile.h) on member blockIdx.y, tile blockIdx.x.
//
// Tile shape and depth, measured (tools/dp_ensemble_ab.py, one MI355X, one call; us/step for all members together at
// 64 x 128x128 / 16 x 256x256, medians of 5 repeats of 2000 steps; as 64 / 16 lbm_dp contexts in the same runs: 37.9 / 30.2;
// profiles/dp_ensemble_throughput.txt):
//   16x16, T <= 8, 1024 threads (149 KB of LDS, one workgroup per CU)   28.82 / 28.61
//   16x8,  T <= 8, 1024 threads (111 KB, one per CU)                    46.29 / 46.08
//   16x16, T <= 3, 1024 threads ( 73 KB, two per CU, 62 VGPRs)          20.25 / 19.92   <- instantiated
//   16x16, T <= 3,  512 threads ( 73 KB, two per CU)                    20.61 / 20.22
//   16x8,  T <= 5,  512 threads ( 68 KB, two per CU)                    27.43 / 27.28
//   16x8,  T <= 4,  512 threads ( 56 KB, two per CU)                    28.11 / 27.86
//   16x8,  T <= 3,  512 threads ( 46 KB, three per CU)                  23.53 / 23.20
// Two workgroups per CU win at either height (one's loads and stores run under the other's sub-steps, and a shallow region
// recomputes 1.28 x the tile per step against 2.15 x at T = 8); 16x16 at T <= 2 / 1: 25.85 / 51.75 on the first case.  One form
// serves both sizes.  Ensembles whose tiles all get a CU of their own (<= 256 tiles) run 19-30 % faster at T <= 8 (1 x 128x128
// 1.95 against 2.40); that form is not instantiated.  0 scratch, 0 spills in all.
// LDS: 74 280 B plain and with FORCE or TRT, 74 464 B with WALL, 74 472 B with OPEN, 74 656 B with both; at most 81 920 B for
// two workgroups per CU.  An ensemble has each option on or off for all members, so no instance branches per member; a member
// without a moving cell takes the WALL branch nowhere.
//
// The FORCE instance states its two workgroups per CU (NT / 128 waves per SIMD) to the compiler: 60 VGPRs, 78 SGPRs, 0 scratch.
// So do the TRT, OPEN and WALL instances (DESIGN.md section 3.7 holds their tables).  The gated kernel of a steady run
// (dp_steady_kernels.h) calls dp_tile the same way and so advances a member with the very same instructions.
template <int TX, int TY, int TMAX, int NT, bool FORCE, bool TRT, bool OPEN, bool WALL = false>
__global__ __launch_bounds__(NT, (FORCE || TRT || OPEN || WALL) ? NT / 128 : 1) void d2q9_dp_ensemble(const DensArgsOf<WALL> a) {
  dp_tile<TX, TY, TMAX, NT, FORCE, TRT, OPEN, WALL, DensGrid<WALL>>(a);
}

// ---- second reduction stage with a member axis: dp_reduce's partition and order, fixed, no atomics -------------------
// grid = (blocks, steps, members): block b of step r of member m adds in[r * in_stride + m * in_member + i] for i in its
// contiguous chunk (lane-strided, then the wave butterfly, then the four waves in order) into
// out[m * out_member + r * out_stride + b].  With the block count lbm_dp takes for a grid of the member's ny * nseg this
// adds a step's segments in the order dp_reduce adds them there: once into av_sum, or twice (partials per block, then one
// block per step and member).  active: NULL, or one word per member; a member whose word is 0 has stopped
// (dp_steady_kernels.h), its tiles wrote no segment sums and its record is left alone.
static __global__ __launch_bounds__(kBlock) void dens_reduce(const double *in, unsigned long long in_stride,
                                                             unsigned long long in_member, long n, double *out,
                                                             unsigned long long out_stride, unsigned long long out_member,
                                                             const int *active) {
  if (active && active[blockIdx.z] == 0) return;  // uniform over the workgroup, before the barrier
  const long chunk = (n + gridDim.x - 1) / gridDim.x;
  const long i0 = (long)blockIdx.x * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
  const double *p = in + (size_t)blockIdx.y * in_stride + (size_t)blockIdx.z * in_member;
  double acc = 0.0;
  for (long i = i0 + threadIdx.x; i < i1; i += kBlock) acc += p[i];
  const double t = dp_block_sum(acc);
  if (threadIdx.x == 0) out[(size_t)blockIdx.z * out_member + (size_t)blockIdx.y * out_stride + blockIdx.x] = t;
}

// ---- the helper kernels of dp_kernels.h with a member axis (blockIdx.y), same per-cell arithmetic --------------------

// accelerate_flow of row ny-2 of every member (kernels.cl:9-53): prologue of a run.  active: as dens_reduce
static __global__ void dens_accelerate_row(double *cells, unsigned long long plane_stride, unsigned long long member_stride,
                                           const uint8_t *mask, const DensMember *members, int nx, int ny, const int *active) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= nx || (active && active[blockIdx.y] == 0)) return;
  const DensMember mc = members[blockIdx.y];
  const int row = ny - 2;
  double f[9];
  double *c = cells + (size_t)blockIdx.y * member_stride + (size_t)row * 9 * plane_stride + x;
#pragma unroll
  for (int k = 0; k < 9; k++) f[k] = c[k * plane_stride];
  dp_accelerate_cell(f, mask[(size_t)blockIdx.y * ((size_t)nx * ny) + (size_t)row * nx + x] != 0, mc.aw1, mc.aw2);
#pragma unroll
  for (int k = 0; k < 9; k++) c[k * plane_stride] = f[k];
}

// every member's rest state from its own density (values of d2q9-bgk.c:529-550, computed on the host in double)
static __global__ void dens_init_cells(double *cells, unsigned long long plane_stride, unsigned long long member_stride,
                                       const DensMember *members, int nx, size_t n) {
  const DensMember mc = members[blockIdx.y];
  cells += (size_t)blockIdx.y * member_stride;
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
    const size_t y = c / nx;
    const size_t i = y * 9 * plane_stride + (c - y * nx);
    cells[i] = mc.w0;
#pragma unroll
    for (int k = 1; k <= 4; k++) cells[k * plane_stride + i] = mc.w1;
#pragma unroll
    for (int k = 5; k <= 8; k++) cells[k * plane_stride + i] = mc.w2;
  }
}

// device layout <-> the caller's double[members][9][ny][nx] (staged in the grid array that is not current, one transfer
// for the whole ensemble).  TO_DEVICE: flat -> cells, else cells -> flat.  par: NULL, or one word per member that says which
// of the two grid arrays holds that member's current state (0: cells, 1: cells_alt) once members have stopped on different
// launch parities (dp_steady_kernels.h).
template <bool TO_DEVICE>
static __global__ void dens_pack_planes(double *cells, double *cells_alt, const int *par, unsigned long long plane_stride,
                                        unsigned long long member_stride, int nx, size_t n, double *flat) {
  if (par && par[blockIdx.y]) cells = cells_alt;
  cells += (size_t)blockIdx.y * member_stride;
  flat += (size_t)blockIdx.y * 9 * n;
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
    const size_t y = c / nx;
    const size_t i = y * 9 * plane_stride + (c - y * nx);
#pragma unroll
    for (int k = 0; k < 9; k++) {
      if (TO_DEVICE) cells[k * plane_stride + i] = flat[k * n + c];
      else flat[k * n + c] = cells[k * plane_stride + i];
    }
  }
}

// output stage per member (dp_final_fields: d2q9-bgk.c:787-832, 396-442, in double, the oracle's statements): outputs are
// double[members][ny][nx], partials double[members][gridDim.x] — with dp_final_fields' block count the per-block sums of u
// are those of an lbm_dp context of the member's size, bit for bit.  cells_alt, par: as dens_pack_planes
static __global__ __launch_bounds__(kBlock) void dens_final_fields(const double *cells, const double *cells_alt, const int *par,
                                                                   unsigned long long plane_stride,
                                                                   unsigned long long member_stride, int nx, const uint8_t *mask,
                                                                   size_t n, const DensMember *members, double *u_x, double *u_y,
                                                                   double *u, double *pressure, double *partials) {
#pragma clang fp contract(off)
  const double c_sq = 1.0 / 3.0;
  const double density = members[blockIdx.y].density;
  if (par && par[blockIdx.y]) cells = cells_alt;
  cells += (size_t)blockIdx.y * member_stride;
  mask += (size_t)blockIdx.y * n;
  const size_t off = (size_t)blockIdx.y * n;
  double tot_u = 0.0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    double ux = 0.0, uy = 0.0, uu = 0.0, pr = density * c_sq;
    if (mask[i] == 0) {
      double f[9];
      const size_t y = i / nx;
      const size_t cell = y * 9 * plane_stride + (i - y * nx);
#pragma unroll
      for (int k = 0; k < 9; k++) f[k] = cells[k * plane_stride + cell];
      dp_output_cell(f, ux, uy, uu, pr);
      tot_u += uu;
    }
    if (u_x) u_x[off + i] = ux;
    if (u_y) u_y[off + i] = uy;
    if (u) u[off + i] = uu;
    if (pressure) pressure[off + i] = pr;
  }
  const double t = dp_block_sum(tot_u);
  if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

}  // namespace lbm

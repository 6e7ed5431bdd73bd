// Device side of a DOUBLE-PRECISION ENSEMBLE (include/lbm.h: lbm_dens_*): N independent fp64 grids of one size, each with
// its own run constants, obstacle map and state, advanced by one launch per (up to) TMAX timesteps.
//
// d2q9_dp_ensemble is d2q9_dp_multi (dp_kernels.h) with a member axis, the way d2q9_ensemble (ensemble_kernels.h) is
// d2q9_multi's, and here the two are one body (dp_tile, dp_tile.h) on two Grids: nothing is mirrored by hand.
// member = blockIdx.y, tile = blockIdx.x; a member's two grids, mask and segment sums lie a member stride
// apart, in the layout of dp_kernels.h (row-interleaved SoA in double, planes padded to 32 doubles).  x and y wrap inside
// the member: members never interact.  The per-cell arithmetic is dp_collide_cell / dp_accelerate_cell of dp_kernels.h, so a
// member's cells are bit-identical to an lbm_dp context on the same inputs; the velocity sum keeps that header's scheme
// (every 16-cell row segment in one fixed tree, a step's segments added per member by dp_reduce), so a member's av_vels are
// bit-identical too.  The kernels around the step (reduction, prologue, rest state, pack, output stage) and the table of
// per-member constants (DpMember) are dp_kernels.h's, one set for both families.
#pragma once
#include "dp_kernels.h"

namespace lbm {

struct DensArgs {
  const double *src;         // member m: src + m * member_stride
  double *dst;
  const uint8_t *mask;       // member m: mask + m * nx * ny
  const DpMember *members; // [members], and behind them the open-boundary table (OPEN: dens_open_table, dp_kernels.h), the wall
                           // densities (WALL: dens_wall_table), the subgrid constants (LES: dens_les_table) and the body forces
                           // (DRIVE: dens_drive_table)
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

// Member blockIdx.y as dp_tile takes it (dp_tile.h): its arrays a member stride into the ensemble's, its constants from the
// DpMember load, its profile, rho_out, rho_wall and subgrid constants from the tables behind the members
template <bool WALL>
struct DensGrid {
  static constexpr bool kStageRhoOut = true;   // rho_out lies in a table in global memory: no load under the outlet's branch
  static constexpr bool kStageLes = true;      // the subgrid constants too, and six SGPRs across the loops are six too many here
  static constexpr bool kStageDrive = true;    // and the body force, for the same reason
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
    const DpMember mc = a.members[member];
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
  __device__ __forceinline__ DpLes les() const { return dens_les_table(a.members, (int)gridDim.y, a.ny)[member]; }
  __device__ __forceinline__ DpDrive drive() const {
    const double *f = dens_drive_table(a.members, (int)gridDim.y, a.ny) + 2 * (size_t)member;
    return DpDrive{f[0], f[1]};
  }
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
//
// LES: two fp64 square roots and one division more per cell, with TRT three divisions, in a kernel at 60-63 of 64 VGPRs and at its
// 80 SGPRs.  What keeps 31 of the 32 LES instances of either ensemble kernel at two workgroups per CU with 0 scratch: the rate is
// formed before the equilibrium and fenced, with TRT one division and one pair of speeds after the other (dp_collide_cell: without
// these two the TRT + WALL + LES instance spills 8 B); the
// three constants lie in LDS (kStageLes, 24 B) and are addressed from an opaque zero; the collision loop takes its cell from an
// opaque copy of the loop index; store_segments' lane is opaque (dp_tile.h).  The one instance that still spilled 8 B per lane
// under the hint, TRT + OPEN + WALL + LES without FORCE (with FORCE it fits), does not state it: left to itself the compiler
// schedules it into 64 VGPRs with 0 scratch, so it, too, runs two workgroups per CU (74 680 B of LDS).  Cross-compiled figures
// of all 32: DESIGN.md section 3.7, profiles/les_throughput.txt.
//
// DRIVE: the source of the body force is added behind the relaxation lines and fenced, the two components lie in 16 B of LDS
// (kStageDrive) and are read at each of their two uses (dp_collide_cell, dp_tile.h).  26 of the 32 DRIVE instances of either
// ensemble kernel have 64 VGPRs, 0 scratch; the six with LES and without OPEN that also have FORCE or WALL spill 8 B per lane under
// the hint and keep it: without it they take 66-68 VGPRs, which is one workgroup per CU.
template <int NT, bool FORCE, bool TRT, bool OPEN, bool WALL, bool LES, bool DRIVE = false>
constexpr int dens_waves_per_simd() {
  if (!DRIVE && !FORCE && TRT && OPEN && WALL && LES) return 1;
  return (FORCE || TRT || OPEN || WALL || LES || DRIVE) ? NT / 128 : 1;
}

template <int TX, int TY, int TMAX, int NT, bool FORCE, bool TRT, bool OPEN, bool WALL = false, bool LES = false, bool DRIVE = false>
__global__ __launch_bounds__(NT, (dens_waves_per_simd<NT, FORCE, TRT, OPEN, WALL, LES, DRIVE>())) void d2q9_dp_ensemble(const DensArgsOf<WALL> a) {
  dp_tile<TX, TY, TMAX, NT, FORCE, TRT, OPEN, WALL, LES, DRIVE, DensGrid<WALL>>(a);
}

}  // namespace lbm

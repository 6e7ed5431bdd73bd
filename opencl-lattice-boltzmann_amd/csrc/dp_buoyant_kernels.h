// The flow step of a handle whose scalar acts back on it (include/lbm.h, "Buoyancy"; lbm_dbuoy_*): one timestep per launch in
// d2q9_dp_step's lanes, with a force density per cell formed from the scalar's current array, for a context or for every member
// of an ensemble.
//
// With a scalar on every launch already advances one step (the scalar reads each step's velocities), so the LDS-tile kernels buy
// nothing here, and they have room for neither a second lattice nor a per-cell force (dp_tile.h: 152 of 160 KB of LDS, 62-64
// VGPRs).  dp_collide_cell takes its force through a callable; this kernel hands it one that returns the cell's own pair from
// registers.  No tile kernel, and no instance of d2q9_dp_step, is touched.
//
//   d2q9_dp_buoyant   lane = 2 neighbouring cells of a row, member axis on blockIdx.y, per-member constants from a DpBuoyMember
//                     table (dp_kernels.h; a context holds a table of one).  d2q9_dp_step's loads, its dp_segment_tree8 and its
//                     segment layout at the member's place in the ring, plus five 16-B loads of the scalar's planes: about 184 B
//                     per lattice update.  No LDS, no atomics.
//   d2q9_dp_buoyant_gated  the same lane body (dp_buoyant_lanes.inl) behind the members' `active` words, for the legs of a steady
//                     run on the scalar's record (include/lbm.h, "Scalar record")
//
// Why the lane body is written out here and not shared with d2q9_dp_step: that kernel takes every constant as a kernel argument
// and knows one grid, this one reads them from a table by member index and offsets every array by the member; a body shared by
// both would put an accessor layer (dp_tile.h's Grid) under d2q9_dp_step's 64 instances per unit, whose instructions a library
// without this option must keep.  The per-cell functions are the shared ones, so the cells are the same bits.
#pragma once
#include "dp_kernels.h"

namespace lbm {

// The pair dp_collide_cell asks for, held per cell (DpDriveHeld's is one pair per launch)
struct DpDriveCell {
  DpDrive f;
  __device__ __forceinline__ DpDrive operator()() const { return f; }
};

struct DpBuoyArgs {
  const double *src;         // member m: src + m * member_stride
  double *dst;
  const uint8_t *mask;       // member m: mask + m * nx * ny
  const double *scalar;      // the scalar's CURRENT array (the one the scalar step of this flow step wrote): member m
                             // m * 5 * plane_stride * ny in, g_k(x, y) at y * 5 * plane_stride + k * plane_stride + x
  const DpBuoyMember *members;
  const double *wall_u;      // WALL: [2][members][ny][nx], u_x then u_y
  double *seg;               // [members][ny][nseg] segment sums of this step; FORCE: [3][members][ny][nseg], |u|, F_x, F_y
  unsigned long long plane_stride, member_stride;
  int nx, ny;
  int lanes_per_row;         // as DpStepArgs
  int accel_row;             // row that gets the NEXT step's accelerate_flow, or -1
};

// One timestep of every member, lane = cells x0, x0+1 of one row of member blockIdx.y.  FORCE, TRT, OPEN, WALL, LES: as in
// d2q9_dp_step, on the member's constants.  The force of a cell is dp_buoy_force of its own five stored scalar values; a
// blocked cell takes none (dp_collide_cell's obstacle branch reads no force).
template <bool FORCE, bool TRT, bool OPEN, bool WALL = false, bool LES = false>
static __global__ __launch_bounds__(kBlock) void d2q9_dp_buoyant(const DpBuoyArgs a) {
#include "dp_buoyant_lanes.inl"
}

// d2q9_dp_buoyant behind a test of the members' `active` words, for a leg of a steady run (dp_steady_kernels.h): one copy of the
// arithmetic (dp_buoyant_lanes.inl); the workgroups of a stopped member return before they touch its cells or its segment sums,
// uniformly.
template <bool FORCE, bool TRT, bool OPEN, bool WALL = false, bool LES = false>
static __global__ __launch_bounds__(kBlock) void d2q9_dp_buoyant_gated(const DpBuoyArgs a, const int *active) {
  if (active[blockIdx.y] == 0) return;
#include "dp_buoyant_lanes.inl"
}

}  // namespace lbm

// Running statistics of the double-precision families (include/lbm.h, "Running statistics"): one kernel, dp_stats_sample, which
// adds one sample of the current state to six planes of sums per member.  The fields of a cell are dp_final_fields' (dp_output_cell
// on the nine stored values, with buoyancy on dp_buoy_force of the cell's five stored scalar values; a blocked cell gives 0, 0 and
// the member's density / 3), so a sample holds the bits lbm_dp_final_state would return at that step count.  No flow kernel, no
// argument struct and no helper kernel of dp_kernels.h changes with it.
// Its arguments are dp_final_fields' where they apply: cells, mask, members, drive, scalar and buoy.  cells_alt, par and scalar_alt
// do not: they place the members of a ragged ensemble, which refuses the statistics, as the steady runs that make one refuse to
// start while statistics are on.
//
// A streaming kernel: per cell 72 B of state, one mask byte, 48 B of sums read and 48 B written (with buoyancy 40 B of scalar more).
// Lanes run along x in d2q9_dp_step's geometry, two neighbouring cells per lane, x0 even: every load and store of a plane is 16 B a
// lane and a whole 1-KiB segment a wave, aligned because plane_stride is a multiple of 32 doubles, in the state as in the sums,
// which lie on the device as [members][6][ny][plane_stride].  For odd nx the row's last lane loads one double beyond the row,
// inside the plane's padding (plane_stride >= nx + 1 then), uses none of it, and adds +0.0 to the padding of the sums.
// A wave is 64 lanes of ONE row, a block four rows: the row of a lane comes from the block's index by one division that is uniform
// over the block, none per cell.  No LDS, no cross-lane work, no order of summation to fix.  The grid is capped (dp_host.h:
// stats_sample) and a block strides over the rows it does not reach at once.
// 70 VGPRs without buoyancy, 90 with (hipcc's kernel-resource-usage, profiles/stats_throughput.txt), no scratch: launch bounds of
// kBlock alone leave seven and five waves a SIMD, each lane with up to fifteen 16-B loads ahead of its first store.  That ran at
// 0.81 of the copy rate on an 8192 x 8192 grid, so no second launch bound squeezes the registers for more.
#pragma once
#include "dp_kernels.h"

namespace lbm {

struct DpStatsArgs {
  const double *cells;        // the current grid array; member m lies m * member_stride in
  const uint8_t *mask;        // [members][ny][nx]
  const DpMember *members;    // the density of a blocked cell's pressure
  const double *drive;        // NULL, or the members' body forces, double[members][2] (dp_final_fields' drive)
  const double *scalar;       // BUOY: the current scalar array, member m 5 * plane_stride * ny doubles in
  const DpBuoyMember *buoy;   // BUOY: the members' buoyant constants (drive is not read)
  double *sums;               // [members][6][ny][plane_stride]
  unsigned long long plane_stride, member_stride;
  int nx, ny;
  int xblocks;                // blocks along a row: ceil(ceil(nx / 2) / 64)
  int rowgroups;              // blocks along y; block r takes rows 4 r + wave, then every 4 * rowgroups rows on
};

constexpr int kStatsLanes = 64;                  // lanes of a block along x: one wave
constexpr int kStatsRows = kBlock / kStatsLanes; // rows of a block: one a wave

template <bool BUOY>
static __global__ __launch_bounds__(kBlock) void dp_stats_sample(const DpStatsArgs a) {
#pragma clang fp contract(off)
  const unsigned member = blockIdx.y;
  const unsigned rg = blockIdx.x / (unsigned)a.xblocks;   // uniform over the block
  const unsigned xb = blockIdx.x - rg * (unsigned)a.xblocks;
  const int x0 = 2 * (int)(xb * kStatsLanes + (threadIdx.x & (kStatsLanes - 1)));
  if (x0 >= a.nx) return;
  const bool has_b = x0 + 1 < a.nx;
  const size_t ps = a.plane_stride, plane = ps * (size_t)a.ny;
  const double blocked_pr = a.members[member].density * (1.0 / 3.0);   // dp_final_fields' density * c_sq
  const double *cells = a.cells + (size_t)member * a.member_stride + x0;
  const uint8_t *mask = a.mask + (size_t)member * ((size_t)a.nx * a.ny) + x0;
  double *sums = a.sums + (size_t)member * 6 * plane + x0;
  const double *drive = a.drive ? a.drive + 2 * (size_t)member : nullptr;
  const double *scalar = nullptr;
  DpBuoy bu{};
  if constexpr (BUOY) {
    bu = a.buoy[member].buoy;
    scalar = a.scalar + (size_t)member * 5 * plane + x0;
  }
  for (int y = (int)(rg * kStatsRows + (threadIdx.x >> 6)); y < a.ny; y += kStatsRows * a.rowgroups) {
    const double *c = cells + (size_t)y * 9 * ps;
    v2d f[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = *reinterpret_cast<const v2d *>(c + k * ps);
    const uint8_t *m = mask + (size_t)y * a.nx;
    const bool ob_a = m[0] != 0, ob_b = !has_b || m[1] != 0;
    double fa[9], fb[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
      fa[k] = f[k].x;
      fb[k] = f[k].y;
    }
    double pair_a[2], pair_b[2];
    const double *drv_a = drive, *drv_b = drive;
    if constexpr (BUOY) {
      const double *s = scalar + (size_t)y * 5 * ps;
      v2d g[5];
#pragma unroll
      for (int k = 0; k < 5; k++) g[k] = *reinterpret_cast<const v2d *>(s + k * ps);
      const double ga[5] = {g[0].x, g[1].x, g[2].x, g[3].x, g[4].x}, gb[5] = {g[0].y, g[1].y, g[2].y, g[3].y, g[4].y};
      const DpDrive da = dp_buoy_force(ga, bu), db = dp_buoy_force(gb, bu);
      pair_a[0] = da.f_x;
      pair_a[1] = da.f_y;
      pair_b[0] = db.f_x;
      pair_b[1] = db.f_y;
      drv_a = pair_a;
      drv_b = pair_b;
    }
    // a blocked cell: 0, 0 and the member's density / 3; the row's last lane of an odd nx has no second cell and adds +0.0
    double ux_a = 0.0, uy_a = 0.0, pr_a = blocked_pr, ux_b = 0.0, uy_b = 0.0, pr_b = has_b ? blocked_pr : 0.0, uu;
    if (!ob_a) dp_output_cell(fa, drv_a, ux_a, uy_a, uu, pr_a);
    if (!ob_b) dp_output_cell(fb, drv_b, ux_b, uy_b, uu, pr_b);
    const v2d v[6] = {{ux_a, ux_b}, {uy_a, uy_b}, {pr_a, pr_b}, {ux_a * ux_a, ux_b * ux_b}, {uy_a * uy_a, uy_b * uy_b},
                      {ux_a * uy_a, ux_b * uy_b}};
    double *sp = sums + (size_t)y * ps;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      v2d *p = reinterpret_cast<v2d *>(sp + k * plane);
      *p = *p + v[k];
    }
  }
}

}  // namespace lbm

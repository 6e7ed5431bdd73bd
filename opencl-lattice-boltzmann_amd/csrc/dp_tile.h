// The LDS-tile step of the double-precision families, written once: the body of d2q9_dp_multi (dp_kernels.h, one grid) and
// of d2q9_dp_ensemble / d2q9_dp_ensemble_gated (dp_ensemble_kernels.h, dp_steady_kernels.h: many grids, member = blockIdx.y).
// Each of those kernels names its Grid and calls dp_tile on its own argument struct; what a family does to find its grid
// (member offsets, the DpMember load, the tables behind it) is in its Grid and nowhere else, so a physics option is one
// edit here.  dp_kernels.h includes this file below the per-cell functions it is built on; it is not included on its own.
//
// What the two argument structs name alike, dp_tile reads from them: plane_stride, seg_step, nx, ny, nseg, tiles_x, T,
// accel_next.  A Grid is built from the argument struct and supplies what differs:
//   src, dst, mask, seg_out           this grid's or member's arrays, offsets applied
//   omega, omega_m, aw1, aw2          its run constants
//   comp()                            FORCE: the stride between the |u|, F_x and F_y components of a step's segment sums, 32 bits
//   u_in(), rho_out()                 OPEN: its inlet profile [ny] and its outlet density
//   wall_u_x(), wall_u_y()            WALL: the arrays that hold its wall velocities,
//   wall_cell0(), rho_wall()                its cell (0,0) in them, and its wall density
//   les()                             LES: its tau0, les_k and magic parameter (DpLes)
//   kStageLes                         LES: they go to LDS with the region, or are held in SGPRs
//   drive()                           DRIVE: its body force F_x, F_y (DpDrive)
//   kStageDrive                       DRIVE: they go to LDS with the region, or are held in SGPRs
//   kStageRhoOut                      the one switch: rho_out goes to LDS with the profile, or is read where it is used
// The option members are functions: an instance without the option never evaluates them, and one with it evaluates them where
// it uses them, under the branch of a marked cell, so no register holds a table's address across the loops (the ensemble runs
// at 62-63 of its 64 VGPRs and is short of SGPRs).  dp_tile builds the Grid itself, behind the tile's own place: the compiler's
// schedule follows the order of these statements, and in this order every ensemble instance is, instruction for instruction,
// the kernel that had this body to itself.  Of the four places where the two copies of this body had
// drifted apart, three have the ensemble's form in both families now (the pinned region load under WALL, the opaque lane of
// store_segments, a 32-bit component stride); the fourth is kStageRhoOut.
#pragma once

namespace lbm {

// NT threads, TX x TY output tile, T <= TMAX timesteps per launch: a (TX + 2T) x (TY + 2T) region around the tile is loaded
// into LDS, advanced T times LDS -> LDS on a region that shrinks by one cell per step (halo cells computed redundantly by the
// neighbouring tiles; x and y wrap inside the grid), and the central tile is stored (d2q9_multi's scheme, d2q9_kernels.h).  Each
// step's |u| of the tile's cells goes to an LDS tile of its own; one lane per 16-cell segment adds it up in the segment tree
// of dp_kernels.h while the next step runs.  Tile shapes and depths are each family's own choice, measured beside its kernel.
//
// FORCE (the option "force": the momentum-exchange force on the blocked cells, include/lbm.h): a blocked cell of the tile has
// both values of every link in lds[in] and the neighbours' bytes in lmask; a pass of one lane per tile cell before each step's
// collision loop evaluates dp_force_cell there.  Two more double-buffered LDS tiles beside tval would cost the ensemble its two
// workgroups per CU (74 276 + 8 192 B; 28.8 against 20.3 us), and single-buffered ones put a barrier and the segment lanes' sums
// on every step's critical path (28.7 us, as bad).  The pass needs neither: F_x and F_y never touch LDS, a segment's sixteen
// lanes add them in registers in the tree's order.  No LDS beyond the FORCE = false instance's.
//
// TRT (the two-relaxation-time collision): dp_collide_cell<true> in the collision loop, nothing else.
//
// OPEN (velocity inlet on column 0, pressure outlet on column nx - 1): the fix keys on the GRID column of every region cell (a
// tile at one end of the grid recomputes cells of the other end in its halo, and a region wider than nx holds column 0 more
// than once).  The region load, which has the grid column, marks the fluid cells of the two columns in two spare bits of their
// lmask byte; the collision loop branches on the byte it reads anyway, applies dp_open_inlet / dp_open_outlet to a marked cell
// before dp_collide_cell and has no accelerate_flow.  Blocked-ness is the low two bits, the neighbour bytes of the force pass
// included.  The profile on the region's rows and, where it lies in global memory (kStageRhoOut), rho_out are staged in LDS with
// the region (8 (kRY + 1) B; reading them from global memory under the branch put a load's latency on every step of an end
// tile: 23.2 against 19.6 us/step on an ensemble of 64 x 128x128).
//
// WALL (a wall velocity per blocked cell): two doubles per region cell would be 16 KB more LDS in d2q9_dp_multi, which holds
// 152 of 160 KB, and 7 744 B in the ensemble, whose 74 472 B must stay at or below 81 920 for two workgroups per CU; a moving
// cell is rare.  A pass behind the region load reads the two velocities of every blocked cell by its grid cell and marks one that
// moves in a third spare bit of its byte (kWallMoving); a pass behind the collision loop finds the grid cell of a marked byte
// from its region cell (the region's rows and columns in the grid are staged in LDS as gy * nx and gx, 4 (kRY + kRX) B; nx * ny
// is below 2^31 for every grid whose two arrays a device holds), reads the two values and rho_wall from global memory under
// that branch and adds dp_wall_cell's terms to the bounce-back in LDS.  Every copy of a wall cell in a region wider than the
// grid gets the velocity of its own grid cell.  With the branch inside the collision loop the compiler, at the ensemble's 64
// VGPRs, issued the nine plane loads of the region load one after the other: 29.5 against 19.5 us/step on 64 x 128x128 with a
// spinning disc, 25.8 now (tools/wall_ab.py).
//
// LES (the Smagorinsky subgrid viscosity): dp_collide_cell<TRT, true> on g.les() in the collision loop, nothing else.
//
// DRIVE (a uniform body force, Guo forcing): dp_collide_cell<TRT, LES, true> on g.drive() in the collision loop, nothing else.  The
// two components are wave-uniform: held in SGPRs, or, where the kernel has none to spare (kStageDrive), in 16 B of LDS beside the
// subgrid constants and read per cell from an opaque zero, as those are.
//
// The false instance of each flag is the kernel without it, instruction for instruction.
template <int TX, int TY, int TMAX, int NT, bool FORCE, bool TRT, bool OPEN, bool WALL, bool LES, bool DRIVE, class Grid, class Args>
__device__ __forceinline__ void dp_tile(const Args a) {
  constexpr bool MARKED = OPEN || WALL;   // lmask bytes carry marks above the low two bits
  static_assert(TX % kDpSeg == 0, "a tile row is whole segments");
  static_assert(TY * (TX / kDpSeg) <= NT, "one lane per segment of the tile");
  constexpr int kRX = TX + 2 * TMAX, kRY = TY + 2 * TMAX;
  __shared__ double lds[2][9][kRY * kRX];
  __shared__ uint8_t lmask[kRY * kRX];
  __shared__ double tval[2][TY][TX];
  const int tid = threadIdx.x;
  const int T = a.T;
  const int RX = TX + 2 * T, RY = TY + 2 * T;
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
  const int gx0 = tile_x * TX - T, gy0 = tile_y * TY - T;  // region cell (0,0)
  const size_t ps = a.plane_stride, rs = 9 * ps;
  const Grid g(a);   // here, not in the kernel: see the head of this file
  // LES: the three constants, read once, before the kernel's first store to global memory (behind one, a load by member index
  // is a vector load under the collision loop's branch, every cell: four VGPRs and twenty scalar instructions of address
  // arithmetic).  kStageLes: into LDS with the region, where six more SGPRs held across the loops would be spilled to the lanes
  // of a VGPR that the kernel does not have (the ensemble's instances are at their 80 SGPRs); else into SGPRs here.
  [[maybe_unused]] DpLes les{};
  [[maybe_unused]] double *lles = nullptr;
  if constexpr (LES) {
    if constexpr (Grid::kStageLes) {
      __shared__ double les_consts[3];
      lles = les_consts;
    } else {
      les = g.les();
    }
  }
  // DRIVE: the two components, read once like the subgrid constants, into LDS (kStageDrive) or into SGPRs
  [[maybe_unused]] DpDrive drv{};
  [[maybe_unused]] double *ldrv = nullptr;
  if constexpr (DRIVE) {
    if constexpr (Grid::kStageDrive) {
      __shared__ double drive_consts[2];
      ldrv = drive_consts;
    } else {
      drv = g.drive();
    }
  }
  // OPEN: the profile on the region's rows and, behind them, rho_out (kStageRhoOut), staged in LDS with the region: a marked cell
  // reads them under its branch without a global load on a step's critical path, and no register holds an address across the loops
  [[maybe_unused]] double *lopen = nullptr;
  if constexpr (OPEN) {
    __shared__ double open_rows[kRY + (Grid::kStageRhoOut ? 1 : 0)];
    lopen = open_rows;
  }
  // WALL: where the region's rows and columns lie in the grid, gy * nx per row and then gx per column, staged with the region:
  // a moving cell finds its two velocities without a division in the step loop
  [[maybe_unused]] int *lwall = nullptr;
  if constexpr (WALL) {
    __shared__ int wall_cells[kRY + kRX];
    lwall = wall_cells;
  }
  // grid row of region row ry: periodic wrap (kernels.cl:91-93)
  auto grid_row = [&](int ry) {
    int r = (gy0 + ry) % a.ny;
    return r < 0 ? r + a.ny : r;
  };
  // segment sums of step s (1-based) from tval[s & 1]
  auto store_segments = [&](int s) {
    constexpr int kSegs = TY * (TX / kDpSeg);
    int lane = tid;
    // as in the force pass below: nothing of this is kept across the collision loop (WALL: its branch needs the registers)
    if constexpr (FORCE || WALL || LES || DRIVE) asm volatile("" : "+v"(lane));
    if (lane < kSegs) {
      const int oy = lane / (TX / kDpSeg), sx = lane - oy * (TX / kDpSeg);
      const int gy = tile_y * TY + oy;
      const double *v = &tval[s & 1][oy][sx * kDpSeg];
      double p[8];
#pragma unroll
      for (int i = 0; i < 8; i++) p[i] = v[2 * i] + v[2 * i + 1];
      const double tot = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
      const int seg = tile_x * (TX / kDpSeg) + sx;
      if (gy < a.ny && seg < a.nseg) g.seg_out[(size_t)(s - 1) * a.seg_step + (size_t)gy * a.nseg + seg] = tot;
    }
  };

  // region -> LDS (periodic wrap in x, kernels.cl:99-102)
  const float rinv = 1.0f / (float)RX;
  for (int i = tid; i < RX * RY; i += NT) {
    const int ry = (int)(((float)i + 0.5f) * rinv), rx = i - ry * RX;
    int gx = (gx0 + rx) % a.nx;
    if (gx < 0) gx += a.nx;
    const int gy = grid_row(ry);
    const double *p = g.src + (size_t)gy * rs + gx;
    if constexpr (WALL) {
      // At the 64 VGPRs of two workgroups per CU the compiler issues the nine loads of a WALL instance one after the other,
      // each waited for before the next (29.5 against 19.5 us/step on 64 x 128x128).  One statement that takes all nine values
      // keeps them in flight together, as the WALL = false instances have them.
      double v[9];
#pragma unroll
      for (int k = 0; k < 9; k++) v[k] = p[k * ps];
      asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]));
#pragma unroll
      for (int k = 0; k < 9; k++) lds[0][k][ry * kRX + rx] = v[k];
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++) lds[0][k][ry * kRX + rx] = p[k * ps];
    }
    uint8_t mb = g.mask[(size_t)gy * a.nx + gx];
    if constexpr (OPEN) {
      if (mb == 0 && gx == 0) mb = kOpenInlet;
      if (mb == 0 && gx == a.nx - 1) mb = kOpenOutlet;
    }
    lmask[ry * kRX + rx] = mb;
  }
  if constexpr (OPEN) {
    static_assert(kRY + 1 <= NT, "one lane per region row");
    const double *u_in = g.u_in();
    if (tid < RY) lopen[tid] = u_in[grid_row(tid)];
    if constexpr (Grid::kStageRhoOut)
      if (tid == RY) lopen[kRY] = g.rho_out();
  }
  if constexpr (LES && Grid::kStageLes) {
    if (tid == 0) {
      const DpLes l = g.les();
      lles[0] = l.tau0, lles[1] = l.les_k, lles[2] = l.magic;
    }
  }
  if constexpr (DRIVE && Grid::kStageDrive) {
    if (tid == 64) {   // the second wave's first lane: the first's stages the subgrid constants
      const DpDrive d = g.drive();
      ldrv[0] = d.f_x, ldrv[1] = d.f_y;
    }
  }
  if constexpr (WALL) {
    // The marks, in a pass of its own: every lane revisits the bytes it wrote itself (no barrier) and reads the two velocities
    // of a blocked cell.  From an opaque copy of the lane index, as the force pass: nothing of this is kept in registers across
    // the region load, whose nine plane loads the compiler otherwise issues one after the other.
    int mine = tid;
    asm volatile("" : "+v"(mine));
    for (int i = mine; i < RX * RY; i += NT) {
      const int ry = (int)(((float)i + 0.5f) * rinv), rx = i - ry * RX;
      const uint8_t mb = lmask[ry * kRX + rx];
      if ((mb & kOpenBlocked) != 0) {
        int gx = (gx0 + rx) % a.nx;
        if (gx < 0) gx += a.nx;
        const size_t at = g.wall_cell0() + (size_t)grid_row(ry) * a.nx + gx;
        const double *u_y = g.wall_u_y();
        if (dp_wall_moves(g.wall_u_x()[at], u_y[at])) lmask[ry * kRX + rx] = mb | kWallMoving;
      }
    }
    static_assert(kRY + kRX <= NT, "one lane per region row and column");
    if (mine < RY) {
      lwall[mine] = grid_row(mine) * a.nx;
    } else if (mine < RY + RX) {
      int gx = (gx0 + mine - RY) % a.nx;
      lwall[kRY + mine - RY] = gx < 0 ? gx + a.nx : gx;
    }
  }
  __syncthreads();

  for (int s = 1; s <= T; s++) {
    if (s > 1) store_segments(s - 1);
    if constexpr (FORCE) {
      // The force of step s, from the state it streams (lds[in]): one lane per cell of the tile (every one, and its eight
      // neighbours, is inside the region of every step; cells past the grid's edge and fluid cells count +0.0), sixteen
      // neighbouring lanes = one row segment.  The segment tree of store_segments over those lanes in registers
      // (dp_segment_tree16: every lane ends with the tree's bits), and the segment's first lane stores F_x and F_y one and two
      // components (g.comp()) behind |u|.  No LDS, no barrier: the pass reads what the last barrier published and writes only
      // global memory.  A pass of its own, from an opaque copy of the lane index, so that the collision loop below is the
      // FORCE = false one and keeps nothing of this in registers.
      static_assert(kDpSeg == 16 && (TX * TY) % 64 == 0 && NT % 64 == 0, "whole waves of whole segments take the butterfly");
      int first = tid;
      asm volatile("" : "+v"(first));
      static_assert(TX * TY <= NT, "one lane per cell of the tile");
      if (const int i = first; i < TX * TY) {
        const int oy = i / TX, ox = i - oy * TX;
        const int c = (oy + T) * kRX + ox + T;
        const int gy = tile_y * TY + oy;
        double fx = 0.0, fy = 0.0;
        // 2: blocked, outside the body; WALL: a moving cell's byte carries its mark
        const bool counts = (WALL ? lmask[c] & kOpenBlocked : lmask[c]) == 1 && tile_x * TX + ox < a.nx && gy < a.ny;
        if (counts) {
          const double(*f)[kRY * kRX] = lds[(s - 1) & 1];
          const double gth[9] = {0.0, f[1][c - 1], f[2][c - kRX], f[3][c + 1], f[4][c + kRX], f[5][c - kRX - 1],
                                 f[6][c - kRX + 1], f[7][c + kRX + 1], f[8][c + kRX - 1]};
          double own[9];
#pragma unroll
          for (int k = 0; k < 9; k++) own[k] = f[k][c];
          // OPEN: a marked fluid neighbour reads as fluid; WALL: a marked moving one as blocked
          auto nbyte = [&](int at) -> uint8_t { return MARKED ? (uint8_t)(lmask[at] & kOpenBlocked) : lmask[at]; };
          const uint8_t nb[9] = {0, nbyte(c - 1), nbyte(c - kRX), nbyte(c + 1), nbyte(c + kRX), nbyte(c - kRX - 1),
                                 nbyte(c - kRX + 1), nbyte(c + kRX + 1), nbyte(c + kRX - 1)};
          dp_force_cell(gth, own, nb, fx, fy);
        }
        if (__ballot(counts) != 0ull) {   // a wave without a counting cell adds +0.0 to +0.0
          fx = dp_segment_tree16(fx);
          fy = dp_segment_tree16(fy);
        }
        const int seg = tile_x * (TX / kDpSeg) + ox / kDpSeg;
        if ((ox & (kDpSeg - 1)) == 0 && gy < a.ny && seg < a.nseg) {
          double *at = g.seg_out + (size_t)(s - 1) * a.seg_step + (size_t)gy * a.nseg + seg;
          const unsigned comp = g.comp();   // below 2^31 in both families (the create calls' bounds)
          at[comp] = fx;
          at[2 * (size_t)comp] = fy;
        }
      }
    }
    const int in = (s - 1) & 1, out = s & 1;
    const int w = RX - 2 * s, h = RY - 2 * s;
    [[maybe_unused]] const bool accel_step = (s < T) || a.accel_next;
    const float inv = 1.0f / (float)w;
    for (int i = tid; i < w * h; i += NT) {
      // LES: the cell from an opaque copy of i.  Otherwise the compiler carries four sums of the lane index, the step and a
      // constant across the step loop, one for each use below, and the instance with all five options is one VGPR short.
      int at = i;
      if constexpr (LES || DRIVE) asm volatile("" : "+v"(at));
      const int q = (int)(((float)at + 0.5f) * inv);
      const int rx = s + (at - q * w), ry = s + q;
      const int c = ry * kRX + rx;
      double gth[9], o[9];
      gth[0] = lds[in][0][c];
      gth[1] = lds[in][1][c - 1];
      gth[2] = lds[in][2][c - kRX];
      gth[3] = lds[in][3][c + 1];
      gth[4] = lds[in][4][c + kRX];
      gth[5] = lds[in][5][c - kRX - 1];
      gth[6] = lds[in][6][c - kRX + 1];
      gth[7] = lds[in][7][c + kRX + 1];
      gth[8] = lds[in][8][c + kRX - 1];
      const uint8_t mb = lmask[c];
      const bool obst = MARKED ? (mb & kOpenBlocked) != 0 : mb != 0;
      if constexpr (OPEN) {
        if (mb & kOpenInlet) dp_open_inlet(gth, lopen[ry]);
        else if (mb & kOpenOutlet) dp_open_outlet(gth, Grid::kStageRhoOut ? lopen[kRY] : g.rho_out());
      }
      if constexpr (LES && Grid::kStageLes) {
        // from an opaque zero: the address is formed here, per cell; as constants the compiler holds it across the loops, in
        // two VGPRs (one for tau0 and les_k, one for magic)
        int zero = 0;
        asm volatile("" : "+v"(zero));
        les = DpLes{lles[zero], lles[zero + 1], TRT ? lles[zero + 2] : 0.0};
      }
      double t;
      if constexpr (DRIVE && Grid::kStageDrive) {
        // from an opaque zero, at each of the collision's two uses: no register holds the pair, or its address, in between
        auto staged = [ldrv]() {
          int zero = 0;
          asm volatile("" : "+v"(zero));
          return DpDrive{ldrv[zero], ldrv[zero + 1]};
        };
        t = dp_collide_cell<TRT, LES, DRIVE>(gth, obst, g.omega, g.omega_m, les, staged, o);
      } else {
        t = dp_collide_cell<TRT, LES, DRIVE>(gth, obst, g.omega, g.omega_m, les, DpDriveHeld{drv}, o);
      }
      if constexpr (!OPEN)
        if (accel_step && grid_row(ry) == a.ny - 2) dp_accelerate_cell(o, obst, g.aw1, g.aw2);
#pragma unroll
      for (int k = 0; k < 9; k++) lds[out][k][c] = o[k];
      // the tile's own cells: every one is inside the region of every step; cells past the grid's edge count 0
      const int ox = rx - T, oy = ry - T;
      if (ox >= 0 && ox < TX && oy >= 0 && oy < TY)
        tval[s & 1][oy][ox] = (tile_x * TX + ox < a.nx && tile_y * TY + oy < a.ny) ? t : 0.0;
    }
    if constexpr (WALL) {
      // The moving cells, in a pass of its own behind the collision loop, which stays the WALL = false one: every lane
      // revisits the cells it wrote itself (no barrier), and one whose byte is marked adds the wall's terms to the bounce-back
      // it stored.  From an opaque copy of the lane index, as the force pass.
      int first = tid;
      asm volatile("" : "+v"(first));
      for (int i = first; i < w * h; i += NT) {
        const int q = (int)(((float)i + 0.5f) * inv);
        const int rx = s + (i - q * w), ry = s + q;
        const int c = ry * kRX + rx;
        if (lmask[c] & kWallMoving) {
          const size_t at = g.wall_cell0() + (size_t)(lwall[ry] + lwall[kRY + rx]);
          double o[9];
#pragma unroll
          for (int k = 1; k < 9; k++) o[k] = lds[out][k][c];
          const double *u_y = g.wall_u_y();
          dp_wall_cell(o, g.wall_u_x()[at], u_y[at], g.rho_wall());
#pragma unroll
          for (int k = 1; k < 9; k++) lds[out][k][c] = o[k];
        }
      }
    }
    __syncthreads();
  }
  store_segments(T);

  // central tile -> global
  const int fin = T & 1;
  for (int i = tid; i < TX * TY; i += NT) {
    const int oy = i / TX, ox = i - oy * TX;
    const int gx = tile_x * TX + ox, gy = tile_y * TY + oy;
    if (gx < a.nx && gy < a.ny) {
      const int c = (oy + T) * kRX + ox + T;
      double *d = g.dst + (size_t)gy * rs + gx;
#pragma unroll
      for (int k = 0; k < 9; k++) d[k * ps] = lds[fin][k][c];
    }
  }
}

}  // namespace lbm

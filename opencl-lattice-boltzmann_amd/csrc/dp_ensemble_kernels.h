// Device side of a DOUBLE-PRECISION ENSEMBLE (include/lbm.h: lbm_dens_*): N independent fp64 grids of one size, each with
// its own run constants, obstacle map and state, advanced by one launch per (up to) TMAX timesteps.
//
// d2q9_dp_ensemble is d2q9_dp_multi (dp_kernels.h) with a member axis, the way d2q9_ensemble (ensemble_kernels.h) is
// d2q9_multi's: member = blockIdx.y, tile = blockIdx.x; a member's two grids, mask and segment sums lie a member stride
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

// grid = (tiles per member, members), NT threads.  TX x TY output tile, T <= TMAX steps LDS -> LDS on a region that shrinks
// by one cell per step (d2q9_dp_multi's scheme; halo cells are computed redundantly by the member's neighbouring tiles).
// Each step's |u| of the tile's cells goes to an LDS tile of its own; one lane per 16-cell segment adds it up in the
// segment tree of dp_kernels.h while the next step runs.  The body is d2q9_dp_multi's with member offsets, the DensMember
// load and NT: a change to that kernel's loops has to be mirrored here (tests/test_dp_ensemble_gpu.py pins the bits).
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
// The tile body is a function of its own so that the gated kernel of a steady run (dp_steady_kernels.h) advances a member
// with the very same instructions.
//
// FORCE (the option "force": the momentum-exchange force on the blocked cells, include/lbm.h): d2q9_dp_multi's pass, before
// each step's collision loop.  Two more double-buffered LDS tiles beside tval would bring 16 x 16 at T <= 3 to 74 276 + 8 192 =
// 82 468 B, one workgroup per CU (the 28.8 against 20.3 us of the table above), and single-buffered ones put a barrier and the
// segment lanes' sums on every step's critical path (measured: 28.7 us, as bad).  The pass needs neither: F_x and F_y never
// touch LDS, a segment's sixteen lanes add them in registers in the tree's order.  74 280 B in both instances.
//
// TRT (lbm_dtrt_*: the two-relaxation-time collision): dp_collide_cell<true> with the member's omega_m in the collision
// loop, nothing else.  An ensemble is all TRT or all BGK, so no instance branches per member.
//
// OPEN (lbm_dopen_*: velocity inlet on column 0, pressure outlet on column nx - 1): d2q9_dp_multi's scheme.  The region load
// marks the fluid cells of the two columns in spare bits of their lmask byte, the collision loop applies dp_open_inlet /
// dp_open_outlet to a marked cell before dp_collide_cell and has no accelerate_flow.  The member's u_in on the region's rows
// and its rho_out are staged in LDS with the region (184 B; reading them from global memory under the branch put a load's
// latency on every step of an end tile: 23.2 against 19.6 us/step on 64 x 128x128).  An ensemble is all open or all periodic.
//
// WALL (lbm_dwall_*: a wall velocity per blocked cell): d2q9_dp_multi's scheme.  The 74 472 B of LDS must stay at or below 81 920
// for two workgroups per CU, and two doubles per region cell would be 7 744 B; a moving cell is rare.  A pass behind the region
// load reads the two velocities of every blocked cell by its grid cell and marks one that moves in a third spare bit of its
// lmask byte; a pass behind the collision loop finds the grid cell of a marked byte (the region's rows and columns in the grid
// are staged in LDS, 176 B), reads the member's two values and its rho_wall from global memory under that branch and adds
// dp_wall_cell's terms to the bounce-back in LDS.  With the branch inside the collision loop the compiler, at the 64 VGPRs of
// two workgroups per CU, issued the nine plane loads of the region load one after the other: 29.5 against 19.5 us/step on
// 64 x 128x128 with a spinning disc, 25.8 now (tools/wall_ab.py).  74 464 B of LDS without and 74 656 B with OPEN.  An ensemble
// has wall velocities on or off for all members; a member without a moving cell takes the branch nowhere.
template <int TX, int TY, int TMAX, int NT, bool FORCE, bool TRT, bool OPEN, bool WALL = false>
__device__ __forceinline__ void dens_tile(const DensArgsOf<WALL> a) {
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
  const int member = blockIdx.y;
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
  const int gx0 = tile_x * TX - T, gy0 = tile_y * TY - T;  // region cell (0,0)
  const size_t ps = a.plane_stride, rs = 9 * ps;
  const double *const src = a.src + (size_t)member * a.member_stride;
  double *const dst = a.dst + (size_t)member * a.member_stride;
  const uint8_t *const mask = a.mask + (size_t)member * ((size_t)a.nx * a.ny);
  double *const seg_out = a.seg + (size_t)member * ((size_t)a.ny * a.nseg);
  const DensMember mc = a.members[member];
  // OPEN: the member's profile on the region's rows and, behind them, its rho_out, staged in LDS with the region: a marked
  // cell reads them under its branch without a global load on a step's critical path, and no register holds an address
  // across the loops.  184 B.
  [[maybe_unused]] double *lopen = nullptr;
  if constexpr (OPEN) {
    __shared__ double open_rows[kRY + 1];
    lopen = open_rows;
  }
  // WALL: where the region's rows and columns lie in the member's grid, gy * nx per row and then gx per column, staged with the
  // region (176 B): a moving cell finds its two velocities without a division in the step loop
  [[maybe_unused]] int *lwall = nullptr;
  if constexpr (WALL) {
    __shared__ int wall_cells[kRY + kRX];
    lwall = wall_cells;
  }
  // grid row of region row ry: periodic wrap inside the member (kernels.cl:91-93)
  auto grid_row = [&](int ry) {
    int r = (gy0 + ry) % a.ny;
    return r < 0 ? r + a.ny : r;
  };
  // segment sums of step s (1-based) from tval[s & 1]
  auto store_segments = [&](int s) {
    constexpr int kSegs = TY * (TX / kDpSeg);
    int lane = tid;
    // as in the force pass below: nothing of this is kept across the collision loop (WALL: its branch needs the registers)
    if constexpr (FORCE || WALL) asm volatile("" : "+v"(lane));
    if (lane < kSegs) {
      const int oy = lane / (TX / kDpSeg), sx = lane - oy * (TX / kDpSeg);
      const int gy = tile_y * TY + oy;
      const double *v = &tval[s & 1][oy][sx * kDpSeg];
      double p[8];
#pragma unroll
      for (int i = 0; i < 8; i++) p[i] = v[2 * i] + v[2 * i + 1];
      const double tot = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
      const int seg = tile_x * (TX / kDpSeg) + sx;
      if (gy < a.ny && seg < a.nseg) seg_out[(size_t)(s - 1) * a.seg_step + (size_t)gy * a.nseg + seg] = tot;
    }
  };

  // region -> LDS (periodic wrap in x, kernels.cl:99-102)
  const float rinv = 1.0f / (float)RX;
  for (int i = tid; i < RX * RY; i += NT) {
    const int ry = (int)(((float)i + 0.5f) * rinv), rx = i - ry * RX;
    int gx = (gx0 + rx) % a.nx;
    if (gx < 0) gx += a.nx;
    const int gy = grid_row(ry);
    const double *p = src + (size_t)gy * rs + gx;
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
    uint8_t mb = mask[(size_t)gy * a.nx + gx];
    if constexpr (OPEN) {
      if (mb == 0 && gx == 0) mb = kOpenInlet;
      if (mb == 0 && gx == a.nx - 1) mb = kOpenOutlet;
    }
    lmask[ry * kRX + rx] = mb;
  }
  if constexpr (OPEN) {
    static_assert(kRY + 1 <= NT, "one lane per region row");
    const double *u_in = dens_open_table(a.members, (int)gridDim.y) + (size_t)member * (a.ny + 1);
    if (tid < RY) lopen[tid] = u_in[grid_row(tid)];
    if (tid == RY) lopen[kRY] = u_in[a.ny];
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
        const size_t at = (size_t)member * ((size_t)a.nx * a.ny) + (size_t)grid_row(ry) * a.nx + gx;
        const double *u_y = a.wall_u + (size_t)gridDim.y * ((size_t)a.nx * a.ny);
        if (dp_wall_moves(a.wall_u[at], u_y[at])) lmask[ry * kRX + rx] = mb | kWallMoving;
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
      // (dp_segment_tree16: every lane ends with the tree's bits), and the segment's first lane stores F_x
      // and F_y one and two components (members * ny * nseg each) behind |u|.  No LDS, no barrier: the pass reads what the last barrier
      // published and writes only global memory.  A pass of its own, from an opaque copy of the lane index, so that the
      // collision loop below is the FORCE = false one and keeps nothing of this in registers.
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
          const double g[9] = {0.0, f[1][c - 1], f[2][c - kRX], f[3][c + 1], f[4][c + kRX], f[5][c - kRX - 1],
                               f[6][c - kRX + 1], f[7][c + kRX + 1], f[8][c + kRX - 1]};
          double own[9];
#pragma unroll
          for (int k = 0; k < 9; k++) own[k] = f[k][c];
          // OPEN: a marked fluid neighbour reads as fluid; WALL: a marked moving one as blocked
          auto nbyte = [&](int at) -> uint8_t { return MARKED ? (uint8_t)(lmask[at] & kOpenBlocked) : lmask[at]; };
          const uint8_t nb[9] = {0, nbyte(c - 1), nbyte(c - kRX), nbyte(c + 1), nbyte(c + kRX), nbyte(c - kRX - 1),
                                 nbyte(c - kRX + 1), nbyte(c + kRX + 1), nbyte(c + kRX - 1)};
          dp_force_cell(g, own, nb, fx, fy);
        }
        if (__ballot(counts) != 0ull) {   // a wave without a counting cell adds +0.0 to +0.0
          fx = dp_segment_tree16(fx);
          fy = dp_segment_tree16(fy);
        }
        const int seg = tile_x * (TX / kDpSeg) + ox / kDpSeg;
        if ((ox & (kDpSeg - 1)) == 0 && gy < a.ny && seg < a.nseg) {
          double *at = seg_out + (size_t)(s - 1) * a.seg_step + (size_t)gy * a.nseg + seg;
          const unsigned comp = gridDim.y * (unsigned)(a.ny * a.nseg);   // members * ny * nseg < 2^31 (lbm_dens_create's bounds)
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
      const int q = (int)(((float)i + 0.5f) * inv);
      const int rx = s + (i - q * w), ry = s + q;
      const int c = ry * kRX + rx;
      double g[9], o[9];
      g[0] = lds[in][0][c];
      g[1] = lds[in][1][c - 1];
      g[2] = lds[in][2][c - kRX];
      g[3] = lds[in][3][c + 1];
      g[4] = lds[in][4][c + kRX];
      g[5] = lds[in][5][c - kRX - 1];
      g[6] = lds[in][6][c - kRX + 1];
      g[7] = lds[in][7][c + kRX + 1];
      g[8] = lds[in][8][c + kRX - 1];
      const uint8_t mb = lmask[c];
      const bool obst = MARKED ? (mb & kOpenBlocked) != 0 : mb != 0;
      if constexpr (OPEN) {
        if (mb & kOpenInlet) dp_open_inlet(g, lopen[ry]);
        else if (mb & kOpenOutlet) dp_open_outlet(g, lopen[kRY]);
      }
      const double t = dp_collide_cell<TRT>(g, obst, mc.omega, mc.omega_m, o);
      if constexpr (!OPEN)
        if (accel_step && grid_row(ry) == a.ny - 2) dp_accelerate_cell(o, obst, mc.aw1, mc.aw2);
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
          const size_t at = (size_t)member * ((size_t)a.nx * a.ny) + (size_t)(lwall[ry] + lwall[kRY + rx]);
          double o[9];
#pragma unroll
          for (int k = 1; k < 9; k++) o[k] = lds[out][k][c];
          const double *u_y = a.wall_u + (size_t)gridDim.y * ((size_t)a.nx * a.ny);
          dp_wall_cell(o, a.wall_u[at], u_y[at], dens_wall_table(a.members, (int)gridDim.y, a.ny)[member]);
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
      double *d = dst + (size_t)gy * rs + gx;
#pragma unroll
      for (int k = 0; k < 9; k++) d[k * ps] = lds[fin][k][c];
    }
  }
}

// The FORCE instance states its two workgroups per CU (NT / 128 waves per SIMD) to the compiler: 60 VGPRs, 78 SGPRs, 0 scratch.
// So do the TRT and the OPEN instances (DESIGN.md section 3.7 holds their tables).
template <int TX, int TY, int TMAX, int NT, bool FORCE, bool TRT, bool OPEN, bool WALL = false>
__global__ __launch_bounds__(NT, (FORCE || TRT || OPEN || WALL) ? NT / 128 : 1) void d2q9_dp_ensemble(const DensArgsOf<WALL> a) {
  dens_tile<TX, TY, TMAX, NT, FORCE, TRT, OPEN, WALL>(a);
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
  __shared__ double wsum[kBlock / 64];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wsum[0];
    for (int i = 1; i < kBlock / 64; i++) t += wsum[i];
    out[(size_t)blockIdx.z * out_member + (size_t)blockIdx.y * out_stride + blockIdx.x] = t;
  }
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
      double local_density = 0.0;
      const size_t y = i / nx;
      const size_t cell = y * 9 * plane_stride + (i - y * nx);
#pragma unroll
      for (int k = 0; k < 9; k++) {
        f[k] = cells[k * plane_stride + cell];
        local_density += f[k];
      }
      ux = (f[1] + f[5] + f[8] - f[3] - f[6] - f[7]) / local_density;
      uy = (f[2] + f[5] + f[6] - f[4] - f[7] - f[8]) / local_density;
      uu = __builtin_sqrt(ux * ux + uy * uy);
      pr = local_density * c_sq;
      tot_u += uu;
    }
    if (u_x) u_x[off + i] = ux;
    if (u_y) u_y[off + i] = uy;
    if (u) u[off + i] = uu;
    if (pressure) pressure[off + i] = pr;
  }
  __shared__ double wsum[kBlock / 64];
  tot_u = wave_sum(tot_u);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = tot_u;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wsum[0];
    for (int i = 1; i < kBlock / 64; i++) t += wsum[i];
    partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

}  // namespace lbm

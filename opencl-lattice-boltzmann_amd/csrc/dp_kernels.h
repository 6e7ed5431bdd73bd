// Device side of the DOUBLE-PRECISION contexts (include/lbm.h: lbm_dp_*): the reference's accelerate_flow + timestep
// (kernels.cl:9-53, 56-231) with every distribution, density, momentum and velocity in fp64, as in the fp64 ancestor that
// wrote the reference's golden files (check/*.dat).
//
// Layout: the row-interleaved SoA of d2q9_kernels.h in double — f_k(x, y) at y*9*plane_stride + k*plane_stride + x, plane_stride
// a multiple of 32 doubles (256 B).  A lane holds two neighbouring cells (x0 even, one 16-B load per plane), so the nine loads
// and nine stores of a wave are whole 1-KiB segments as in the fp32 kernels.  The mask is one byte per cell.
//
// Two kernel forms, both built on dp_collide_cell / dp_accelerate_cell (bit-identical cells):
//   d2q9_dp_step    one timestep per launch, lane = 2 cells; the bandwidth-bound form (144 B per lattice update)
//   d2q9_dp_multi   T <= 8 timesteps per launch on an LDS-resident tile with redundant halo (d2q9_multi's scheme);
//                   launch-bound small grids
// and one reduction that does not depend on the form: every kernel writes the sum of |u| over each 16-cell row segment
// (x = 16s .. 16s+15 of row y) in one fixed tree, ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)) with p_i the sum of cells 2i, 2i+1,
// and dp_reduce adds the segments of a step in a fixed order.  So av_vels, too, are bit-identical between the forms and
// between runs.
//
// With the option "force" the kernels also record the momentum-exchange force on the blocked cells (include/lbm.h, "Drag and
// lift"): dp_force_cell per blocked cell, its two components summed per segment in the same tree and per step by the same
// dp_reduce, so that record, too, is bit-identical between the forms.  Every step kernel has a `bool FORCE` template
// parameter; the false instances are the kernels without it, instruction for instruction.
#pragma once
#include "d2q9_kernels.h"

#include <cmath>
#include <type_traits>

namespace lbm {

constexpr int kDpSeg = 16;  // cells per row segment of the velocity sum

typedef double v2d __attribute__((ext_vector_type(2)));

// The second relaxation rate of the two-relaxation-time operator from omega and the magic parameter
// Lambda = (1/omega - 1/2)(1/omega_m - 1/2), on the host, in double: the three statements of include/lbm.h ("Two relaxation
// times"), contraction off.  The callers have refused magic <= 0 and omega >= 2.
inline double dp_trt_omega_minus(double omega, double magic) {
#pragma clang fp contract(off)
  const double tp = 1.0 / omega - 0.5;
  const double tm = magic / tp + 0.5;
  const double omega_m = 1.0 / tm;
  return omega_m;
}

// Subgrid viscosity (include/lbm.h, "Subgrid viscosity"): what an LES instance takes beyond omega and omega_m.  tau0 and les_k
// are the header's two host statements on the context's or member's omega and Smagorinsky constant; magic is read by the
// TRT instances alone, which recompute the second rate per cell.
struct DpLes {
  double tau0, les_k, magic;
};
inline DpLes dp_les_constants(double omega, double c, double magic) {
#pragma clang fp contract(off)
  const double tau0 = 1.0 / omega;
  const double les_k = (18.0 * std::sqrt(2.0)) * (c * c);
  return DpLes{tau0, les_k, magic};
}

// Body force (include/lbm.h, "Body force"): what a DRIVE instance takes beyond that, the constant force density of the context
// or member.  Everything else the statements need (the two halves, c_k . F, the odd source) a cell forms from these two.
struct DpDrive {
  double f_x, f_y;
};
inline bool dp_drive_on(double f_x, double f_y) { return !(f_x == 0.0 && f_y == 0.0); }
// dp_collide_cell asks for the two components where it uses them, twice per cell, through a callable: one that reads them from
// LDS holds no register in between.  This one returns a pair held in SGPRs; the DRIVE = false instances pass it empty.
struct DpDriveHeld {
  DpDrive f{};
  __device__ __forceinline__ DpDrive operator()() const { return f; }
};

// Collision of one cell in fp64.  TRT = false: BGK (kernels.cl:119-198), the statements of the fp64 oracle
// (oracle/d2q9_oracle.c, timestep_row) with pairwise momenta, contraction off: every kernel that inlines this rounds
// identically, and the cell equals the oracle's pairwise no-FMA build bit for bit; omega_m is not read.  TRT = true: the
// two-relaxation-time operator of include/lbm.h ("Two relaxation times") - moments, equilibrium and the obstacle branch are
// the same statements, only the relaxation lines differ: of each pair of opposite speeds the symmetric part of eq - g relaxes
// with omega, the antisymmetric part with omega_m.  Returns |u| = sqrt(j^2)/rho of a fluid cell, 0 for an obstacle.
// LES = true: the Smagorinsky rate of include/lbm.h ("Subgrid viscosity") in place of omega, and with TRT the second rate
// recomputed from it; the header's statements, from g and the moments alone, BEFORE the equilibrium and fenced: nothing of uvec
// or eq is alive under the two square roots and the divisions (placed behind the equilibrium, seven of the eight BGK ensemble
// instances spilled 8-36 B per lane).  omega and omega_m are not read.  LES = false: the kernel without it, `les` is not read.
// DRIVE = true: Guo forcing of include/lbm.h ("Body force") - the two momenta gain half the force before anything reads them, and
// the relaxation lines gain the source, its even part under 1 - omega / 2, its odd part, with TRT, under 1 - omega_m / 2.  The
// source is added in a pass of its own BEHIND the relaxation lines and fenced from them: there nothing of the equilibrium is
// alive, only out[], the two momenta, densinv and the rates, so the peak of the equilibrium loop is the DRIVE = false one plus
// nothing (formed inside that loop, as the header's order of statements suggests, all 32 ensemble instances spilled 40-68 B per
// lane).  drv() is called twice, before the shift and before the source.  DRIVE = false: the kernel without it, `drv` is not read.
template <bool TRT, bool LES = false, bool DRIVE = false, class Drv = DpDriveHeld>
__device__ __forceinline__ double dp_collide_cell(const double (&g)[9], bool obstacle, double omega, double omega_m,
                                                  [[maybe_unused]] const DpLes &les, [[maybe_unused]] const Drv &drv,
                                                  double (&out)[9]) {
#pragma clang fp contract(off)
  if (obstacle) {
    // bounce-back: the un-relaxed value leaves through the opposite speed (kernels.cl:69, 187-197)
    out[0] = g[0]; out[1] = g[3]; out[2] = g[4]; out[3] = g[1]; out[4] = g[2];
    out[5] = g[7]; out[6] = g[8]; out[7] = g[5]; out[8] = g[6];
    return 0.0;
  }
  const double ic_sq = 3.0;
  const double w0 = 4.0 / 9.0, w1 = 1.0 / 9.0, w2 = 1.0 / 36.0;
  double dens = g[0];
#pragma unroll
  for (int k = 1; k < 9; k++) dens += g[k];
  std::conditional_t<LES || DRIVE, double, const double> densinv = 1.0 / dens;
  const double diag_a = g[5] - g[7], diag_b = g[8] - g[6];
  std::conditional_t<LES || DRIVE, double, const double> u_x = (g[1] - g[3]) + (diag_a + diag_b);
  std::conditional_t<LES || DRIVE, double, const double> u_y = (g[2] - g[4]) + (diag_a - diag_b);
  if constexpr (DRIVE) {
    const DpDrive f = drv();
    u_x = u_x + 0.5 * f.f_x;
    u_y = u_y + 0.5 * f.f_y;
  }
  if constexpr (LES) {
    const double d57 = g[5] + g[7], d68 = g[6] + g[8], dgs = d57 + d68;
    const double p = dens * (1.0 / 3.0);
    const double pxx = ((g[1] + g[3]) + dgs) - (p + (u_x * u_x) * densinv);
    const double pyy = ((g[2] + g[4]) + dgs) - (p + (u_y * u_y) * densinv);
    const double pxy = (d57 - d68) - (u_x * u_y) * densinv;
    const double q = __builtin_sqrt((pxx * pxx + pyy * pyy) + 2.0 * (pxy * pxy));
    const double tau = 0.5 * (les.tau0 + __builtin_sqrt(les.tau0 * les.tau0 + les.les_k * (q * densinv)));
    omega = 1.0 / tau;
    if constexpr (TRT) {
      double tp = tau - 0.5;
      asm volatile("" : "+v"(omega), "+v"(tp));   // one division after the other
      const double tm = les.magic / tp + 0.5;
      omega_m = 1.0 / tm;
      asm volatile("" : "+v"(omega_m));
    }
    asm volatile("" : "+v"(omega), "+v"(dens), "+v"(u_x), "+v"(u_y), "+v"(densinv));
  }
  const double u_sq = u_x * u_x + u_y * u_y;
  double uvec[9];
  uvec[0] = 0.0;
  uvec[1] = u_x;        uvec[2] = u_y;
  uvec[3] = -u_x;       uvec[4] = -u_y;
  uvec[5] = u_x + u_y;  uvec[6] = -u_x + u_y;
  uvec[7] = -u_x - u_y; uvec[8] = u_x - u_y;
  const double half_densinv_icsq = 0.5 * densinv * ic_sq;
  double eq[9];
  eq[0] = w0 * (dens - half_densinv_icsq * u_sq);
#pragma unroll
  for (int k = 1; k < 9; k++) {
    const double t = uvec[k] * ic_sq;
    const double tsq = t * uvec[k];
    eq[k] = ((k < 5) ? w1 : w2) * (dens + t + half_densinv_icsq * (tsq - u_sq));
  }
  constexpr int pairs[4][2] = {{1, 3}, {2, 4}, {5, 7}, {6, 8}};
  if constexpr (TRT) {
    out[0] = g[0] + omega * (eq[0] - g[0]);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int k = pairs[i][0], q = pairs[i][1];
      const double a = eq[k] - g[k], b = eq[q] - g[q];
      const double sp = 0.5 * (a + b), sm = 0.5 * (a - b);
      const double rp = omega * sp, rm = omega_m * sm;
      out[k] = g[k] + (rp + rm);
      out[q] = g[q] + (rp - rm);
      // with both rates in VGPRs, one pair after the other: four in flight together do not fit 64 VGPRs
      if constexpr (LES) asm volatile("" : "+v"(out[k]), "+v"(out[q]), "+v"(dens));
    }
  } else {
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = g[k] + omega * (eq[k] - g[k]);
  }
  if constexpr (DRIVE) {
    // the source, behind the relaxation lines: se[k] is the same value on the two speeds of a pair and so[q] = -so[k], so a pair
    // forms them once; under BGK pe * (se[q] + so[q]) is pe * (se[k] - so[k]), the same bits
    asm volatile("" : "+v"(out[0]), "+v"(out[1]), "+v"(out[2]), "+v"(out[3]), "+v"(out[4]), "+v"(out[5]), "+v"(out[6]), "+v"(out[7]),
                 "+v"(out[8]));
    // |u| here: u_sq is not held across the source
    double speed = __builtin_sqrt(u_sq) * densinv;
    asm volatile("" : "+v"(u_x), "+v"(u_y), "+v"(densinv), "+v"(speed));
    const DpDrive f = drv();
    const double v_x = u_x * densinv, v_y = u_y * densinv;
    const double uF = v_x * f.f_x + v_y * f.f_y;
    const double t3 = 3.0 * uF;
    const double pe = 1.0 - 0.5 * omega;
    [[maybe_unused]] double po = 0.0;
    if constexpr (TRT) po = 1.0 - 0.5 * omega_m;
    out[0] = out[0] + pe * (w0 * (0.0 - t3));
    const double cF[9] = {0.0, f.f_x, f.f_y, -f.f_x, -f.f_y, f.f_x + f.f_y, -f.f_x + f.f_y, -f.f_x - f.f_y, f.f_x - f.f_y};
    // uvec[k] again, from the fenced momenta: the same bits, and nothing of uvec is held across the relaxation lines
    const double uv[9] = {0.0, u_x, u_y, -u_x, -u_y, u_x + u_y, -u_x + u_y, -u_x - u_y, u_x - u_y};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int k = pairs[i][0], q = pairs[i][1];
      const double cv = uv[k] * densinv;
      const double se = ((k < 5) ? w1 : w2) * (9.0 * (cv * cF[k]) - t3);
      const double so = ((k < 5) ? 1.0 / 3.0 : 1.0 / 12.0) * cF[k];   // 3 w_k
      if constexpr (TRT) {
        const double fe = pe * se, fo = po * so;
        out[k] = out[k] + (fe + fo);
        out[q] = out[q] + (fe - fo);
      } else {
        out[k] = out[k] + pe * (se + so);
        out[q] = out[q] + pe * (se - so);
      }
    }
    return speed;
  }
  return __builtin_sqrt(u_sq) * densinv;
}

// accelerate_flow on one cell (kernels.cl:24-42): fluid, and none of the three west-side densities would go negative
__device__ __forceinline__ void dp_accelerate_cell(double (&f)[9], bool obstacle, double aw1, double aw2) {
#pragma clang fp contract(off)
  if (!obstacle && (f[3] - aw1) > 0.0 && (f[6] - aw2) > 0.0 && (f[7] - aw2) > 0.0) {
    f[1] += aw1; f[5] += aw2; f[8] += aw2;
    f[3] -= aw1; f[6] -= aw2; f[7] -= aw2;
  }
}

// Open boundaries (include/lbm.h, "Open boundaries"): the Zou-He fix of a FLUID cell's gathered values, between gather and
// dp_collide_cell.  The inlet (column 0) replaces the three values that crossed the x wrap from column nx - 1 so that the
// cell carries the velocity (u, 0); the outlet (column nx - 1) replaces the three that came from column 0 so that it carries
// the density rho_out.  The header's statements, one IEEE operation per operator, contraction off.
__device__ __forceinline__ void dp_open_inlet(double (&g)[9], double u) {
#pragma clang fp contract(off)
  const double s0 = (g[0] + g[2]) + g[4];
  const double s1 = (g[3] + g[6]) + g[7];
  const double rho = (s0 + 2.0 * s1) / (1.0 - u);
  const double ru = rho * u;
  const double d = 0.5 * (g[2] - g[4]);
  g[1] = g[3] + (2.0 / 3.0) * ru;
  g[5] = (g[7] - d) + (1.0 / 6.0) * ru;
  g[8] = (g[6] + d) + (1.0 / 6.0) * ru;
}
__device__ __forceinline__ void dp_open_outlet(double (&g)[9], double rho_out) {
#pragma clang fp contract(off)
  const double s0 = (g[0] + g[2]) + g[4];
  const double s1 = (g[1] + g[5]) + g[8];
  const double ru = (s0 + 2.0 * s1) - rho_out;
  const double d = 0.5 * (g[2] - g[4]);
  g[3] = g[1] - (2.0 / 3.0) * ru;
  g[7] = (g[5] + d) - (1.0 / 6.0) * ru;
  g[6] = (g[8] - d) - (1.0 / 6.0) * ru;
}

// The LDS-tile kernels' mark of a fluid cell of column 0 / column nx - 1 in its lmask byte (OPEN instances only): the region
// load knows the grid column, the collision loop does not.  Blocked-ness is the low two bits there (body_map.h: 0, 1, 2).
constexpr uint8_t kOpenInlet = 4, kOpenOutlet = 8, kOpenBlocked = 3;

// Moving walls (include/lbm.h, "Moving walls"): a blocked cell with a wall velocity adds 6 w_k rho_wall c_k . u_wall to what it
// bounces back.  `out` holds the plain bounce-back of dp_collide_cell's obstacle branch (out[1] = g[3], ...), so each line is
// the header's statement: one IEEE operation per operator, contraction off.  A cell whose two components compare equal to 0.0
// is at rest and never comes here: no arithmetic touches it, signed zeros survive.
__device__ __forceinline__ bool dp_wall_moves(double u_x, double u_y) { return !(u_x == 0.0 && u_y == 0.0); }
__device__ __forceinline__ void dp_wall_cell(double (&out)[9], double u_x, double u_y, double rho_wall) {
#pragma clang fp contract(off)
  const double rx = rho_wall * u_x, ry = rho_wall * u_y;
  const double a = (2.0 / 3.0) * rx, b = (2.0 / 3.0) * ry;
  const double p = (1.0 / 6.0) * (rx + ry), q = (1.0 / 6.0) * (ry - rx);
  out[1] = out[1] + a; out[3] = out[3] - a;
  out[2] = out[2] + b; out[4] = out[4] - b;
  out[5] = out[5] + p; out[7] = out[7] - p;
  out[6] = out[6] + q; out[8] = out[8] - q;
}

// The LDS-tile kernels' mark of a blocked cell that moves, in a third spare bit of its lmask byte (WALL instances only): a pass
// behind the region load reads the cell's two velocities by its grid cell and marks it, a pass behind the collision loop
// finds the grid cell of a marked byte and reads them again under that branch - a moving cell is rare, and no LDS holds a
// velocity.
constexpr uint8_t kWallMoving = 16;

// The wall velocities of a context, [ny][nx] each, and its wall density: what a WALL instance takes beyond the arguments of
// the kernel without it.  The WALL = false instances keep the argument struct of a library without moving walls.
struct DpWall {
  const double *u_x, *u_y;
  double rho_wall;
};

// Momentum-exchange force on one blocked cell o in the step that streams the state f (include/lbm.h): for k = 1..8 in
// ascending order, if the neighbour x = o - c_k is fluid, s = f_k(x) + f_opp(k)(o) goes into F with the signs of c_k.
//   g[k]   = f_k(o - c_k), what o gathers in that step        own[k] = o's own stored f_k
//   nb[k]  = mask byte of o - c_k (non-zero: blocked, in the body or not; the link does not count)
// One addition per link term, contraction off; a cell without a counted link gives +0.0, +0.0.
__device__ __forceinline__ void dp_force_cell(const double (&g)[9], const double (&own)[9], const uint8_t (&nb)[9], double &fx,
                                              double &fy) {
#pragma clang fp contract(off)
  fx = 0.0;
  fy = 0.0;
  if (nb[1] == 0) { const double s = g[1] + own[3]; fx += s; }            // E
  if (nb[2] == 0) { const double s = g[2] + own[4]; fy += s; }            // N
  if (nb[3] == 0) { const double s = g[3] + own[1]; fx -= s; }            // W
  if (nb[4] == 0) { const double s = g[4] + own[2]; fy -= s; }            // S
  if (nb[5] == 0) { const double s = g[5] + own[7]; fx += s; fy += s; }   // NE
  if (nb[6] == 0) { const double s = g[6] + own[8]; fx -= s; fy += s; }   // NW
  if (nb[7] == 0) { const double s = g[7] + own[5]; fx -= s; fy -= s; }   // SW
  if (nb[8] == 0) { const double s = g[8] + own[6]; fx += s; fy -= s; }   // SE
}

// The segment tree over sixteen neighbouring lanes, one cell each (lane l of the segment holds cell l): pairs, then quads,
// then the two halves of each half, then the two halves - ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)) with p_i the sum of cells 2i,
// 2i+1 in every lane, because IEEE addition commutes.  DPP moves inside a row of sixteen lanes (quad_perm [1,0,3,2] and
// [2,3,0,1], row_half_mirror, row_mirror: after each stage the lanes that trade hold their group's one value, so a mirror
// serves as the exchange); all lanes of the wave active.
template <int CTRL>
__device__ __forceinline__ double dp_dpp_move(double v) {
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double dp_segment_tree16(double v) {
#pragma clang fp contract(off)
  v += dp_dpp_move<0xB1>(v);
  v += dp_dpp_move<0x4E>(v);
  v += dp_dpp_move<0x141>(v);
  v += dp_dpp_move<0x140>(v);
  return v;
}
// The same tree over the eight neighbouring lanes of a segment that hold two cells each (d2q9_dp_step's lanes): v is the
// lane's pair sum p_i, then xor 1, 2, 4 (IEEE addition commutes: every lane of the segment ends with the tree's bits)
__device__ __forceinline__ double dp_segment_tree8(double v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

// The sum of v over a workgroup of kBlock lanes in one fixed order, returned to lane 0 (0.0 elsewhere): the wave butterfly, then
// the four waves in order.  Every lane of the workgroup calls it (a barrier), once per kernel.
__device__ __forceinline__ double dp_block_sum(double v) {
  __shared__ double wsum[kBlock / 64];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    t = wsum[0];
    for (int i = 1; i < kBlock / 64; i++) t += wsum[i];
  }
  return t;
}

// Output stage, one fluid cell from its nine values: the columns of final_state.dat (d2q9-bgk.c:787-832, 396-442) in double,
// the oracle's statements (cell_moments), contraction off.  drv: NULL, or the body force of the grid (include/lbm.h, "Body
// force"): the reported velocity is the physical one.  f is a STORED state, the values behind a collision, whose momentum is the
// collided cell's plus the whole force: each momentum sum less half the force before the division.
__device__ __forceinline__ void dp_output_cell(const double (&f)[9], const double *drv, double &ux, double &uy, double &uu,
                                               double &pr) {
#pragma clang fp contract(off)
  double local_density = 0.0;
#pragma unroll
  for (int k = 0; k < 9; k++) local_density += f[k];
  double jx = f[1] + f[5] + f[8] - f[3] - f[6] - f[7];
  double jy = f[2] + f[5] + f[6] - f[4] - f[7] - f[8];
  if (drv) {
    jx = jx - 0.5 * drv[0];
    jy = jy - 0.5 * drv[1];
  }
  ux = jx / local_density;
  uy = jy / local_density;
  uu = __builtin_sqrt(ux * ux + uy * uy);
  pr = local_density * (1.0 / 3.0);
}

// Buoyancy (include/lbm.h, "Buoyancy"): the force density of one cell from its five STORED scalar values, the header's four
// statements, contraction off.  f0 is the body force of lbm_ddrive_set, (0.0, 0.0) while that is off.
struct DpBuoy {
  double b_x, b_y, c_ref;
  double f0_x, f0_y;
};
__device__ __forceinline__ DpDrive dp_buoy_force(const double (&g)[5], const DpBuoy &b) {
#pragma clang fp contract(off)
  const double c = (((g[0] + g[1]) + g[2]) + g[3]) + g[4];
  const double d = c - b.c_ref;
  return DpDrive{b.f0_x + b.b_x * d, b.f0_y + b.b_y * d};
}
// What a buoyant handle's kernels read per member, in device memory, by member index (a wave-uniform load): a context holds a
// table of one.  The scalar step and the output stage read `buoy` alone; the flow kernel (dp_buoyant_kernels.h) reads everything
// d2q9_dp_step takes as arguments.  Written by dp_host.h (buoy_table) from the handle's settings before a run and before the
// output stage.
struct DpBuoyMember {
  DpBuoy buoy;
  double omega, omega_m, aw1, aw2;   // as DpMember
  double rho_out, rho_wall;          // OPEN, WALL
  DpLes les;                         // LES
  const double *u_in;                // OPEN: the member's inlet profile, [ny]
  double pad;
};
static_assert(sizeof(DpBuoyMember) == 128, "a member's buoyant constants are two 64-B lines");

// Host side: the instance six run-time options choose.  f(force, trt, open, wall, les, drive) is called once, with the
// std::bool_constant of each option, so a launch site names its kernel's template flags as decltype(force)::value, ... and widens
// its argument struct where wall, les or drive is true.  Every launch site goes through here: the 64 instances of a kernel are
// these 64.
template <class F>
inline void dp_with_flags(bool force, bool trt, bool open, bool wall, bool les, bool drive, F &&f) {
  auto pick = [](bool on, auto &&g) { on ? g(std::true_type{}) : g(std::false_type{}); };
  pick(force, [&](auto fo) {
    pick(trt, [&](auto tr) {
      pick(open, [&](auto op) {
        pick(wall, [&](auto wa) { pick(les, [&](auto le) { pick(drive, [&](auto dr) { f(fo, tr, op, wa, le, dr); }); }); });
      });
    });
  });
}

// DRIVE: the two components behind whatever the instance without it takes; the DRIVE = false structs are those of a library
// without the option
template <class Base>
struct DpDriveArgs : Base {
  DpDrive drive;
};

struct DpStepArgs {
  const double *src;
  double *dst;
  const uint8_t *mask;       // [ny][nx]
  double *seg;               // [ny][nseg] segment sums of this step; FORCE: [3][ny][nseg], |u|, F_x, F_y
  unsigned long long plane_stride;
  int nx, ny;
  int lanes_per_row;         // ceil(nx / 2) rounded up to a multiple of 8: eight lanes = one 16-cell segment
  int accel_row;             // row that gets the NEXT step's accelerate_flow, or -1
  double omega, aw1, aw2;
  double omega_m;            // TRT: the second relaxation rate (dp_trt_omega_minus)
  const double *u_in;        // OPEN: the inlet profile, [ny]
  double rho_out;            // OPEN: the outlet density
};
struct DpStepWallArgs : DpStepArgs {
  DpWall wall;
};
// LES: the three constants behind whatever the instance without it takes; the LES = false structs are those of a library
// without the option
struct DpStepLesArgs : DpStepArgs {
  DpLes les;
};
struct DpStepWallLesArgs : DpStepWallArgs {
  DpLes les;
};
template <bool WALL, bool LES = false>
using DpStepPlainArgsOf = std::conditional_t<LES, std::conditional_t<WALL, DpStepWallLesArgs, DpStepLesArgs>,
                                             std::conditional_t<WALL, DpStepWallArgs, DpStepArgs>>;
template <bool WALL, bool LES = false, bool DRIVE = false>
using DpStepArgsOf = std::conditional_t<DRIVE, DpDriveArgs<DpStepPlainArgsOf<WALL, LES>>, DpStepPlainArgsOf<WALL, LES>>;

// One timestep, lane = cells x0, x0+1 of one row.  x-1 / x+1 neighbours: aligned 16-B loads plus one scalar load per
// streamed plane at the wrap column (an L1 hit).  A lane past the row's end (x0 >= nx) only joins the segment sum with 0.
// FORCE: a lane with a blocked cell also loads that cell's own streamed planes and its eight neighbours' mask bytes, under a
// branch, for dp_force_cell; fluid cells and lanes past the row's end count +0.0.
// TRT: dp_collide_cell<true>, nothing else; the false instances are the kernels without it, as with FORCE.
// OPEN: the fluid cell of column 0 (cell a of the lane x0 == 0) and of column nx - 1 (cell b where nx is even, cell a of the
// row's last lane where it is odd) go through dp_open_inlet / dp_open_outlet before the collision; the host passes accel_row
// -1.  The false instances are the kernels without it.
// WALL: a lane with a blocked cell loads that cell's two wall velocities under the branch it takes for the obstacle, and a
// cell that moves goes through dp_wall_cell after its bounce-back.  The false instances are the kernels without it.
// LES: dp_collide_cell<TRT, true> on a.les, nothing else.  The false instances are the kernels without it.
// DRIVE: dp_collide_cell<TRT, LES, true> on a.drive, nothing else.  The false instances are the kernels without it.
// static, like the helper kernels below: two translation units include this header (lbm_dp.cpp, lbm_dens.cpp).
template <bool FORCE, bool TRT, bool OPEN, bool WALL = false, bool LES = false, bool DRIVE = false>
static __global__ __launch_bounds__(kBlock) void d2q9_dp_step(const DpStepArgsOf<WALL, LES, DRIVE> a) {
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  const unsigned lpr = (unsigned)a.lanes_per_row;
  const int y = (int)(t / lpr);
  const int x0 = 2 * (int)(t - (unsigned)y * lpr);
  double tot = 0.0;
  double tfx = 0.0, tfy = 0.0;
  const bool live = y < a.ny && x0 < a.nx;
  if (live) {
    const bool has_b = x0 + 1 < a.nx;
    const size_t ps = a.plane_stride, rs = 9 * ps;
    const int ys = (y == 0) ? a.ny - 1 : y - 1, yn = (y + 1 == a.ny) ? 0 : y + 1;  // kernels.cl:91-93
    const int xw = (x0 == 0) ? a.nx - 1 : x0 - 1;                                  // kernels.cl:99-102
    const int xe = (x0 + 2 < a.nx) ? x0 + 2 : 0;  // east of cell x0+1, or of x0 when x0 is the row's last cell
    const double *rc = a.src + (size_t)y * rs, *rsth = a.src + (size_t)ys * rs, *rnth = a.src + (size_t)yn * rs;
    const v2d c0 = *reinterpret_cast<const v2d *>(rc + x0);
    const v2d c1 = *reinterpret_cast<const v2d *>(rc + ps + x0);
    const v2d c3 = *reinterpret_cast<const v2d *>(rc + 3 * ps + x0);
    const v2d c2 = *reinterpret_cast<const v2d *>(rsth + 2 * ps + x0);
    const v2d c5 = *reinterpret_cast<const v2d *>(rsth + 5 * ps + x0);
    const v2d c6 = *reinterpret_cast<const v2d *>(rsth + 6 * ps + x0);
    const v2d c4 = *reinterpret_cast<const v2d *>(rnth + 4 * ps + x0);
    const v2d c7 = *reinterpret_cast<const v2d *>(rnth + 7 * ps + x0);
    const v2d c8 = *reinterpret_cast<const v2d *>(rnth + 8 * ps + x0);
    const double w1 = rc[ps + xw], w5 = rsth[5 * ps + xw], w8 = rnth[8 * ps + xw];
    const double e3 = rc[3 * ps + xe], e6 = rsth[6 * ps + xe], e7 = rnth[7 * ps + xe];
    const uint8_t *m = a.mask + (size_t)y * a.nx + x0;
    const bool ob_a = m[0] != 0, ob_b = has_b && m[1] != 0;
    double ga[9] = {c0.x, w1, c2.x, has_b ? c3.y : e3, c4.x, w5, has_b ? c6.y : e6, has_b ? c7.y : e7, w8};
    double gb[9] = {c0.y, c1.x, c2.y, e3, c4.y, c5.x, e6, e7, c8.x};
    if constexpr (FORCE) {
      double fxa = 0.0, fya = 0.0, fxb = 0.0, fyb = 0.0;
      // cell x of this row: its own planes 1..8 and the masks of (x -+ 1, y -+ 1), periodic (kernels.cl:91-102)
      auto cell_force = [&](int x, const double (&g)[9], double &fx, double &fy) {
        const int xl = (x == 0) ? a.nx - 1 : x - 1, xr = (x + 1 == a.nx) ? 0 : x + 1;
        const uint8_t *mc = a.mask + (size_t)y * a.nx, *ms = a.mask + (size_t)ys * a.nx, *mn = a.mask + (size_t)yn * a.nx;
        double own[9];
        own[0] = 0.0;
#pragma unroll
        for (int k = 1; k < 9; k++) own[k] = rc[k * ps + x];
        const uint8_t nb[9] = {0, mc[xl], ms[x], mc[xr], mn[x], ms[xl], ms[xr], mn[xr], mn[xl]};
        dp_force_cell(g, own, nb, fx, fy);
      };
      // byte 1: blocked and counted; 2: blocked, outside the body (include/lbm.h, "Drag of a body")
      if (m[0] == 1) cell_force(x0, ga, fxa, fya);
      if (has_b && m[1] == 1) cell_force(x0 + 1, gb, fxb, fyb);
      tfx = has_b ? fxa + fxb : fxa + 0.0;
      tfy = has_b ? fya + fyb : fya + 0.0;
    }
    if constexpr (OPEN) {
      if (x0 == 0 && !ob_a) dp_open_inlet(ga, a.u_in[y]);
      if (has_b) {
        if (x0 + 2 == a.nx && !ob_b) dp_open_outlet(gb, a.rho_out);
      } else if (!ob_a) {
        dp_open_outlet(ga, a.rho_out);   // nx odd: the row's last lane holds column nx - 1 alone
      }
    }
    double oa[9], ob[9];
    DpLes les{};
    if constexpr (LES) les = a.les;
    DpDriveHeld drv{};
    if constexpr (DRIVE) drv.f = a.drive;
    const double ta = dp_collide_cell<TRT, LES, DRIVE>(ga, ob_a, a.omega, a.omega_m, les, drv, oa);
    const double tb = dp_collide_cell<TRT, LES, DRIVE>(gb, ob_b, a.omega, a.omega_m, les, drv, ob);
    if constexpr (WALL) {
      const size_t at = (size_t)y * a.nx + x0;   // ob_b implies has_b: at + 1 is a cell of this row
      if (ob_a) {
        const double u_x = a.wall.u_x[at], u_y = a.wall.u_y[at];
        if (dp_wall_moves(u_x, u_y)) dp_wall_cell(oa, u_x, u_y, a.wall.rho_wall);
      }
      if (ob_b) {
        const double u_x = a.wall.u_x[at + 1], u_y = a.wall.u_y[at + 1];
        if (dp_wall_moves(u_x, u_y)) dp_wall_cell(ob, u_x, u_y, a.wall.rho_wall);
      }
    }
    if (y == a.accel_row) {
      dp_accelerate_cell(oa, ob_a, a.aw1, a.aw2);
      dp_accelerate_cell(ob, ob_b, a.aw1, a.aw2);
    }
    double *d = a.dst + (size_t)y * rs + x0;
    if (has_b) {
#pragma unroll
      for (int k = 0; k < 9; k++) {
        v2d v = {oa[k], ob[k]};
        *reinterpret_cast<v2d *>(d + k * ps) = v;
      }
      tot = ta + tb;
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++) d[k * ps] = oa[k];
      tot = ta + 0.0;
    }
  }
  // the segment's tree across its eight lanes: the d2q9_dp_multi tree's bits
  tot = dp_segment_tree8(tot);
  if (y < a.ny && ((t - (unsigned)y * lpr) & 7u) == 0) a.seg[(size_t)y * (lpr >> 3) + ((t - (unsigned)y * lpr) >> 3)] = tot;
  if constexpr (FORCE) {
    tfx = dp_segment_tree8(tfx);
    tfy = dp_segment_tree8(tfy);
    if (y < a.ny && ((t - (unsigned)y * lpr) & 7u) == 0) {
      const size_t comp = (size_t)a.ny * (lpr >> 3);
      const size_t at = (size_t)y * (lpr >> 3) + ((t - (unsigned)y * lpr) >> 3);
      a.seg[comp + at] = tfx;
      a.seg[2 * comp + at] = tfy;
    }
  }
}

struct DpMultiArgs {
  const double *src;
  double *dst;
  const uint8_t *mask;
  double *seg;              // [T][ny][nseg]: the segment sums of each of the T steps; FORCE: [T][3][ny][nseg], |u|, F_x, F_y
  unsigned long long plane_stride, seg_step;   // seg_step = ny * nseg; FORCE: 3 ny nseg
  int nx, ny, nseg;
  int tiles_x;
  int T;                    // steps in this launch
  int accel_next;           // apply the following step's accelerate_flow to the final state
  double omega, aw1, aw2;
  double omega_m;           // TRT: the second relaxation rate (dp_trt_omega_minus)
  const double *u_in;       // OPEN: the inlet profile, [ny]
  double rho_out;           // OPEN: the outlet density
};
struct DpMultiWallArgs : DpMultiArgs {
  DpWall wall;
};
struct DpMultiLesArgs : DpMultiArgs {
  DpLes les;
};
struct DpMultiWallLesArgs : DpMultiWallArgs {
  DpLes les;
};
template <bool WALL, bool LES = false>
using DpMultiPlainArgsOf = std::conditional_t<LES, std::conditional_t<WALL, DpMultiWallLesArgs, DpMultiLesArgs>,
                                              std::conditional_t<WALL, DpMultiWallArgs, DpMultiArgs>>;
template <bool WALL, bool LES = false, bool DRIVE = false>
using DpMultiArgsOf = std::conditional_t<DRIVE, DpDriveArgs<DpMultiPlainArgsOf<WALL, LES>>, DpMultiPlainArgsOf<WALL, LES>>;

}  // namespace lbm
#include "dp_tile.h"   // dp_tile, on the per-cell functions above
namespace lbm {

// The one grid of a context as dp_tile takes it (dp_tile.h): the argument struct's own fields
template <bool WALL, bool LES = false, bool DRIVE = false>
struct DpMultiGrid {
  static constexpr bool kStageRhoOut = false;   // rho_out is a kernel argument, in SGPRs already; in LDS it cost two VGPRs
  static constexpr bool kStageLes = false;      // so are the subgrid constants, and this kernel has SGPRs to spare
  static constexpr bool kStageDrive = false;    // and the body force
  const DpMultiArgsOf<WALL, LES, DRIVE> &a;
  const double *src;
  double *dst;
  const uint8_t *mask;
  double *seg_out;
  double omega, omega_m, aw1, aw2;
  __device__ __forceinline__ explicit DpMultiGrid(const DpMultiArgsOf<WALL, LES, DRIVE> &a_)
      : a(a_), src(a_.src), dst(a_.dst), mask(a_.mask), seg_out(a_.seg), omega(a_.omega), omega_m(a_.omega_m),
        aw1(a_.aw1), aw2(a_.aw2) {}
  __device__ __forceinline__ unsigned comp() const { return (unsigned)(a.ny * a.nseg); }
  __device__ __forceinline__ const double *u_in() const { return a.u_in; }
  __device__ __forceinline__ double rho_out() const { return a.rho_out; }
  __device__ __forceinline__ size_t wall_cell0() const { return 0; }
  __device__ __forceinline__ const double *wall_u_x() const { return a.wall.u_x; }
  __device__ __forceinline__ const double *wall_u_y() const { return a.wall.u_y; }
  __device__ __forceinline__ double rho_wall() const { return a.wall.rho_wall; }
  __device__ __forceinline__ DpLes les() const { return a.les; }
  __device__ __forceinline__ DpDrive drive() const { return a.drive; }
};

// T <= TMAX timesteps per launch on one grid: dp_tile (dp_tile.h) with kMultiThreads threads, tile = blockIdx.x.
//
// Tile shape and depth, measured (tools/dp_throughput.py, one call, us/step at 128^2 / 256^2 / 512^2; profiles/dp_throughput.txt):
//   16x16, T <= 8 (149 KB of LDS, one workgroup per CU)  1.98 / 2.53 / 8.07   <- instantiated
//   16x8,  T <= 8 (113 KB)                               1.71 / 3.60 / 12.09  (wins only where every tile has a CU of its own)
//   16x16, T <= 4 (85 KB)                                2.13 / 2.99 / 8.43
// and one step per launch (d2q9_dp_step) 3.78 / 4.45 / 9.53, at 1024^2 23.8 against this kernel's 28.2: auto up to 300K cells.
// With every option on the tile holds about 152 of the 160 KB of LDS.
template <int TX, int TY, int TMAX, bool FORCE, bool TRT, bool OPEN, bool WALL = false, bool LES = false, bool DRIVE = false>
__global__ __launch_bounds__(kMultiThreads) void d2q9_dp_multi(const DpMultiArgsOf<WALL, LES, DRIVE> a) {
  dp_tile<TX, TY, TMAX, kMultiThreads, FORCE, TRT, OPEN, WALL, LES, DRIVE, DpMultiGrid<WALL, LES, DRIVE>>(a);
}

// What differs from member to member, in device memory, read by member index (a wave-uniform load), as EnsMember.  An
// ensemble holds a table of these (lbm_dens.cpp), a context a table of one (lbm_dp.cpp): the helper kernels below read a
// grid's constants here in both families.  Behind the table, in the same allocation, lie the four tables of the options'
// per-member constants (dens_*_table below), in both families too: a context's are an ensemble's of one member (dp_host.h
// writes them; the ensemble's step kernels and the output stage read them, a context's step kernels take theirs as arguments).
struct DpMember {
  double omega, aw1, aw2;  // aw1 = density*accel/9, aw2 = density*accel/36 (kernels.cl:14-15), in double
  double density;
  double w0, w1, w2;       // rest state (d2q9-bgk.c:529-531)
  union {
    double omega_m;        // the second relaxation rate of the TRT instances (dp_trt_omega_minus); omega where the member is BGK
    double pad;            // the name under which member_constants (host_common.h) zeroes the table's last slot
  };
};
static_assert(sizeof(DpMember) == 64, "a member's constants are one 64-B line");

// Open boundaries: member m's inlet profile u_in[ny] and, behind it, its rho_out lie m * (ny + 1) doubles into a second table,
// which starts where the table of DpMember ends: one allocation, and DensArgs is the struct of a library without it.
__host__ __device__ inline const double *dens_open_table(const DpMember *members, int n) {
  return reinterpret_cast<const double *>(members + n);
}
// Moving walls: member m's rho_wall is entry m of a third table, behind the open-boundary table
__host__ __device__ inline const double *dens_wall_table(const DpMember *members, int n, int ny) {
  return dens_open_table(members, n) + (size_t)n * (ny + 1);
}
// Subgrid viscosity: member m's DpLes (tau0, les_k, magic; dp_kernels.h) is entry m of a fourth table, behind the wall table
__host__ __device__ inline const DpLes *dens_les_table(const DpMember *members, int n, int ny) {
  return reinterpret_cast<const DpLes *>(dens_wall_table(members, n, ny) + n);
}

// Body force: member m's F_x, F_y are entry m of a fifth table, double[n][2], behind the subgrid table
__host__ __device__ inline const double *dens_drive_table(const DpMember *members, int n, int ny) {
  return reinterpret_cast<const double *>(dens_les_table(members, n, ny) + n);
}

// ---- the helper kernels: one set for both families --------------------------------------------------------------------
// Each has a member axis (blockIdx.y; blockIdx.z in dp_reduce): member m's grid lies m * member_stride into cells, its mask
// m * nx * ny into mask, its constants at members[m].  An ensemble launches them over its members, a context with one member
// (lbm_dp.cpp), so what a member and a context compute here is one kernel's work.  The block count along x fixes the order of
// every sum and is each launch site's own.

// ---- second reduction stage: fixed order, no atomics ---------------------------------------------------------------
// grid = (blocks, steps, members): block b of step r of member m adds in[r * in_stride + m * in_member + i] for i in its
// contiguous chunk (lane-strided, then the wave butterfly, then the four waves in order) into
// out[m * out_member + r * out_stride + b].  Run once into av_sum, or twice (partials per block, then one block per step and
// member) where a step has many segments (dp_host.h: reduce_steps).  active: NULL, or one word per member; a member whose word
// is 0 has stopped (dp_steady_kernels.h), its tiles wrote no segment sums and its record is left alone.
static __global__ __launch_bounds__(kBlock) void dp_reduce(const double *in, unsigned long long in_stride,
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

// accelerate_flow of row ny-2 of every member (kernels.cl:9-53): prologue of a run.  active: as dp_reduce
static __global__ void dp_accelerate_row(double *cells, unsigned long long plane_stride, unsigned long long member_stride,
                                         const uint8_t *mask, const DpMember *members, int nx, int ny, const int *active) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= nx || (active && active[blockIdx.y] == 0)) return;
  const DpMember mc = members[blockIdx.y];
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
static __global__ void dp_init_cells(double *cells, unsigned long long plane_stride, unsigned long long member_stride,
                                     const DpMember *members, int nx, size_t n) {
  const DpMember mc = members[blockIdx.y];
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
// for all members).  TO_DEVICE: flat -> cells, else cells -> flat.  par: NULL, or one word per member that says which
// of the two grid arrays holds that member's current state (0: cells, 1: cells_alt) once members have stopped on different
// launch parities (dp_steady_kernels.h).
template <bool TO_DEVICE>
static __global__ void dp_pack_planes(double *cells, double *cells_alt, const int *par, unsigned long long plane_stride,
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

// output stage per member: the columns of final_state.dat and the velocity sum (dp_output_cell: d2q9-bgk.c:787-832, 396-442, in
// double, the oracle's statements); obstacle cells give 0, 0, 0, density/3.  Outputs are double[members][ny][nx], partials
// double[members][gridDim.x]: the per-block sums of u.  cells_alt, par: as dp_pack_planes.  drive: NULL, or the members' body
// forces, double[members][2] (include/lbm.h, "Body force": the reported velocity is corrected by half of it).  buoy: NULL, or the
// members' buoyant constants, and scalar the current scalar array, member m 5 * plane_stride * ny doubles in (include/lbm.h,
// "Buoyancy": the half-force of each cell is that of its own five stored scalar values; drive is not read); scalar_alt: the
// scalar array of a member whose word par[m] is set (the scalar's two arrays in the order of the flow's)
static __global__ __launch_bounds__(kBlock) void dp_final_fields(const double *cells, const double *cells_alt, const int *par,
                                                                 unsigned long long plane_stride,
                                                                 unsigned long long member_stride, int nx, const uint8_t *mask,
                                                                 size_t n, const DpMember *members, const double *drive,
                                                                 const double *scalar, const double *scalar_alt,
                                                                 const DpBuoyMember *buoy,
                                                                 double *u_x, double *u_y, double *u, double *pressure,
                                                                 double *partials) {
#pragma clang fp contract(off)
  const double c_sq = 1.0 / 3.0;
  const double density = members[blockIdx.y].density;
  if (par && par[blockIdx.y]) cells = cells_alt;
  cells += (size_t)blockIdx.y * member_stride;
  mask += (size_t)blockIdx.y * n;
  const size_t off = (size_t)blockIdx.y * n;
  if (drive) drive += 2 * (size_t)blockIdx.y;
  DpBuoy bu{};
  if (buoy) {
    bu = buoy[blockIdx.y].buoy;
    if (par && par[blockIdx.y]) scalar = scalar_alt;
    scalar += (size_t)blockIdx.y * (5 * plane_stride * (n / nx));
  }
  double tot_u = 0.0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    double ux = 0.0, uy = 0.0, uu = 0.0, pr = density * c_sq;
    if (mask[i] == 0) {
      double f[9];
      const size_t y = i / nx;
      const size_t cell = y * 9 * plane_stride + (i - y * nx);
#pragma unroll
      for (int k = 0; k < 9; k++) f[k] = cells[k * plane_stride + cell];
      if (buoy) {
        const double *s = scalar + y * 5 * plane_stride + (i - y * nx);
        const double g[5] = {s[0], s[plane_stride], s[2 * plane_stride], s[3 * plane_stride], s[4 * plane_stride]};
        const DpDrive fo = dp_buoy_force(g, bu);
        const double pair[2] = {fo.f_x, fo.f_y};
        dp_output_cell(f, pair, ux, uy, uu, pr);
      } else {
        dp_output_cell(f, drive, ux, uy, uu, pr);
      }
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

// output stage: the force of the CURRENT state as the next step would stream it (include/lbm.h: lbm_dforce,
// lbm_dforce_ens).  grid = (blocks of d2q9_dp_step's lanes, members): member m's state lies m * member_stride into cells (or
// cells_alt where par[m] is set: dp_pack_planes), its mask m * nx * ny into mask, its segment sums m * ny * nseg into
// seg_x and seg_y, its aw1, aw2 are members[m]'s.  A blocked cell gathers from each fluid neighbour that neighbour's value after accelerate_flow: on row
// ny - 2 the neighbour's nine values go through dp_accelerate_cell in registers, the state is not written.  The per-cell
// function, the segment tree and, behind it, the reduction are the step kernels', so the value equals the record entry
// the next step writes, bit for bit.
struct DpForceArgs {
  const double *cells, *cells_alt;
  const int *par;
  const uint8_t *mask;
  double *seg_x, *seg_y;     // [members][ny][nseg]
  const DpMember *members;
  unsigned long long plane_stride, member_stride;
  int nx, ny;
  int lanes_per_row;         // as DpStepArgs
  int no_accel;              // open boundaries: the next step has no accelerate_flow, the neighbours' values go as stored
};

static __global__ __launch_bounds__(kBlock) void dp_force_state(const DpForceArgs a) {
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  const unsigned lpr = (unsigned)a.lanes_per_row;
  const int member = blockIdx.y;
  const int y = (int)(t / lpr);
  const int x0 = 2 * (int)(t - (unsigned)y * lpr);
  double tfx = 0.0, tfy = 0.0;
  if (y < a.ny && x0 < a.nx) {
    const bool has_b = x0 + 1 < a.nx;
    const size_t ps = a.plane_stride, rs = 9 * ps;
    const double *cells = ((a.par && a.par[member]) ? a.cells_alt : a.cells) + (size_t)member * a.member_stride;
    const uint8_t *mask = a.mask + (size_t)member * ((size_t)a.nx * a.ny);
    const double aw1 = a.members[member].aw1, aw2 = a.members[member].aw2;
    const int ys = (y == 0) ? a.ny - 1 : y - 1, yn = (y + 1 == a.ny) ? 0 : y + 1;  // kernels.cl:91-93
    auto cell_force = [&](int x, double &fx, double &fy) {
      const int xl = (x == 0) ? a.nx - 1 : x - 1, xr = (x + 1 == a.nx) ? 0 : x + 1;   // kernels.cl:99-102
      // the neighbour o - c_k of speed k (the cell o gathers f_k from)
      const int qx[9] = {x, xl, x, xr, x, xl, xr, xr, xl};
      const int qy[9] = {y, y, ys, y, yn, ys, ys, yn, yn};
      double g[9], own[9];
      uint8_t nb[9];
      const double *o = cells + (size_t)y * rs + x;
#pragma unroll
      for (int k = 0; k < 9; k++) own[k] = o[k * ps];
      g[0] = 0.0;
      nb[0] = 0;
#pragma unroll
      for (int k = 1; k < 9; k++) {
        nb[k] = mask[(size_t)qy[k] * a.nx + qx[k]];
        g[k] = 0.0;
        if (nb[k] == 0) {
          double f[9];
          const double *q = cells + (size_t)qy[k] * rs + qx[k];
#pragma unroll
          for (int j = 0; j < 9; j++) f[j] = q[j * ps];
          if (!a.no_accel && qy[k] == a.ny - 2) dp_accelerate_cell(f, false, aw1, aw2);
          g[k] = f[k];
        }
      }
      dp_force_cell(g, own, nb, fx, fy);
    };
    double fxa = 0.0, fya = 0.0, fxb = 0.0, fyb = 0.0;
    const uint8_t *m = mask + (size_t)y * a.nx + x0;
    if (m[0] == 1) cell_force(x0, fxa, fya);                  // 2: blocked, outside the body
    if (has_b && m[1] == 1) cell_force(x0 + 1, fxb, fyb);
    tfx = has_b ? fxa + fxb : fxa + 0.0;
    tfy = has_b ? fya + fyb : fya + 0.0;
  }
  // d2q9_dp_step's tree
  tfx = dp_segment_tree8(tfx);
  tfy = dp_segment_tree8(tfy);
  if (y < a.ny && ((t - (unsigned)y * lpr) & 7u) == 0) {
    const size_t at = (size_t)member * ((size_t)a.ny * (lpr >> 3)) + (size_t)y * (lpr >> 3) + ((t - (unsigned)y * lpr) >> 3);
    a.seg_x[at] = tfx;
    a.seg_y[at] = tfy;
  }
}

}  // namespace lbm

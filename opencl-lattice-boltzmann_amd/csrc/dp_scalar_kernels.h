// Passive scalar transport for the double-precision families (include/lbm.h, "Scalar transport"; lbm_dscalar_*): a D2Q5
// advection-diffusion lattice carried by the flow of a context or of each member of an ensemble, advanced by a kernel of its own.
// No flow kernel, argument struct or launch knows of the passive scalar: it reads the flow's state, the flow never reads it.  With
// buoyancy on (include/lbm.h, "Buoyancy") the flow step is a kernel of its own that does (dp_buoyant_kernels.h).
//
// Layout: five populations per cell in the flow's row-interleaved SoA - g_k(x, y) at y*5*plane_stride + k*plane_stride + x with the
// flow's plane_stride, two arrays, double-buffered, member m's grid mc.state_off doubles in.  Speeds 0..4 are the flow's 0..4
// (rest, E, N, W, S).
//
//   dp_scalar_step    one scalar step per launch, lane = 2 neighbouring cells of a row (d2q9_dp_step's lanes), member axis on
//                     blockIdx.y.  About 157 B per lattice update: 72 read from the flow, 40 + 40 of the scalar, the mask bytes.
//                     No LDS, no atomics.  <false>: the passive scalar.  <true>: a scalar that acts back (include/lbm.h,
//                     "Buoyancy"): the velocity it advects with is less half of each cell's own force; two more 16-B loads per lane
//                     (the cell's own g_2, g_4), about 173 B per update.
//   dp_scalar_init    g_k = w_k c0 on every cell
//   dp_scalar_field   output stage: the sum of a fluid cell's five stored values, 0.0 on a blocked cell
//   dp_scalar_pack    device layout <-> double[members][5][ny][nx] (dp_pack_planes with five planes)
//
// Every statement of the header is one IEEE operation per written operator, contraction off, so a member equals a context and
// both equal the numpy restatement (tests/_scalar_ref.py) bit for bit.
#pragma once
#include "dp_kernels.h"

namespace lbm {

// The relaxation rate of a scalar from its diffusivity, on the host, in double, contraction off (the header's statement).  The
// callers have refused D <= 0.
inline double dp_scalar_omega(double diffusivity) {
#pragma clang fp contract(off)
  const double tau = 3.0 * diffusivity + 0.5;
  return 1.0 / tau;
}

// What differs from member to member, in device memory, read by member index (a wave-uniform load): a context holds a table of
// one.  Offsets in elements of the array they index.
struct DpScalarMember {
  double omega_s;
  unsigned long long state_off;   // into the scalar arrays: m * 5 * plane_stride * ny
  unsigned long long flow_off;    // into the flow's grid array: m * member_stride
  unsigned long long cell_off;    // into mask and c_wall: m * nx * ny
  unsigned long long in_off;      // into c_in: m * ny
  const double *drive;            // NULL, or the member's body force F_x, F_y (dp_output_cell: the physical velocity)
  double pad[2];
};
static_assert(sizeof(DpScalarMember) == 64, "a member's scalar constants are one 64-B line");

struct DpScalarArgs {
  const double *flow;             // the state the flow's next step streams (after its accelerate_flow)
  const double *src;
  double *dst;
  const uint8_t *mask;            // [members][ny][nx], non-zero: blocked
  const double *c_wall;           // [members][ny][nx]: NaN insulating, finite held at that value; read at blocked cells only
  const double *c_in;             // [members][ny]: the inlet value of every row (open boundaries)
  const DpScalarMember *members;
  unsigned long long plane_stride;
  int nx, ny;
  int lanes_per_row;              // as DpStepArgs
  int open;                       // the flow has open boundaries: the inlet and outlet statements on columns 0 and nx - 1
};
// BUOY: the members' buoyant constants behind what the instance without it takes; the BUOY = false struct is that of a library
// without the option
struct DpScalarBuoyArgs : DpScalarArgs {
  const DpBuoyMember *buoy;
};
template <bool BUOY>
using DpScalarArgsOf = std::conditional_t<BUOY, DpScalarBuoyArgs, DpScalarArgs>;

// What a fluid cell gathers along speed k from a blocked neighbour q: its own opposite value comes back (insulating, half-way
// bounce-back), or the wall's value less it (a wall held at c_wall(q)).
__device__ __forceinline__ double dp_scalar_wall(double own_opp, double c_wall) {
#pragma clang fp contract(off)
  if (c_wall != c_wall) return own_opp;
  return (1.0 / 3.0) * c_wall - own_opp;
}

// Statements 4-6 of the header on the gathered values h and the cell's velocity: the relaxed values
__device__ __forceinline__ void dp_scalar_collide(const double (&h)[5], double u_x, double u_y, double omega_s, double (&out)[5]) {
#pragma clang fp contract(off)
  const double c = (((h[0] + h[1]) + h[2]) + h[3]) + h[4];
  const double a_x = 3.0 * (c * u_x);
  const double a_y = 3.0 * (c * u_y);
  double e[5];
  e[0] = (1.0 / 3.0) * c;
  e[1] = (1.0 / 6.0) * (c + a_x);
  e[3] = (1.0 / 6.0) * (c - a_x);
  e[2] = (1.0 / 6.0) * (c + a_y);
  e[4] = (1.0 / 6.0) * (c - a_y);
#pragma unroll
  for (int k = 0; k < 5; k++) out[k] = h[k] + omega_s * (e[k] - h[k]);
}

// One scalar step, lane = cells x0, x0+1 of one row.  16-B loads of the nine flow planes of the two cells and of g_0, g_2 (south
// row), g_4 (north row); the x-neighbours of g_1 and g_3 as d2q9_dp_step forms w1 and e3: the pair's other half plus one scalar
// load at the wrap or edge column.  A lane past the row's end is idle.  A cell's own g_2, g_4 and a neighbour's c_wall are read
// only under the branch of a blocked neighbour (or of a blocked cell, which copies its five values through).
// BUOY: the lane loads its two cells' own g_2 and g_4 always, forms each cell's force from its five stored values (dp_buoy_force on
// the member's b, c_ref and F0) and hands dp_output_cell that pair in place of the member's body force, which is not read.  The
// false instance is the kernel without it, instruction for instruction.
template <bool BUOY>
static __global__ __launch_bounds__(kBlock) void dp_scalar_step(const DpScalarArgsOf<BUOY> a) {
#pragma clang fp contract(off)
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  const unsigned lpr = (unsigned)a.lanes_per_row;
  const int y = (int)(t / lpr);
  const int x0 = 2 * (int)(t - (unsigned)y * lpr);
  if (y >= a.ny || x0 >= a.nx) return;
  const DpScalarMember mc = a.members[blockIdx.y];
  const bool has_b = x0 + 1 < a.nx;
  const size_t ps = a.plane_stride, frs = 9 * ps, grs = 5 * ps;
  const int ys = (y == 0) ? a.ny - 1 : y - 1, yn = (y + 1 == a.ny) ? 0 : y + 1;
  const int xw = (x0 == 0) ? a.nx - 1 : x0 - 1;
  const int xe = (x0 + 2 < a.nx) ? x0 + 2 : 0;  // east of cell x0+1, or of x0 when x0 is the row's last cell
  const double *fc = a.flow + mc.flow_off + (size_t)y * frs + x0;
  const double *gc = a.src + mc.state_off + (size_t)y * grs;
  const double *gs = a.src + mc.state_off + (size_t)ys * grs, *gn = a.src + mc.state_off + (size_t)yn * grs;
  v2d f[9];
#pragma unroll
  for (int k = 0; k < 9; k++) f[k] = *reinterpret_cast<const v2d *>(fc + k * ps);
  const v2d c0 = *reinterpret_cast<const v2d *>(gc + x0);
  const v2d c1 = *reinterpret_cast<const v2d *>(gc + ps + x0);
  const v2d c3 = *reinterpret_cast<const v2d *>(gc + 3 * ps + x0);
  const v2d c2 = *reinterpret_cast<const v2d *>(gs + 2 * ps + x0);
  const v2d c4 = *reinterpret_cast<const v2d *>(gn + 4 * ps + x0);
  const double w1 = gc[ps + xw], e3 = gc[3 * ps + xe];
  const uint8_t *mask = a.mask + mc.cell_off;
  const uint8_t *mrow = mask + (size_t)y * a.nx, *msth = mask + (size_t)ys * a.nx, *mnth = mask + (size_t)yn * a.nx;
  const double *cw = a.c_wall + mc.cell_off;
  const bool ob_a = mrow[x0] != 0, ob_b = has_b && mrow[x0 + 1] != 0;
  const bool blk_w = mrow[xw] != 0, blk_e = mrow[xe] != 0;

  // cell x of this row: own = its stored g_0, g_1, g_3; east / west: the streamed values and whether their cells are blocked
  auto cell = [&](int x, bool blocked, double own0, double own1, double own3, double from_w, bool w_blocked, int x_w, double from_e,
                  bool e_blocked, int x_e, double from_s, double from_n, const double (&fl)[9], const double *drv, double (&out)[5]) {
    if (blocked) {
      out[0] = own0; out[1] = own1; out[2] = gc[2 * ps + x]; out[3] = own3; out[4] = gc[4 * ps + x];
      return;
    }
    double h[5];
    h[0] = own0;
    h[1] = w_blocked ? dp_scalar_wall(own3, cw[(size_t)y * a.nx + x_w]) : from_w;
    h[3] = e_blocked ? dp_scalar_wall(own1, cw[(size_t)y * a.nx + x_e]) : from_e;
    h[2] = from_s;
    if (msth[x] != 0) h[2] = dp_scalar_wall(gc[4 * ps + x], cw[(size_t)ys * a.nx + x]);
    h[4] = from_n;
    if (mnth[x] != 0) h[4] = dp_scalar_wall(gc[2 * ps + x], cw[(size_t)yn * a.nx + x]);
    if (a.open) {
      if (x == 0) h[1] = a.c_in[mc.in_off + y] - (((h[0] + h[2]) + h[3]) + h[4]);
      if (x == a.nx - 1) h[3] = own3;
    }
    double u_x, u_y, uu, pr;
    dp_output_cell(fl, drv, u_x, u_y, uu, pr);
    dp_scalar_collide(h, u_x, u_y, mc.omega_s, out);
  };

  double fa[9], fb[9];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    fa[k] = f[k].x;
    fb[k] = f[k].y;
  }
  double oa[5], ob[5];
  // the force of each cell's own five stored values; without BUOY the member's body force, or NULL
  [[maybe_unused]] double pa[2], pb[2];
  const double *drv_a = mc.drive, *drv_b = mc.drive;
  if constexpr (BUOY) {
    const DpBuoy bu = a.buoy[blockIdx.y].buoy;
    const v2d o2 = *reinterpret_cast<const v2d *>(gc + 2 * ps + x0);
    const v2d o4 = *reinterpret_cast<const v2d *>(gc + 4 * ps + x0);
    const double sa[5] = {c0.x, c1.x, o2.x, c3.x, o4.x}, sb[5] = {c0.y, c1.y, o2.y, c3.y, o4.y};
    const DpDrive fa_ = dp_buoy_force(sa, bu), fb_ = dp_buoy_force(sb, bu);
    pa[0] = fa_.f_x, pa[1] = fa_.f_y;
    pb[0] = fb_.f_x, pb[1] = fb_.f_y;
    drv_a = pa, drv_b = pb;
  }
  // cell a: its west neighbour is column xw, its east neighbour cell b or, where the lane has none, column xe
  cell(x0, ob_a, c0.x, c1.x, c3.x, w1, blk_w, xw, has_b ? c3.y : e3, has_b ? ob_b : blk_e, has_b ? x0 + 1 : xe, c2.x, c4.x, fa, drv_a, oa);
  double *d = a.dst + mc.state_off + (size_t)y * grs + x0;
  if (has_b) {
    cell(x0 + 1, ob_b, c0.y, c1.y, c3.y, c1.x, ob_a, x0, e3, blk_e, xe, c2.y, c4.y, fb, drv_b, ob);
#pragma unroll
    for (int k = 0; k < 5; k++) {
      v2d v = {oa[k], ob[k]};
      *reinterpret_cast<v2d *>(d + k * ps) = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 5; k++) d[k * ps] = oa[k];
  }
}

// g_k = w_k c0 on every cell of every member: c0 = double[members][ny][nx]
static __global__ void dp_scalar_init(double *g, unsigned long long plane_stride, unsigned long long member_stride, int nx, size_t n,
                                      const double *c0) {
#pragma clang fp contract(off)
  g += (size_t)blockIdx.y * member_stride;
  c0 += (size_t)blockIdx.y * n;
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
    const size_t y = c / nx;
    const size_t i = y * 5 * plane_stride + (c - y * nx);
    const double v = c0[c];
    g[i] = (1.0 / 3.0) * v;
#pragma unroll
    for (int k = 1; k <= 4; k++) g[k * plane_stride + i] = (1.0 / 6.0) * v;
  }
}

// output stage per member: out = double[members][ny][nx]
static __global__ void dp_scalar_field(const double *g, unsigned long long plane_stride, unsigned long long member_stride, int nx,
                                       const uint8_t *mask, size_t n, double *out) {
#pragma clang fp contract(off)
  g += (size_t)blockIdx.y * member_stride;
  mask += (size_t)blockIdx.y * n;
  out += (size_t)blockIdx.y * n;
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
    double v = 0.0;
    if (mask[c] == 0) {
      const size_t y = c / nx;
      const double *p = g + y * 5 * plane_stride + (c - y * nx);
      v = (((p[0] + p[plane_stride]) + p[2 * plane_stride]) + p[3 * plane_stride]) + p[4 * plane_stride];
    }
    out[c] = v;
  }
}

// device layout <-> the caller's double[members][5][ny][nx].  TO_DEVICE: flat -> g, else g -> flat.
template <bool TO_DEVICE>
static __global__ void dp_scalar_pack(double *g, unsigned long long plane_stride, unsigned long long member_stride, int nx, size_t n,
                                      double *flat) {
  g += (size_t)blockIdx.y * member_stride;
  flat += (size_t)blockIdx.y * 5 * n;
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
    const size_t y = c / nx;
    const size_t i = y * 5 * plane_stride + (c - y * nx);
#pragma unroll
    for (int k = 0; k < 5; k++) {
      if (TO_DEVICE) g[k * plane_stride + i] = flat[k * n + c];
      else flat[k * n + c] = g[k * plane_stride + i];
    }
  }
}

}  // namespace lbm

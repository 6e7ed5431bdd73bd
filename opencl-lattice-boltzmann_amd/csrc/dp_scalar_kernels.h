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
//   dp_scalar_step_rec  the same lane body with the scalar's record (include/lbm.h, "Scalar record"): three segment sums a step,
//                     and the members' `active` words of a steady run
//   dp_scalar_gather  after a steady run that left the members on different arrays: every member onto one
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
  constexpr bool RECORD = false;
  [[maybe_unused]] double rec[3];
#include "dp_scalar_lane.inl"
}

// dp_scalar_step with the scalar's record: seg = [3][members][ny][nseg], the segment sums of c, c u_x and c u_y of this step, each
// the lane's pair sum through dp_segment_tree8 as d2q9_dp_buoyant forms the flow's (the lane body under the lane test, the trees
// and the stores of lane 0 of each segment outside it: every lane of a wave takes part in the shuffles).  active: NULL for an
// ordinary run, or the members' words during a leg of a steady run (dp_steady_kernels.h): the workgroups of a stopped member
// return before any load, uniformly.  No LDS, no atomics.
template <bool BUOY>
static __global__ __launch_bounds__(kBlock) void dp_scalar_step_rec(const DpScalarArgsOf<BUOY> a, double *seg, const int *active) {
#pragma clang fp contract(off)
  if (active && active[blockIdx.y] == 0) return;
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  const unsigned lpr = (unsigned)a.lanes_per_row;
  const int y = (int)(t / lpr);
  const unsigned lane = t - (unsigned)y * lpr;
  const int x0 = 2 * (int)lane;
  constexpr bool RECORD = true;
  double rec[3] = {0.0, 0.0, 0.0};
  if (y < a.ny && x0 < a.nx) {
#include "dp_scalar_lane.inl"
  }
  const unsigned nseg = lpr >> 3;
  const size_t per = (size_t)a.ny * nseg, comp = (size_t)gridDim.y * per;
  const size_t at = (size_t)blockIdx.y * per + (size_t)y * nseg + (lane >> 3);
#pragma unroll
  for (int v = 0; v < 3; v++) {
    const double s = dp_segment_tree8(rec[v]);
    if (y < a.ny && (lane & 7u) == 0) seg[(size_t)v * comp + at] = s;
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

// output stage per member: out = double[members][ny][nx].  g_alt, par: NULL, or the other scalar array and one word per member
// that says which of the two holds that member's state (0: g, 1: g_alt) once members have stopped on different launch parities
// (dp_pack_planes)
static __global__ void dp_scalar_field(const double *g, const double *g_alt, const int *par, unsigned long long plane_stride,
                                       unsigned long long member_stride, int nx, const uint8_t *mask, size_t n, double *out) {
#pragma clang fp contract(off)
  if (par && par[blockIdx.y]) g = g_alt;
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

// device layout <-> the caller's double[members][5][ny][nx].  TO_DEVICE: flat -> g, else g -> flat.  g_alt, par: as dp_scalar_field.
template <bool TO_DEVICE>
static __global__ void dp_scalar_pack(double *g, double *g_alt, const int *par, unsigned long long plane_stride,
                                      unsigned long long member_stride, int nx, size_t n, double *flat) {
  if (par && par[blockIdx.y]) g = g_alt;
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

// Every member whose word par[m] is set: its state from g_alt onto g (member_stride doubles, the padding between rows with it).
// The others' workgroups return at once.
static __global__ void dp_scalar_gather(double *g, const double *g_alt, const int *par, unsigned long long member_stride) {
  if (par[blockIdx.y] == 0) return;
  g += (size_t)blockIdx.y * member_stride;
  g_alt += (size_t)blockIdx.y * member_stride;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < member_stride; i += (size_t)gridDim.x * blockDim.x) g[i] = g_alt[i];
}

}  // namespace lbm

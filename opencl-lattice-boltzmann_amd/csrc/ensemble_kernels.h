// Device side of an ENSEMBLE (include/lbm.h: lbm_ens_*): N independent grids of one size, each with its own run
// constants, obstacle map and state, advanced by one launch per (up to) eight timesteps.
//
// A grid of a few hundred cells a side cannot fill 256 CUs (128x128 is 32 tiles of 32x16) and every launch of d2q9_multi
// on it is a launch latency plus one tile's latency chain.  d2q9_ensemble is that kernel with a member axis: member =
// blockIdx.y, tile = blockIdx.x; a member's grids and mask lie member_stride apart in the library's device layout
// (row-interleaved planes, d2q9_kernels.h), so a launch has N times the tiles and one launch latency.  The per-cell
// arithmetic is collide_cell / accelerate_cell, as in every other kernel: a member's state is bit-identical to the
// same grid advanced by single steps in a context of its own.  Members never interact: x and y wrap inside the member.
#pragma once
#include "d2q9_kernels.h"

namespace lbm {

// What differs from member to member, in device memory, read by member index (a wave-uniform load): keeping it out of
// the kernel arguments keeps them as lean as MultiArgs without its slab and peer fields (d2q9_kernels.h, MultiArgs:
// what SGPR-resident arguments cost this kernel family).
struct EnsMember {
  float omega, aw1, aw2;   // aw1 = density*accel/9, aw2 = density*accel/36 (kernels.cl:14-15)
  float density;
  float w0, w1, w2;        // rest state (d2q9-bgk.c:529-531)
  float pad;
};

struct EnsArgs {
  const float *src;         // member m: src + m * member_stride
  float *dst;
  const uint8_t *mask;      // member m: mask + m * nx * ny
  const EnsMember *members;
  float *partials;          // [T][members][tiles]: per-tile sums of |j|/rho for each of the T steps
  unsigned long long plane_stride, member_stride;   // row_stride = 9 * plane_stride
  int nx, ny;
  int tiles_x;
  int T;                    // steps in this launch
  int accel_next;           // apply the following step's accelerate_flow to the final state
};

// grid = (tiles per member, members).  TX x TY output tile, T <= kMultiMaxT steps LDS -> LDS on a region that shrinks by
// one cell per step (d2q9_multi's scheme; halo cells are computed redundantly by the member's neighbouring tiles).
// Instantiated for 16x16 (75 KB of LDS) and 16x8 (57 KB) tiles, 50 VGPRs: two workgroups share a CU, so one's loads and
// stores overlap the other's sub-steps (lbm_ensemble.cpp, build_ens: the measurements behind the choice).
// The tile body is a function of its own so that the gated kernel of a steady run (steady_kernels.h) advances a member with
// the very same instructions.
template <int TX, int TY>
__device__ __forceinline__ void ens_tile(const EnsArgs a) {
  constexpr int kRX = TX + 2 * kMultiMaxT, kRY = TY + 2 * kMultiMaxT;
  __shared__ float lds[2][9][kRY * kRX];
  __shared__ uint8_t lmask[kRY * kRX];
  __shared__ float wsum[kMultiMaxT][kMultiThreads / 64];
  const int tid = threadIdx.x;
  const int T = a.T;
  const int RX = TX + 2 * T, RY = TY + 2 * T;
  const int member = blockIdx.y;
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
  const int gx0 = tile_x * TX - T, gy0 = tile_y * TY - T;  // region cell (0,0)
  const size_t ps = a.plane_stride, rs = 9 * ps;
  const float *const src = a.src + (size_t)member * a.member_stride;
  float *const dst = a.dst + (size_t)member * a.member_stride;
  const uint8_t *const mask = a.mask + (size_t)member * ((size_t)a.nx * a.ny);
  const EnsMember mc = a.members[member];
  // grid row of region row ry: periodic wrap inside the member (kernels.cl:91-93)
  auto grid_row = [&](int ry) {
    int r = (gy0 + ry) % a.ny;
    return r < 0 ? r + a.ny : r;
  };

  // region -> LDS (periodic wrap in x, kernels.cl:99-102)
  {
    const float inv = 1.0f / (float)RX;
    for (int i = tid; i < RX * RY; i += kMultiThreads) {
      const int ry = (int)(((float)i + 0.5f) * inv), rx = i - ry * RX;
      int gx = (gx0 + rx) % a.nx;
      if (gx < 0) gx += a.nx;
      const int gy = grid_row(ry);
      const float *p = src + (size_t)gy * rs + gx;
#pragma unroll
      for (int k = 0; k < 9; k++) lds[0][k][ry * kRX + rx] = p[k * ps];
      lmask[ry * kRX + rx] = mask[(size_t)gy * a.nx + gx];
    }
  }
  __syncthreads();

  for (int s = 1; s <= T; s++) {
    const int in = (s - 1) & 1, out = s & 1;
    const int w = RX - 2 * s, h = RY - 2 * s;
    const float inv = 1.0f / (float)w;
    const bool accel_step = (s < T) || a.accel_next;
    float sum = 0.f;
    for (int i = tid; i < w * h; i += kMultiThreads) {
      const int q = (int)(((float)i + 0.5f) * inv);
      const int rx = s + (i - q * w), ry = s + q;
      const int c = ry * kRX + rx;
      float g[9], o[9];
      g[0] = lds[in][0][c];
      g[1] = lds[in][1][c - 1];
      g[2] = lds[in][2][c - kRX];
      g[3] = lds[in][3][c + 1];
      g[4] = lds[in][4][c + kRX];
      g[5] = lds[in][5][c - kRX - 1];
      g[6] = lds[in][6][c - kRX + 1];
      g[7] = lds[in][7][c + kRX + 1];
      g[8] = lds[in][8][c + kRX - 1];
      const bool obst = lmask[c] != 0;
      const float t = collide_cell(g, obst, mc.omega, o);
      if (accel_step && grid_row(ry) == a.ny - 2) accelerate_cell(o, obst, mc.aw1, mc.aw2);
#pragma unroll
      for (int k = 0; k < 9; k++) lds[out][k][c] = o[k];
      // only the tile's own cells count (and, for tiles hanging over the grid edge, only real cells)
      const int ox = rx - T, oy = ry - T;
      if (ox >= 0 && ox < TX && oy >= 0 && oy < TY && tile_x * TX + ox < a.nx && tile_y * TY + oy < a.ny) sum += t;
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) wsum[s - 1][tid >> 6] = sum;
    __syncthreads();
  }

  // central tile -> global
  {
    const int fin = T & 1;
    for (int i = tid; i < TX * TY; i += kMultiThreads) {
      const int oy = i / TX, ox = i - oy * TX;
      const int gx = tile_x * TX + ox, gy = tile_y * TY + oy;
      if (gx < a.nx && gy < a.ny) {
        const int c = (oy + T) * kRX + ox + T;
        float *d = dst + (size_t)gy * rs + gx;
#pragma unroll
        for (int k = 0; k < 9; k++) d[k * ps] = lds[fin][k][c];
      }
    }
  }
  if (tid < T) {
    float t = wsum[tid][0];
    for (int i = 1; i < kMultiThreads / 64; i++) t += wsum[tid][i];
    a.partials[((size_t)tid * gridDim.y + member) * gridDim.x + blockIdx.x] = t;
  }
}

template <int TX, int TY>
__global__ __launch_bounds__(kMultiThreads) void d2q9_ensemble(const EnsArgs a) {
  ens_tile<TX, TY>(a);
}

// ---- second reduction stage, batched: one workgroup per (buffered step, member) -------------------
// partials = [steps][members][tiles]; sums a member's tiles of one step in a fixed order (fp64) into
// av_sum[member * record + first + step].  grid = (members, steps).  active: NULL, or one word per member; a member whose
// word is 0 has stopped (steady_kernels.h), its tiles wrote no partial sums and its record is left alone.
static __global__ __launch_bounds__(kBlock) void ens_reduce_partials(const float *partials, int tiles, double *av_sum,
                                                                     unsigned long long record, int first, const int *active) {
  if (active && active[blockIdx.x] == 0) return;
  const float *p = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * tiles;
  double acc = 0.0;
  for (int i = threadIdx.x; i < tiles; i += kBlock) acc += (double)p[i];
  __shared__ double wsum[kBlock / 64];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wsum[0];
    for (int i = 1; i < kBlock / 64; i++) t += wsum[i];
    av_sum[(size_t)blockIdx.x * record + first + blockIdx.y] = t;
  }
}

// ---- the helper kernels of d2q9_kernels.h with a member axis (blockIdx.y), same per-cell arithmetic ----------------

// accelerate_flow of row ny-2 of every member (kernels.cl:9-53): prologue of a run.  active: as ens_reduce_partials
static __global__ void ens_accelerate_row(float *cells, unsigned long long plane_stride, unsigned long long member_stride,
                                          const uint8_t *mask, const EnsMember *members, int nx, int ny, const int *active) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= nx || (active && active[blockIdx.y] == 0)) return;
  const EnsMember mc = members[blockIdx.y];
  cells += (size_t)blockIdx.y * member_stride;
  mask += (size_t)blockIdx.y * ((size_t)nx * ny);
  const int row = ny - 2;
  const size_t c = (size_t)row * 9 * plane_stride + x;
  float f3 = cells[3 * plane_stride + c], f6 = cells[6 * plane_stride + c], f7 = cells[7 * plane_stride + c];
  if (mask[(size_t)row * nx + x] == 0 && (f3 - mc.aw1) > 0.0f && (f6 - mc.aw2) > 0.0f && (f7 - mc.aw2) > 0.0f) {
    cells[1 * plane_stride + c] += mc.aw1;
    cells[5 * plane_stride + c] += mc.aw2;
    cells[8 * plane_stride + c] += mc.aw2;
    cells[3 * plane_stride + c] = f3 - mc.aw1;
    cells[6 * plane_stride + c] = f6 - mc.aw2;
    cells[7 * plane_stride + c] = f7 - mc.aw2;
  }
}

// every member's rest state from its own density (values of d2q9-bgk.c:529-550, computed on the host)
static __global__ void ens_init_cells(float *cells, unsigned long long plane_stride, unsigned long long member_stride,
                                      const EnsMember *members, int nx, size_t n) {
  const EnsMember mc = members[blockIdx.y];
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

// device layout <-> the caller's float[members][9][ny][nx] (staged in the grid that is not current, one transfer for
// the whole ensemble).  TO_DEVICE: flat -> cells, else cells -> flat.  par: NULL, or one word per member that says which
// of the two grid arrays holds that member's current state (0: cells, 1: cells_alt) once members have stopped on different
// launch parities (steady_kernels.h).
template <bool TO_DEVICE>
static __global__ void ens_pack_planes(float *cells, float *cells_alt, const int *par, unsigned long long plane_stride,
                                       unsigned long long member_stride, int nx, size_t n, float *flat) {
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

// output stage per member (final_fields of d2q9_kernels.h: d2q9-bgk.c:787-832, 396-442): outputs are
// float[members][ny][nx], partials float[members][gridDim.x].  cells_alt, par: as ens_pack_planes
static __global__ __launch_bounds__(kBlock) void ens_final_fields(const float *cells, const float *cells_alt, const int *par,
                                                                  unsigned long long plane_stride,
                                                                  unsigned long long member_stride, int nx, const uint8_t *mask,
                                                                  size_t n, const EnsMember *members, float *u_x, float *u_y,
                                                                  float *u, float *pressure, float *partials) {
  const float c_sq = 1.0f / 3.0f;
  const float density = members[blockIdx.y].density;
  if (par && par[blockIdx.y]) cells = cells_alt;
  cells += (size_t)blockIdx.y * member_stride;
  mask += (size_t)blockIdx.y * n;
  const size_t off = (size_t)blockIdx.y * n;
  float tot_u = 0.0f;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    float ux = 0.0f, uy = 0.0f, uu = 0.0f, pr = density * c_sq;
    if (mask[i] == 0) {
      float f[9];
      float local_density = 0.0f;
      const size_t y = i / nx;
      const size_t cell = y * 9 * plane_stride + (i - y * nx);
#pragma unroll
      for (int k = 0; k < 9; k++) {
        f[k] = cells[k * plane_stride + cell];
        local_density += f[k];
      }
      ux = (f[1] + f[5] + f[8] - f[3] - f[6] - f[7]) / local_density;
      uy = (f[2] + f[5] + f[6] - f[4] - f[7] - f[8]) / local_density;
      uu = sqrtf(ux * ux + uy * uy);
      pr = local_density * c_sq;
      tot_u += uu;
    }
    if (u_x) u_x[off + i] = ux;
    if (u_y) u_y[off + i] = uy;
    if (u) u[off + i] = uu;
    if (pressure) pressure[off + i] = pr;
  }
  block_store_partial(tot_u, partials + (size_t)blockIdx.y * gridDim.x);
}

}  // namespace lbm

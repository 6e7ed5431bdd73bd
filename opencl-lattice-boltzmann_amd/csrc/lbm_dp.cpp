// Fourth translation unit of liblbm_hip.so: the host side of the double-precision contexts (include/lbm.h: lbm_dp_*).
//
// A double-precision context is one grid on the current device in fp64: two grid arrays in the row-interleaved layout of
// dp_kernels.h, a byte mask, a ring of per-step segment sums and the av_vels record.  The step loop is that of an
// ordinary single-slab context: a prologue accelerate_flow, then launches of d2q9_dp_step (one step each) or of
// d2q9_dp_multi (up to eight steps each, option "multistep"), each with the next step's acceleration fused into its write
// of row ny-2, and the second reduction stage over the buffered steps.  The reference's counterpart is its one grid and
// in-order queue (d2q9-bgk.c:221-239), in the precision of its fp64 ancestor.
#include "../../include/lbm.h"
#include "dp_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace lbm;
using namespace lbm_host;

// The LDS-tile form's tile height and most steps per launch (16 x 16 at T <= 8 unless a measurement build asks for
// another shape: tools/dp_throughput.py, DESIGN.md "Double precision")
#ifndef LBM_DP_TY
#define LBM_DP_TY 16
#endif
#ifndef LBM_DP_TMAX
#define LBM_DP_TMAX 8
#endif

namespace {

constexpr int kDpTX = 16, kDpTY = LBM_DP_TY, kDpTMax = LBM_DP_TMAX;
constexpr long kDpAutoMultiCells = 300L * 1024;  // the library's bound for "launch-bound" (multistep_effective, lbm_hip.cpp)
constexpr long kDpSegsPerBlock = 4096;           // segments per block of the first reduction stage

}  // namespace

struct lbm_dp {
  lbm_dparams p{};
  Queue q;
  size_t plane_stride = 0;        // doubles
  double *cells[2] = {nullptr, nullptr};
  uint8_t *mask = nullptr;        // [ny][nx]: 0 fluid, 1 blocked and counted in the force, 2 blocked outside the body
  BodyMap body;                   // the host's copy of what the mask was made of (body_map.h)
  DpMember *members = nullptr;    // [1]: this grid's constants as the helper kernels read them (dp_kernels.h), and behind it the
                                  // option tables of an ensemble of one member (dens_*_table; dp_host.h writes them).  The step
                                  // kernels take their constants as arguments, from flow's host copies; of the tables they read
                                  // the inlet profile (dens_open_table), and dp_final_fields the body force (dens_drive_table)
  double *seg = nullptr;          // [ring][ny][nseg]
  double *red = nullptr;          // [ring][red_blocks]: first reduction stage
  double *av_sum = nullptr;       // [max_iters]
  double *fin_partials = nullptr; // [fin_blocks]
  double *force_rec = nullptr;    // option "force": [2][max_iters], F_x then F_y per step
  double *force_now = nullptr;    // [2]: lbm_dforce's F_x, F_y (allocated by the first call)
  int lanes_per_row = 8, nseg = 1, red_blocks = 1, fin_blocks = 1;
  int tiles_x = 1, tiles = 1;
  int ring = 8, ring_fill = 0;
  int multistep = -1;             // option "multistep": -1 auto, 0 one step per launch, 1..8
  FlowState flow;                 // "force", lbm_dtrt_set, lbm_dopen_set, lbm_dwall_set, lbm_dles_set, lbm_ddrive_set: the settings
                                  // of one member (dp_host.h), all off by default; a setter's 0 is that header's NULL array
  ScalarState scalar;             // lbm_dscalar_set: the scalar (dp_host.h), off by default
  BuoyState buoy;                 // lbm_dbuoy_set: the scalar acts back on the flow (dp_host.h), off by default
  StatsState stats;               // lbm_dstats_set: the running statistics (dp_host.h), off by default
  int cur = 0, steps_done = 0;
  bool failed = false;
};

namespace {

int multistep_effective(const lbm_dp *d) {
  if (d->multistep >= 0) return std::min(d->multistep, kDpTMax);
  // auto: the LDS-tile form where a grid is launch-bound (profiles/dp_throughput.txt: it beats one step per launch there)
  return (long)d->p.nx * d->p.ny <= kDpAutoMultiCells ? kDpTMax : 0;
}

void free_dp(lbm_dp *d) {
  queue_drain(d->q);
  for (double *c : d->cells)
    if (c) (void)hipFree(c);
  if (d->mask) (void)hipFree(d->mask);
  if (d->members) (void)hipFree(d->members);
  if (d->seg) (void)hipFree(d->seg);
  if (d->red) (void)hipFree(d->red);
  if (d->av_sum) (void)hipFree(d->av_sum);
  if (d->fin_partials) (void)hipFree(d->fin_partials);
  if (d->force_rec) (void)hipFree(d->force_rec);
  if (d->force_now) (void)hipFree(d->force_now);
  if (d->flow.wall_dev) (void)hipFree(d->flow.wall_dev);
  scalar_free(d->scalar);
  buoy_free(d->buoy);
  stats_free(d->stats);
  queue_destroy(d->q);
  delete d;
}

// the grid and its ring as the setters take them (dp_host.h): a context is one member
FlowGrid flow_grid(lbm_dp *d) {
  return FlowGrid{1, &d->p, d->members, d->q, d->steps_done, d->seg, d->red, d->ring, (size_t)d->p.ny * d->nseg, d->red_blocks, kMultiMaxT};
}

int build_dp(lbm_dp *d, const int32_t *obstacles) {
  const int nx = d->p.nx, ny = d->p.ny;
  const size_t cells = (size_t)nx * ny;
  HIP_TRY(hipGetDevice(&d->q.dev));
  d->plane_stride = ((size_t)(nx + 31) / 32) * 32;   // 256-B lines, >= nx + 1 for odd nx: a lane's second cell stays inside
  d->lanes_per_row = (int)(div_up(div_up(nx, 2), 8) * 8);
  d->nseg = d->lanes_per_row / 8;                    // = ceil(nx / 16)
  d->tiles_x = (int)div_up(nx, kDpTX);
  d->tiles = d->tiles_x * (int)div_up(ny, kDpTY);
  const size_t per_step = (size_t)ny * d->nseg;
  d->red_blocks = (int)std::min(512L, div_up((long)per_step, kDpSegsPerBlock));
  d->ring = ring_steps_of(1, per_step, 1, kMultiMaxT);
  d->fin_blocks = (int)std::max(1L, std::min(div_up((long)cells, kBlock), 2048L));
  if ((long)d->lanes_per_row * ny > 0x7fffffffL)
    return lbm_fail(LBM_ERR_ARG, "a grid of %dx%d cells is beyond the 2^31 lanes of one launch", nx, ny);

  const size_t grid_bytes = (9 * d->plane_stride * ny + 32) * sizeof(double);
  const size_t need = 2 * grid_bytes + cells + 64 + flow_table_bytes(1, ny) + (size_t)d->ring * per_step * sizeof(double) +
                      (size_t)d->ring * d->red_blocks * sizeof(double) + (size_t)d->p.max_iters * sizeof(double) +
                      (size_t)d->fin_blocks * sizeof(double);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b)
    return lbm_fail(LBM_ERR_HIP, "a double-precision grid of %dx%d with max_iters=%d needs %.1f MiB of device memory, %.1f MiB are free",
                    nx, ny, d->p.max_iters, (double)need / 1048576.0, (double)free_b / 1048576.0);

  if (int rc = queue_create(d->q)) return rc;
  for (int i = 0; i < 2; i++) {
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d->cells[i]), grid_bytes));
    HIP_TRY(hipMemset(d->cells[i], 0, grid_bytes));
  }
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d->mask), cells + 64));
  if (int rc = alloc_ring(flow_grid(d), 1)) return rc;
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d->av_sum), (size_t)d->p.max_iters * sizeof(double)));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d->fin_partials), (size_t)d->fin_blocks * sizeof(double)));
  // the tables of one member: aw1, aw2 are run_dp_impl's statements, and the rest state's w0..w2 come from here alone
  if (int rc = flow_create(d->flow, &d->members, &d->p, 1)) return rc;
  body_reset(d->body, obstacles, cells);
  return upload_mask(d->mask, obstacles, cells);
}

// The instance the options choose: FORCE from "force", TRT from lbm_dtrt_set, OPEN from lbm_dopen_set, WALL from lbm_dwall_set,
// LES from lbm_dles_set, DRIVE from lbm_ddrive_set.
// With all off these are the launches of a library without any of them.
// what a WALL instance takes beyond the arguments of the kernel without it
DpWall wall_args(const lbm_dp *d) {
  const size_t n = (size_t)d->p.nx * d->p.ny;
  return DpWall{d->flow.wall_dev, d->flow.wall_dev + n, d->flow.rho_wall[0]};
}

// what an LES instance takes beyond them: the header's two host statements, and the magic parameter as set (either order)
DpLes les_args(const lbm_dp *d) { return les_constants(d->flow, &d->p, 0); }

// what a DRIVE instance takes beyond them, and where dp_final_fields and the scalar read the same pair (NULL while it is off)
DpDrive drive_args(const lbm_dp *d) { return DpDrive{d->flow.drive_f[0], d->flow.drive_f[1]}; }
const double *drive_dev(const lbm_dp *d) { return d->flow.drive ? dens_drive_table(d->members, 1, d->p.ny) : nullptr; }

// the grid as the scalar's helpers take it (dp_host.h): a context is one member
ScalarGrid scalar_grid(const lbm_dp *d) { return ScalarGrid{1, d->p.nx, d->p.ny, d->plane_stride, 0, d->red_blocks, d->p.max_iters}; }

void launch_multi(const lbm_dp *d, const DpMultiArgs &a) {
  const FlowState &f = d->flow;
  dp_with_flags(f.force, f.trt, f.open, f.wall, f.les, f.drive, [&](auto force, auto trt, auto open, auto wall, auto les, auto drive) {
    constexpr bool FORCE = decltype(force)::value, TRT = decltype(trt)::value, OPEN = decltype(open)::value, WALL = decltype(wall)::value,
                   LES = decltype(les)::value, DRIVE = decltype(drive)::value;
    DpMultiArgsOf<WALL, LES, DRIVE> w{};
    static_cast<DpMultiArgs &>(w) = a;
    if constexpr (WALL) w.wall = wall_args(d);
    if constexpr (LES) w.les = les_args(d);
    if constexpr (DRIVE) w.drive = drive_args(d);
    hipLaunchKernelGGL((d2q9_dp_multi<kDpTX, kDpTY, kDpTMax, FORCE, TRT, OPEN, WALL, LES, DRIVE>), dim3(d->tiles), dim3(kMultiThreads), 0,
                       d->q.st, w);
  });
}

void launch_step(const lbm_dp *d, const DpStepArgs &a) {
  const dim3 grid((unsigned)div_up((long)d->lanes_per_row * d->p.ny, kBlock));
  const FlowState &f = d->flow;
  dp_with_flags(f.force, f.trt, f.open, f.wall, f.les, f.drive, [&](auto force, auto trt, auto open, auto wall, auto les, auto drive) {
    constexpr bool FORCE = decltype(force)::value, TRT = decltype(trt)::value, OPEN = decltype(open)::value, WALL = decltype(wall)::value,
                   LES = decltype(les)::value, DRIVE = decltype(drive)::value;
    DpStepArgsOf<WALL, LES, DRIVE> w{};
    static_cast<DpStepArgs &>(w) = a;
    if constexpr (WALL) w.wall = wall_args(d);
    if constexpr (LES) w.les = les_args(d);
    if constexpr (DRIVE) w.drive = drive_args(d);
    hipLaunchKernelGGL((d2q9_dp_step<FORCE, TRT, OPEN, WALL, LES, DRIVE>), grid, dim3(kBlock), 0, d->q.st, w);
  });
}

int run_dp_impl(lbm_dp *d, int nsteps, bool timed, double *ms, bool *launched) {
  if (int rc = check_runnable(nsteps, d->failed, "context")) return rc;
  if (int rc = check_record(d->p.max_iters, d->steps_done, nsteps, "")) return rc;
  if (timed && ms) *ms = 0.0;
  if (nsteps == 0) return LBM_OK;
  HIP_TRY(hipSetDevice(d->q.dev));
  *launched = true;
  const int nx = d->p.nx, ny = d->p.ny;
  const double aw1 = d->p.density * d->p.accel / 9.0;   // kernels.cl:14-15
  const double aw2 = d->p.density * d->p.accel / 36.0;
  // the member's settings as the step kernels take them: element 0 of the host copies, and the profile in the table of one
  const double omega_m = d->flow.omega_m[0], rho_out = d->flow.open_host[ny];
  const double *u_in = dens_open_table(d->members, 1);
  const size_t per_step = (size_t)ny * d->nseg;
  const int nval = seg_values(d->flow);
  const size_t slot = per_step * nval;   // one step in the ring: [nval][ny][nseg]
  const int T = multistep_effective(d);
  // with a scalar on every launch advances one step, in the kernel form "multistep" chooses: the scalar reads each step's velocities
  const bool scalar = d->scalar.on;
  const ScalarGrid sgrid = scalar_grid(d);
  if (scalar)
    if (int rc = scalar_begin_run(d->scalar, sgrid, drive_dev(d))) return rc;
  // with buoyancy on there is one kernel form, d2q9_dp_buoyant: "multistep" chooses nothing
  const bool buoy = scalar && d->buoy.on;
  if (buoy)
    if (int rc = buoy_sync(d->buoy, d->flow, flow_grid(d))) return rc;
  // running statistics: the run is cut at its sample points (stats_plan.h); off, it is one piece
  std::vector<StatsPiece> pieces;
  if (!stats_plan(d->steps_done, nsteps, d->stats.origin, d->stats.every, pieces)) return stats_refuse_plan(d->steps_done, d->stats.origin);
  if (int rc = timed_begin(d->q, timed)) return rc;

  int batch_first = d->steps_done;
  // second reduction stage over the buffered steps
  auto flush = [&]() -> int {
    if (d->ring_fill == 0) return LBM_OK;
    // |u| into av_sum and, with "force", F_x and F_y into their records: the same launches on each value's segments
    for (int v = 0; v < nval; v++) {
      double *record = (v == 0 ? d->av_sum : d->force_rec + (size_t)(v - 1) * d->p.max_iters) + batch_first;
      if (int rc = reduce_steps(d->q.st, d->seg + (size_t)v * per_step, slot, per_step, d->ring_fill, 1, d->red, d->red_blocks, record,
                                0ull, nullptr))
        return rc;
    }
    // the scalar's record: the same steps of its own ring
    if (int rc = scalar_flush(d->scalar, sgrid, d->q.st, d->ring_fill, batch_first, nullptr)) return rc;
    batch_first += d->ring_fill;
    d->ring_fill = 0;
    return LBM_OK;
  };
  // every piece as a run of its length is enqueued; the ring of segment sums and its flushes carry across the cuts
  auto enqueue_piece = [&](int len) -> int {
    // prologue: accelerate_flow of the first step on the current grid (kernels.cl:9-53); later steps get theirs fused into
    // the previous launch's write of row ny-2.  Open boundaries: no accelerate_flow anywhere.
    if (!d->flow.open) {
      hipLaunchKernelGGL(dp_accelerate_row, dim3(div_up(nx, 128), 1), dim3(128), 0, d->q.st, d->cells[d->cur], d->plane_stride, 0ull,
                         (const uint8_t *)d->mask, (const DpMember *)d->members, nx, ny, (const int *)nullptr);
      HIP_TRY(hipGetLastError());
    }
    int i = 0;
    while (i < len) {
      // the LDS-tile form: the remaining steps in as few launches as possible, of equal depth (20 steps at T = 8: 7 + 7 + 6)
      const int rem = len - i;
      const int adv = (T > 0 && !scalar) ? equal_depth(rem, T) : 1;
      if (d->ring_fill + adv > scalar_ring_limit(d->scalar, d->ring))
        if (int rc = flush()) return rc;
      // scalar step n before flow step n, on the state that flow step streams
      if (scalar)
        if (int rc = scalar_step(d->scalar, sgrid, d->q.st, d->cells[d->cur], d->mask, d->flow.open, buoy ? d->buoy.table : nullptr,
                                 d->ring_fill, nullptr))
          return rc;
      const bool accel_next = !d->flow.open && i + adv < len;
      double *seg = d->seg + (size_t)d->ring_fill * slot;
      if (buoy) {
        // flow step n reads the scalar array that scalar step n has just written
        DpBuoyArgs a{};
        a.src = d->cells[d->cur];
        a.dst = d->cells[d->cur ^ 1];
        a.mask = d->mask;
        a.scalar = d->scalar.g[d->scalar.cur];
        a.members = d->buoy.table;
        a.wall_u = d->flow.wall_dev;
        a.seg = seg;
        a.plane_stride = d->plane_stride;
        a.member_stride = 0;
        a.nx = nx;
        a.ny = ny;
        a.lanes_per_row = d->lanes_per_row;
        a.accel_row = accel_next ? ny - 2 : -1;
        if (int rc = buoy_launch(d->q.st, d->flow.force, d->flow.trt, d->flow.open, d->flow.wall, d->flow.les, a, 1)) return rc;
      } else if (T > 0) {
        DpMultiArgs a{};
        a.src = d->cells[d->cur];
        a.dst = d->cells[d->cur ^ 1];
        a.mask = d->mask;
        a.seg = seg;
        a.plane_stride = d->plane_stride;
        a.seg_step = slot;
        a.nx = nx;
        a.ny = ny;
        a.nseg = d->nseg;
        a.tiles_x = d->tiles_x;
        a.T = adv;
        a.accel_next = accel_next ? 1 : 0;
        a.omega = d->p.omega;
        a.aw1 = aw1;
        a.aw2 = aw2;
        a.omega_m = omega_m;
        a.u_in = u_in;
        a.rho_out = rho_out;
        launch_multi(d, a);
      } else {
        DpStepArgs a{};
        a.src = d->cells[d->cur];
        a.dst = d->cells[d->cur ^ 1];
        a.mask = d->mask;
        a.seg = seg;
        a.plane_stride = d->plane_stride;
        a.nx = nx;
        a.ny = ny;
        a.lanes_per_row = d->lanes_per_row;
        a.accel_row = accel_next ? ny - 2 : -1;
        a.omega = d->p.omega;
        a.aw1 = aw1;
        a.aw2 = aw2;
        a.omega_m = omega_m;
        a.u_in = u_in;
        a.rho_out = rho_out;
        launch_step(d, a);
      }
      HIP_TRY(hipGetLastError());
      d->cur ^= 1;
      d->ring_fill += adv;
      i += adv;
    }
    return LBM_OK;
  };
  for (const StatsPiece &piece : pieces) {
    if (int rc = enqueue_piece(piece.len)) return rc;
    // the sample behind a piece that ends on a sample point: the state lbm_dp_final_state would read here
    if (piece.sample)
      if (int rc = stats_sample(d->stats, sgrid, d->q.st, d->cells[d->cur], d->mask, d->members, drive_dev(d),
                                buoy ? d->scalar.g[d->scalar.cur] : nullptr, buoy ? d->buoy.table : nullptr))
        return rc;
  }
  if (int rc = flush()) return rc;
  d->steps_done += nsteps;
  return timed_end(d->q, timed, ms);
}

int run_dp(lbm_dp *d, int nsteps, bool timed, double *ms) {
  bool launched = false;
  const int rc = run_dp_impl(d, nsteps, timed, ms, &launched);
  return latch_failure(rc, launched, d->q.st, &d->failed);
}

// the output stage into `d[0..3]` (any may be NULL) and the per-block sums of u
int final_fields_dp(lbm_dp *d, double *const (&dst)[4]) {
  const size_t n = (size_t)d->p.nx * d->p.ny;
  // buoyancy: the half-force of the scalar state that is current, per cell
  const bool buoy = d->scalar.on && d->buoy.on;
  if (buoy)
    if (int rc = buoy_sync(d->buoy, d->flow, flow_grid(d))) return rc;
  hipLaunchKernelGGL(dp_final_fields, dim3(d->fin_blocks, 1), dim3(kBlock), 0, d->q.st, (const double *)d->cells[d->cur],
                     (const double *)nullptr, (const int *)nullptr, d->plane_stride, 0ull, d->p.nx, (const uint8_t *)d->mask, n,
                     (const DpMember *)d->members, drive_dev(d), buoy ? (const double *)d->scalar.g[d->scalar.cur] : (const double *)nullptr,
                     (const double *)nullptr, buoy ? (const DpBuoyMember *)d->buoy.table : (const DpBuoyMember *)nullptr, dst[0], dst[1], dst[2], dst[3],
                     d->fin_partials);
  HIP_TRY(hipGetLastError());
  return LBM_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

int lbm_dp_create(lbm_dp **out, const lbm_dparams *p, const int32_t *obstacles) {
  // every argument error is reported before a device is touched
  if (!out) return lbm_fail(LBM_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (!p) return lbm_fail(LBM_ERR_ARG, "params is NULL");
  if (!obstacles) return lbm_fail(LBM_ERR_ARG, "obstacles is NULL");
  if (p->nx < 3 || p->ny < 3) return lbm_fail(LBM_ERR_ARG, "grid must be at least 3x3 (got %dx%d)", p->nx, p->ny);
  if (p->max_iters < 1) return lbm_fail(LBM_ERR_ARG, "max_iters must be >= 1 (got %d)", p->max_iters);
  if (!positive_finite(p->omega)) return lbm_fail(LBM_ERR_ARG, "omega must be finite and positive (got %g)", p->omega);
  if (!positive_finite(p->density)) return lbm_fail(LBM_ERR_ARG, "density must be finite and positive (got %g)", p->density);
  if (!std::isfinite(p->accel)) return lbm_fail(LBM_ERR_ARG, "accel must be finite (got %g)", p->accel);
  int ndev_visible = 0;
  HIP_TRY(hipGetDeviceCount(&ndev_visible));
  if (ndev_visible < 1) return lbm_fail(LBM_ERR_HIP, "no HIP device visible");

  lbm_dp *d = new lbm_dp();
  d->p = *p;
  if (int rc = build_dp(d, obstacles)) {
    const std::string keep = lbm_last_error();
    free_dp(d);
    return fail_again(rc, keep);
  }
  *out = d;
  return LBM_OK;
}

int lbm_dp_upload(lbm_dp *d, const double *cells) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (int rc = queue_sync(d->q)) return rc;
  const size_t n = (size_t)d->p.nx * d->p.ny;
  const dim3 grid((unsigned)std::min(div_up((long)n, 256), 4096L));
  if (cells) {
    // one transfer of the caller's double[9][ny][nx] into the second grid array (9 nx ny <= its size), then one launch that
    // scatters the planes into the first (d2q9-bgk.c:200-203)
    HIP_TRY(hipMemcpyAsync(d->cells[1], cells, 9 * n * sizeof(double), hipMemcpyHostToDevice, d->q.st));
    hipLaunchKernelGGL(dp_pack_planes<true>, grid, dim3(256), 0, d->q.st, d->cells[0], (double *)nullptr, (const int *)nullptr,
                       d->plane_stride, 0ull, d->p.nx, n, d->cells[1]);
  } else {
    // d2q9-bgk.c:529-550 in double: the member table's w0, w1, w2
    hipLaunchKernelGGL(dp_init_cells, grid, dim3(256), 0, d->q.st, d->cells[0], d->plane_stride, 0ull, (const DpMember *)d->members,
                       d->p.nx, n);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(d->q.st));
  d->cur = 0;
  d->steps_done = 0;
  d->ring_fill = 0;
  // the statistics keep their setting and start anew
  return stats_restart(d->stats, scalar_grid(d), d->q.st, d->steps_done);
}

int lbm_dp_upload_obstacles(lbm_dp *d, const int32_t *obstacles) {
  if (!d || !obstacles) return lbm_fail(LBM_ERR_ARG, "NULL argument");
  if (int rc = queue_sync(d->q)) return rc;
  // the body map, if one was set, described the old map's blocked cells: every blocked cell counts again
  if (int rc = upload_mask(d->mask, obstacles, (size_t)d->p.nx * d->p.ny)) return rc;
  body_reset(d->body, obstacles, (size_t)d->p.nx * d->p.ny);
  // wall velocities stay as set: a kernel reads one only while its cell is blocked; so do the scalar's state and its c_wall
  // open boundaries stay on: the blocked cells of columns 0 and nx - 1 are outside every body
  if (d->flow.open)
    if (int rc = body_rewrite(d->body, d->mask, d->p.nx, true)) return rc;
  // the statistics keep their setting and start anew: the sums before and behind it would be those of two geometries
  return stats_restart(d->stats, scalar_grid(d), d->q.st, d->steps_done);
}

int lbm_dp_run(lbm_dp *d, int nsteps) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  return run_dp(d, nsteps, false, nullptr);
}

int lbm_dp_run_timed(lbm_dp *d, int nsteps, double *ms) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  return run_dp(d, nsteps, true, ms);
}

int lbm_dp_sync(lbm_dp *d) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  return queue_sync(d->q);
}

int lbm_dp_steps_done(const lbm_dp *d) { return d ? d->steps_done : -1; }

int lbm_dp_download(lbm_dp *d, double *cells_out, double *av_vels_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (int rc = queue_sync(d->q)) return rc;
  const size_t n = (size_t)d->p.nx * d->p.ny;
  if (cells_out) {
    // the grid array that is not current is scratch between runs: repack there, then one contiguous transfer
    double *stage = d->cells[d->cur ^ 1];
    hipLaunchKernelGGL(dp_pack_planes<false>, dim3((unsigned)std::min(div_up((long)n, 256), 4096L), 1), dim3(256), 0, d->q.st,
                       d->cells[d->cur], (double *)nullptr, (const int *)nullptr, d->plane_stride, 0ull, d->p.nx, n, stage);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cells_out, stage, 9 * n * sizeof(double), hipMemcpyDeviceToHost, d->q.st));
    HIP_TRY(hipStreamSynchronize(d->q.st));
  }
  if (av_vels_out && d->steps_done > 0) {
    std::vector<double> sums(d->steps_done);
    HIP_TRY(hipMemcpy(sums.data(), d->av_sum, sums.size() * sizeof(double), hipMemcpyDeviceToHost));
    // kernels.cl:202: sum * FREE_CELLS_INV, in double
    for (int t = 0; t < d->steps_done; t++) av_vels_out[t] = sums[t] * d->p.free_cells_inv;
  }
  return LBM_OK;
}

int lbm_dp_final_state(lbm_dp *d, double *u_x, double *u_y, double *u, double *pressure) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (int rc = queue_sync(d->q)) return rc;
  const size_t n = (size_t)d->p.nx * d->p.ny;
  double *outs[4] = {u_x, u_y, u, pressure};
  // the four columns go to the grid array that is not current (4 nx ny of its 9 plane_stride ny doubles)
  double *dst[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < 4; i++)
    if (outs[i]) dst[i] = d->cells[d->cur ^ 1] + (size_t)i * n;
  if (int rc = final_fields_dp(d, dst)) return rc;
  for (int i = 0; i < 4; i++)
    if (outs[i]) HIP_TRY(hipMemcpyAsync(outs[i], dst[i], n * sizeof(double), hipMemcpyDeviceToHost, d->q.st));
  HIP_TRY(hipStreamSynchronize(d->q.st));
  return LBM_OK;
}

int lbm_dp_reynolds(lbm_dp *d, double *reynolds_out) {
  if (!d || !reynolds_out) return lbm_fail(LBM_ERR_ARG, "NULL argument");
  if (int rc = queue_sync(d->q)) return rc;
  double *none[4] = {nullptr, nullptr, nullptr, nullptr};
  if (int rc = final_fields_dp(d, none)) return rc;
  std::vector<double> part(d->fin_blocks);
  HIP_TRY(hipMemcpyAsync(part.data(), d->fin_partials, part.size() * sizeof(double), hipMemcpyDeviceToHost, d->q.st));
  HIP_TRY(hipStreamSynchronize(d->q.st));
  double tot = 0.0;
  for (double v : part) tot += v;
  // av_velocity + calc_reynolds, d2q9-bgk.c:396-442, 747-752, in double
  const double viscosity = 1.0 / 6.0 * (2.0 / d->p.omega - 1.0);
  *reynolds_out = tot * d->p.free_cells_inv * (double)d->p.reynolds_dim / viscosity;
  return LBM_OK;
}

int lbm_dp_set_option(lbm_dp *d, const char *key, long value) {
  if (!d || !key) return lbm_fail(LBM_ERR_ARG, "NULL argument");
  if (!strcmp(key, "multistep")) {
    if (value < -1 || value > kDpTMax) return lbm_fail(LBM_ERR_ARG, "multistep must be -1 (auto), 0 or 1..%d (got %ld)", kDpTMax, value);
    d->multistep = (int)value;
    return LBM_OK;
  }
  if (!strcmp(key, "force")) {
    if (int rc = force_check(value)) return rc;
    return force_set(d->flow, flow_grid(d), value, false, d->force_rec, d->failed);
  }
  return lbm_fail(LBM_ERR_ARG, "unknown option '%s' (a double-precision context has \"multistep\" and \"force\")", key);
}

int lbm_dp_get_option(const lbm_dp *d, const char *key, long *value) {
  if (!d || !key || !value) return lbm_fail(LBM_ERR_ARG, "NULL argument");
  if (!strcmp(key, "multistep")) {
    *value = multistep_effective(d);
    return LBM_OK;
  }
  if (!strcmp(key, "force")) {
    *value = d->flow.force ? 1 : 0;
    return LBM_OK;
  }
  return lbm_fail(LBM_ERR_ARG, "unknown option '%s' (a double-precision context has \"multistep\" and \"force\")", key);
}

int lbm_dforce_record(lbm_dp *d, double *fx_out, double *fy_out) {
  // argument errors before a device is touched
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!fx_out && !fy_out) return lbm_fail(LBM_ERR_ARG, "fx_out and fy_out are both NULL");
  if (!d->flow.force) return lbm_fail(LBM_ERR_STATE, "no force record: option \"force\" is off (lbm_dp_set_option before the first step)");
  if (int rc = queue_sync(d->q)) return rc;
  double *outs[2] = {fx_out, fy_out};
  for (int c = 0; c < 2; c++)
    if (outs[c] && d->steps_done > 0)
      HIP_TRY(hipMemcpy(outs[c], d->force_rec + (size_t)c * d->p.max_iters, (size_t)d->steps_done * sizeof(double),
                        hipMemcpyDeviceToHost));
  return LBM_OK;
}

int lbm_dforce(lbm_dp *d, double *fx, double *fy) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!fx && !fy) return lbm_fail(LBM_ERR_ARG, "fx and fy are both NULL");
  if (int rc = queue_sync(d->q)) return rc;
  if (!d->force_now) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d->force_now), 2 * sizeof(double)));
  DpForceArgs a{};
  a.cells = d->cells[d->cur];
  a.mask = d->mask;
  a.members = d->members;
  a.plane_stride = d->plane_stride;
  a.nx = d->p.nx;
  a.ny = d->p.ny;
  a.no_accel = d->flow.open ? 1 : 0;
  if (int rc = force_state(d->q.st, a, d->nseg, 1, d->seg, d->red, d->red_blocks, d->force_now)) return rc;
  double f[2] = {0.0, 0.0};
  HIP_TRY(hipMemcpyAsync(f, d->force_now, sizeof(f), hipMemcpyDeviceToHost, d->q.st));
  HIP_TRY(hipStreamSynchronize(d->q.st));
  if (fx) *fx = f[0];
  if (fy) *fy = f[1];
  return LBM_OK;
}

int lbm_dbody_set(lbm_dp *d, const int32_t *body) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (d->flow.force && d->steps_done != 0)
    return lbm_fail(LBM_ERR_STATE, "with \"force\" on, a body map is set before the first step (%d done): one record holds one body",
                    d->steps_done);
  if (int rc = queue_sync(d->q)) return rc;
  return body_apply(d->body, d->mask, body, 1, d->p.ny, d->p.nx, false, d->flow.open);
}

int lbm_dbody_get(lbm_dp *d, int32_t *body_out) {
  // argument errors before anything of the context is read
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!body_out) return lbm_fail(LBM_ERR_ARG, "body_out is NULL");
  body_read(d->body, body_out);
  return LBM_OK;
}

// The six setters: the context's value as dp_host.h takes it (an array of one member; the context's "0 = off" is its NULL), the
// check of the values, which reads nothing of the context but p, then the set.
int lbm_dtrt_set(lbm_dp *d, double magic) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  const double *on = magic == 0.0 ? nullptr : &magic;
  if (int rc = trt_check(&d->p, 1, on, false)) return rc;
  return trt_set(d->flow, flow_grid(d), on);
}

int lbm_dtrt_get(const lbm_dp *d, double *magic_out, double *omega_minus_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!magic_out && !omega_minus_out) return lbm_fail(LBM_ERR_ARG, "magic_out and omega_minus_out are both NULL");
  trt_get(d->flow, magic_out, omega_minus_out);
  return LBM_OK;
}

int lbm_dopen_set(lbm_dp *d, const double *u_in, double rho_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (int rc = open_check(&d->p, 1, u_in, &rho_out, false)) return rc;
  return open_set(d->flow, flow_grid(d), d->body, d->mask, u_in, &rho_out);
}

int lbm_dopen_get(const lbm_dp *d, int *on_out, double *u_in_out, double *rho_out_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!on_out && !u_in_out && !rho_out_out) return lbm_fail(LBM_ERR_ARG, "on_out, u_in_out and rho_out_out are all NULL");
  open_get(d->flow, 1, d->p.ny, on_out, u_in_out, rho_out_out);
  return LBM_OK;
}

int lbm_dwall_set(lbm_dp *d, const double *u_x, const double *u_y, double rho_wall) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if ((u_x == nullptr) != (u_y == nullptr))
    return lbm_fail(LBM_ERR_ARG, "%s is NULL and %s is not: a wall velocity has two components (both NULL: off)", u_x ? "u_y" : "u_x",
                    u_x ? "u_x" : "u_y");
  if (int rc = wall_values_check(d->body, &d->p, 1, u_x, u_y, &rho_wall, false)) return rc;
  return wall_set(d->flow, flow_grid(d), u_x, u_y, &rho_wall);
}

int lbm_dwall_get(const lbm_dp *d, int *on_out, double *u_x_out, double *u_y_out, double *rho_wall_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!on_out && !u_x_out && !u_y_out && !rho_wall_out)
    return lbm_fail(LBM_ERR_ARG, "on_out, u_x_out, u_y_out and rho_wall_out are all NULL");
  wall_get(d->flow, on_out, u_x_out, u_y_out, rho_wall_out);
  return LBM_OK;
}

int lbm_dles_set(lbm_dp *d, double c) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  const double *on = c == 0.0 ? nullptr : &c;
  if (int rc = les_check(1, on, false)) return rc;
  return les_set(d->flow, flow_grid(d), on);
}

int lbm_dles_get(const lbm_dp *d, double *c_out, double *les_k_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!c_out && !les_k_out) return lbm_fail(LBM_ERR_ARG, "c_out and les_k_out are both NULL");
  les_get(d->flow, &d->p, 1, c_out, les_k_out);
  return LBM_OK;
}

int lbm_ddrive_set(lbm_dp *d, double f_x, double f_y) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  const double f[2] = {f_x, f_y};
  if (int rc = drive_check(1, f, false)) return rc;
  return drive_set(d->flow, flow_grid(d), dp_drive_on(f_x, f_y) ? f : nullptr);
}

int lbm_ddrive_get(const lbm_dp *d, double *f_x_out, double *f_y_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!f_x_out && !f_y_out) return lbm_fail(LBM_ERR_ARG, "f_x_out and f_y_out are both NULL");
  double f[2];
  drive_get(d->flow, nullptr, f);
  if (f_x_out) *f_x_out = f[0];
  if (f_y_out) *f_y_out = f[1];
  return LBM_OK;
}

int lbm_dscalar_set(lbm_dp *d, double diffusivity, const double *c0, const double *c_wall, const double *c_in) {
  // argument errors before anything of the context is read
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!std::isfinite(diffusivity) || diffusivity < 0.0)
    return lbm_fail(LBM_ERR_ARG, "the diffusivity must be finite and positive, or 0 (off) (got %g)", diffusivity);
  if (diffusivity > 0.0 && !c0) return lbm_fail(LBM_ERR_ARG, "c0 is NULL (the diffusivity is positive: a scalar starts from a field)");
  const ScalarGrid gr = scalar_grid(d);
  if (diffusivity > 0.0)
    if (int rc = scalar_check(gr, false, &diffusivity, c0, c_wall, c_in)) return rc;
  if (diffusivity == 0.0 && d->buoy.on) return buoy_refuse_scalar_off();
  if (diffusivity == 0.0 && d->scalar.on && d->scalar.record) return scalar_record_refuse_scalar_off();
  if (int rc = queue_sync(d->q)) return rc;
  if (diffusivity == 0.0) return scalar_off(d->scalar);
  return scalar_set(d->scalar, gr, d->q.st, &diffusivity, c0, c_wall, c_in, drive_dev(d));
}

int lbm_dscalar_get(const lbm_dp *d, int *on_out, double *diffusivity_out, double *omega_s_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!on_out && !diffusivity_out && !omega_s_out)
    return lbm_fail(LBM_ERR_ARG, "on_out, diffusivity_out and omega_s_out are all NULL");
  if (on_out) *on_out = d->scalar.on ? 1 : 0;
  if (diffusivity_out) *diffusivity_out = d->scalar.on ? d->scalar.diffusivity[0] : 0.0;
  if (omega_s_out) *omega_s_out = d->scalar.on ? d->scalar.omega_s[0] : 0.0;
  return LBM_OK;
}

int lbm_dscalar_field(lbm_dp *d, double *c_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!c_out) return lbm_fail(LBM_ERR_ARG, "c_out is NULL");
  if (!d->scalar.on) return scalar_refuse_off("lbm_dscalar_field");
  if (int rc = queue_sync(d->q)) return rc;
  return scalar_field(d->scalar, scalar_grid(d), d->q.st, d->mask, c_out);
}

int lbm_dscalar_download(lbm_dp *d, double *g_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!g_out) return lbm_fail(LBM_ERR_ARG, "g_out is NULL");
  if (!d->scalar.on) return scalar_refuse_off("lbm_dscalar_download");
  if (int rc = queue_sync(d->q)) return rc;
  return scalar_download(d->scalar, scalar_grid(d), d->q.st, g_out);
}

int lbm_dscalar_upload(lbm_dp *d, const double *g) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!g) return lbm_fail(LBM_ERR_ARG, "g is NULL");
  if (!d->scalar.on) return scalar_refuse_off("lbm_dscalar_upload");
  if (int rc = queue_sync(d->q)) return rc;
  return scalar_upload(d->scalar, scalar_grid(d), d->q.st, g);
}

int lbm_drecord_set(lbm_dp *d, int on) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (int rc = scalar_record_check(d->scalar, on, d->steps_done, false)) return rc;
  if (int rc = queue_sync(d->q)) return rc;
  HIP_TRY(hipSetDevice(d->q.dev));
  return scalar_record_set(d->scalar, scalar_grid(d), on);
}

int lbm_drecord_get(const lbm_dp *d, int *on_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!on_out) return lbm_fail(LBM_ERR_ARG, "on_out is NULL");
  *on_out = d->scalar.on && d->scalar.record ? 1 : 0;
  return LBM_OK;
}

int lbm_drecord(lbm_dp *d, double *content_out, double *flux_x_out, double *flux_y_out) {
  // argument errors before a device is touched
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!content_out && !flux_x_out && !flux_y_out) return lbm_fail(LBM_ERR_ARG, "content_out, flux_x_out and flux_y_out are all NULL");
  if (!d->scalar.on || !d->scalar.record) return scalar_record_refuse_off("lbm_drecord", false);
  if (int rc = queue_sync(d->q)) return rc;
  double *const outs[3] = {content_out, flux_x_out, flux_y_out};
  return scalar_record_read(d->scalar, scalar_grid(d), d->steps_done, nullptr, outs);
}

int lbm_dbuoy_set(lbm_dp *d, double b_x, double b_y, double c_ref) {
  // argument errors before anything of the context is read
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  const double b[3] = {b_x, b_y, c_ref};
  if (int rc = buoy_check_values(b, 1, false)) return rc;
  const bool on = dp_drive_on(b_x, b_y);
  if (int rc = buoy_check_state(d->scalar, d->steps_done, on)) return rc;
  if (int rc = queue_sync(d->q)) return rc;
  HIP_TRY(hipSetDevice(d->q.dev));
  return buoy_set(d->buoy, on ? b : nullptr, 1);
}

int lbm_dbuoy_get(const lbm_dp *d, int *on_out, double *b_out, double *c_ref_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!on_out && !b_out && !c_ref_out) return lbm_fail(LBM_ERR_ARG, "on_out, b_out and c_ref_out are all NULL");
  if (on_out) *on_out = d->buoy.on ? 1 : 0;
  if (b_out) {
    b_out[0] = d->buoy.on ? d->buoy.b[0] : 0.0;
    b_out[1] = d->buoy.on ? d->buoy.b[1] : 0.0;
  }
  if (c_ref_out) *c_ref_out = d->buoy.on ? d->buoy.b[2] : 0.0;
  return LBM_OK;
}

int lbm_dstats_set(lbm_dp *d, int every) {
  // argument errors before anything of the context is read
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (int rc = stats_check(every)) return rc;
  if (int rc = queue_sync(d->q)) return rc;
  return stats_set(d->stats, scalar_grid(d), d->q.st, every, d->steps_done);
}

int lbm_dstats_get(const lbm_dp *d, int *every_out, int *origin_out, int *samples_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!every_out && !origin_out && !samples_out) return lbm_fail(LBM_ERR_ARG, "every_out, origin_out and samples_out are all NULL");
  stats_get(d->stats, every_out, origin_out, samples_out);
  return LBM_OK;
}

int lbm_dstats(lbm_dp *d, double *sums_out) {
  if (!d) return lbm_fail(LBM_ERR_ARG, "context is NULL");
  if (!sums_out) return lbm_fail(LBM_ERR_ARG, "sums_out is NULL");
  if (!d->stats.every) return stats_refuse_off("lbm_dstats", false);
  if (int rc = queue_sync(d->q)) return rc;
  return stats_read(d->stats, scalar_grid(d), sums_out);
}

void lbm_dp_destroy(lbm_dp *d) {
  if (!d) return;
  (void)hipSetDevice(d->q.dev);
  free_dp(d);
}

}  // extern "C"

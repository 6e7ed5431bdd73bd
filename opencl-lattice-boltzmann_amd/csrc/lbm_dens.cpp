// Fifth translation unit of liblbm_hip.so: the host side of the double-precision ensembles (include/lbm.h: lbm_dens_*).
//
// A double-precision ensemble is N independent fp64 grids of one size on one device, each with its own run constants,
// obstacle map and state: lbm_ensemble.cpp's bookkeeping (all members in one pair of arrays a member stride apart, one mask
// array, one table of per-member constants, every entry point one launch or one transfer for all members) over
// lbm_dp.cpp's numerics (the layout and arithmetic of dp_kernels.h, the ring of per-step segment sums, the one- or two-stage
// reduction in a fixed order).  Every size that decides an order of additions - segments per step, blocks of the first
// reduction stage, blocks of the output stage - is computed from the member's nx and ny exactly as lbm_dp.cpp computes it
// from a grid's, so a member's cells, av_vels, fields and Reynolds number are those of an lbm_dp context, bit for bit.
// The reference has no counterpart: one grid, one in-order queue (d2q9-bgk.c:221-239).
//
// A steady run (lbm_dsteady_*) is the same loop cut into legs of `window` steps behind a per-member `active` word that a
// criterion kernel clears on the device (dp_steady_kernels.h), as lbm_ensemble.cpp's.  Members may then stop on different
// launch parities, so from the end of such a run until the next upload the array that holds a member's state is the
// member's own (`par`).
#include "../../include/lbm.h"
#include "dp_host.h"
#include "dp_steady_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace lbm;
using namespace lbm_host;

namespace {

constexpr long kDensMaxCells = 300L * 1024;   // up to here lbm_dp itself takes the LDS-tile form (multistep_effective, lbm_dp.cpp)
constexpr int kDensMaxMembers = 65535;        // member index = blockIdx.y (blockIdx.z in dp_reduce)
constexpr long kDensSegsPerBlock = 4096;      // segments per block of the first reduction stage: lbm_dp.cpp's kDpSegsPerBlock

// The instantiated form of d2q9_dp_ensemble<16, TY, TMAX, threads>: 16 x 16 at T <= 3 with 1024 threads, two workgroups per
// CU (dp_ensemble_kernels.h holds the measurements behind the choice).  A measurement build takes another form:
// make LBM_DENS_FLAGS="-DLBM_DENS_TY=8 -DLBM_DENS_TMAX=4 -DLBM_DENS_THREADS=512" (tools/dp_ensemble_ab.py).
#ifndef LBM_DENS_TY
#define LBM_DENS_TY 16
#endif
#ifndef LBM_DENS_TMAX
#define LBM_DENS_TMAX 3
#endif
#ifndef LBM_DENS_THREADS
#define LBM_DENS_THREADS 1024
#endif
constexpr int kDensTX = 16, kDensTY = LBM_DENS_TY, kDensTMax = LBM_DENS_TMAX, kDensThreads = LBM_DENS_THREADS;

}  // namespace

struct lbm_dens {
  int n = 0;
  int nx = 0, ny = 0, max_iters = 0;
  std::vector<lbm_dparams> p;
  Queue q;
  size_t plane_stride = 0, member_stride = 0;  // doubles
  double *cells[2] = {nullptr, nullptr};
  uint8_t *mask = nullptr;         // [n][ny][nx]: 0 fluid, 1 blocked and counted in the force, 2 blocked outside the body
  BodyMap body;                    // the host's copy of what the mask was made of (body_map.h)
  DpMember *members = nullptr;     // [n], then the open-boundary table double[n][ny + 1] (dens_open_table), then rho_wall[n]
                                   // (dens_wall_table), then DpLes[n] (dens_les_table), then the body forces double[n][2]
                                   // (dens_drive_table): dp_host.h allocates and writes them, the kernels read them
  double *seg = nullptr;           // [ring][n][ny][nseg]
  double *red = nullptr;           // [ring][n][red_blocks]: first reduction stage
  double *av_sum = nullptr;        // [n][max_iters]
  double *fin_partials = nullptr;  // [n][fin_blocks]
  double *force_rec = nullptr;     // option "force": [2][n][max_iters], F_x then F_y per member and step
  double *force_now = nullptr;     // [2][n]: lbm_dforce_ens's F_x, F_y (allocated by the first call)
  FlowState flow;                  // "force", lbm_dtrt_ens_set, lbm_dopen_ens_set, lbm_dwall_ens_set, lbm_dles_ens_set,
                                   // lbm_ddrive_ens_set: the members' settings (dp_host.h), all off by default
  ScalarState scalar;              // lbm_dscalar_ens_set: the members' scalars (dp_host.h), off by default
  BuoyState buoy;                  // lbm_dbuoy_ens_set: the scalars act back on the members' flows (dp_host.h), off by default
  StatsState stats;                // lbm_dstats_ens_set: the members' running statistics (dp_host.h), off by default
  int nseg = 1, red_blocks = 1, fin_blocks = 1;
  int tiles_x = 1, tiles = 1;
  int ring = 8, ring_fill = 0;
  int cur = 0, steps_done = 0;
  bool failed = false;
  // steady runs (allocated by the first lbm_dsteady_run)
  int *steady_words = nullptr;       // device: active[n], par[n], steps[n], conv[n], count
  double *steady_inv = nullptr;      // device: free_cells_inv[n]
  int *steady_count_host = nullptr;  // page-locked: where the count of active members is read back to
  double *stage = nullptr;           // device, double[n][9][ny][nx]: staging of downloads while the ensemble is ragged
  std::vector<int> m_steps, m_conv;  // host copies of the words after the last steady run (empty: none since the upload)
  bool ragged = false;               // members stopped at different step counts: download and output only, until an upload
  int scalar_off = 0;                // while ragged with a scalar on: member m's scalar lies in scalar.g[par[m] ^ scalar_off] (cur and
                                     // scalar.cur both flip once per step: their difference is constant over a run)
  double *scalar_stage = nullptr;    // device, double[n][5][ny][nx]: staging of the scalar's output while the ensemble is ragged
};

namespace {

void free_dens(lbm_dens *e) {
  queue_drain(e->q);
  for (double *c : e->cells)
    if (c) (void)hipFree(c);
  if (e->mask) (void)hipFree(e->mask);
  if (e->members) (void)hipFree(e->members);
  if (e->seg) (void)hipFree(e->seg);
  if (e->red) (void)hipFree(e->red);
  if (e->av_sum) (void)hipFree(e->av_sum);
  if (e->fin_partials) (void)hipFree(e->fin_partials);
  if (e->force_rec) (void)hipFree(e->force_rec);
  if (e->force_now) (void)hipFree(e->force_now);
  if (e->steady_words) (void)hipFree(e->steady_words);
  if (e->steady_inv) (void)hipFree(e->steady_inv);
  if (e->steady_count_host) (void)hipHostFree(e->steady_count_host);
  if (e->stage) (void)hipFree(e->stage);
  if (e->scalar_stage) (void)hipFree(e->scalar_stage);
  if (e->flow.wall_dev) (void)hipFree(e->flow.wall_dev);
  scalar_free(e->scalar);
  buoy_free(e->buoy);
  stats_free(e->stats);
  queue_destroy(e->q);
  delete e;
}

// the members' grids and their ring as the setters take them (dp_host.h)
FlowGrid flow_grid(lbm_dens *e) {
  return FlowGrid{e->n, e->p.data(), e->members, e->q, e->steps_done, e->seg, e->red, e->ring, (size_t)e->ny * e->nseg,
                  e->red_blocks, kDensTMax};
}

int build_dens(lbm_dens *e, const int32_t *obstacles) {
  const int n = e->n, nx = e->nx, ny = e->ny;
  const size_t cells_per = (size_t)nx * ny;
  HIP_TRY(hipGetDevice(&e->q.dev));
  e->tiles_x = (int)div_up(nx, kDensTX);
  e->tiles = e->tiles_x * (int)div_up(ny, kDensTY);
  // the sizes of build_dp (lbm_dp.cpp), from the member's nx and ny alone: they fix the order of every sum
  e->plane_stride = ((size_t)(nx + 31) / 32) * 32;
  e->member_stride = 9 * e->plane_stride * ny;
  e->nseg = (int)div_up(div_up(nx, 2), 8);                     // = ceil(nx / 16)
  const size_t per_step = (size_t)ny * e->nseg;                // one member's segments of one step
  e->red_blocks = (int)std::min(512L, div_up((long)per_step, kDensSegsPerBlock));
  e->fin_blocks = (int)std::max(1L, std::min(div_up((long)cells_per, kBlock), 2048L));
  const size_t all_step = (size_t)n * per_step;
  e->ring = ring_steps_of(n, per_step, 1, kDensTMax);

  // what the ensemble needs against what the device has free: refuse here rather than fail half-way through
  const size_t cells_bytes = ((size_t)n * e->member_stride + 32) * sizeof(double);
  const size_t need = 2 * cells_bytes + (size_t)n * cells_per + 64 + flow_table_bytes(n, ny) +
                      (size_t)e->ring * all_step * sizeof(double) + (size_t)e->ring * n * e->red_blocks * sizeof(double) +
                      (size_t)n * e->max_iters * sizeof(double) + (size_t)n * e->fin_blocks * sizeof(double);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b)
    return lbm_fail(LBM_ERR_HIP, "a double-precision ensemble of %d members of %dx%d with max_iters=%d needs %.1f MiB of device memory, "
                    "%.1f MiB are free", n, nx, ny, e->max_iters, (double)need / 1048576.0, (double)free_b / 1048576.0);

  if (int rc = queue_create(e->q)) return rc;
  for (int i = 0; i < 2; i++) {
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->cells[i]), cells_bytes));
    HIP_TRY(hipMemset(e->cells[i], 0, cells_bytes));
  }
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->mask), (size_t)n * cells_per + 64));
  // the members' tables, every option off: in double these are lbm_dp.cpp's own statements, a member's constants are a context's
  if (int rc = flow_create(e->flow, &e->members, e->p.data(), n)) return rc;
  if (int rc = alloc_ring(flow_grid(e), 1)) return rc;
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->av_sum), (size_t)n * e->max_iters * sizeof(double)));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->fin_partials), (size_t)n * e->fin_blocks * sizeof(double)));
  // the members' byte masks from the caller's int32[n][ny][nx]
  if (int rc = upload_mask(e->mask, obstacles, (size_t)n * cells_per)) return rc;
  body_reset(e->body, obstacles, (size_t)n * cells_per);
  return LBM_OK;
}

// FORCE from the option "force", TRT from lbm_dtrt_ens_set, OPEN from lbm_dopen_ens_set, WALL from lbm_dwall_ens_set, LES from
// lbm_dles_ens_set, DRIVE from lbm_ddrive_ens_set: with all
// off these are the launches of a library without any of them.  active: NULL for an ordinary run, the members' words for a
// leg of a steady run
void launch_dens(const lbm_dens *e, const DensArgs &a, const int *active) {
  const dim3 grid(e->tiles, e->n), block(kDensThreads);
  const FlowState &f = e->flow;
  dp_with_flags(f.force, f.trt, f.open, f.wall, f.les, f.drive, [&](auto force, auto trt, auto open, auto wall, auto les, auto drive) {
    constexpr bool FORCE = decltype(force)::value, TRT = decltype(trt)::value, OPEN = decltype(open)::value, WALL = decltype(wall)::value,
                   LES = decltype(les)::value, DRIVE = decltype(drive)::value;
    DensArgsOf<WALL> w{};
    static_cast<DensArgs &>(w) = a;
    if constexpr (WALL) w.wall_u = e->flow.wall_dev;
    if (!active)
      hipLaunchKernelGGL((d2q9_dp_ensemble<kDensTX, kDensTY, kDensTMax, kDensThreads, FORCE, TRT, OPEN, WALL, LES, DRIVE>), grid, block, 0,
                         e->q.st, w);
    else
      hipLaunchKernelGGL((d2q9_dp_ensemble_gated<kDensTX, kDensTY, kDensTMax, kDensThreads, FORCE, TRT, OPEN, WALL, LES, DRIVE>), grid, block,
                         0, e->q.st, w, active);
  });
}

// the members' grids as the scalar's helpers take them (dp_host.h), and where the output stage and the scalar read the
// members' body forces
ScalarGrid scalar_grid(const lbm_dens *e) {
  return ScalarGrid{e->n, e->nx, e->ny, e->plane_stride, e->member_stride, e->red_blocks, e->max_iters};
}
const double *drive_dev(const lbm_dens *e) { return e->flow.drive ? dens_drive_table(e->members, e->n, e->ny) : nullptr; }

// nsteps steps from step count `first` on, enqueued: the prologue, the launches, the reductions into the record.  Flips
// e->cur per launch; the caller counts the steps.  active: as launch_dens.  With the running statistics on the run is cut at its
// sample points (stats_plan.h): every piece is enqueued as a run of its length, with a sample behind it where it ends on one.
int enqueue_steps(lbm_dens *e, int nsteps, int first, const int *active) {
  const size_t per_step = (size_t)e->ny * e->nseg, all_step = (size_t)e->n * per_step;
  const int nval = seg_values(e->flow);
  const size_t slot = all_step * nval;   // one step in the ring: [nval][n][ny][nseg]
  // with a scalar on every launch advances one step: the scalar reads each step's velocities (during a steady run, which needs
  // the scalar's record, through dp_scalar_step_rec under `active`)
  const bool scalar = e->scalar.on;
  const ScalarGrid sgrid = scalar_grid(e);
  if (scalar)
    if (int rc = scalar_begin_run(e->scalar, sgrid, drive_dev(e))) return rc;
  // with buoyancy on the flow step is d2q9_dp_buoyant, one step per launch (d2q9_dp_buoyant_gated during a steady run)
  const bool buoy = scalar && e->buoy.on;
  if (buoy)
    if (int rc = buoy_sync(e->buoy, e->flow, flow_grid(e))) return rc;
  std::vector<StatsPiece> pieces;
  if (!stats_plan(first, nsteps, e->stats.origin, e->stats.every, pieces)) return stats_refuse_plan(first, e->stats.origin);

  int batch_first = first;
  // second reduction stage over the buffered steps: |u| into av_sum and, with "force", F_x and F_y into their records,
  // the same launches on each value's segments
  auto flush = [&]() -> int {
    if (e->ring_fill == 0) return LBM_OK;
    const unsigned long long record = (unsigned long long)e->max_iters;
    for (int v = 0; v < nval; v++) {
      double *out = (v == 0 ? e->av_sum : e->force_rec + (size_t)(v - 1) * e->n * e->max_iters) + batch_first;
      if (int rc = reduce_steps(e->q.st, e->seg + (size_t)v * all_step, slot, per_step, e->ring_fill, e->n, e->red, e->red_blocks, out,
                                record, active))
        return rc;
    }
    // the scalar's record: the same steps of its own ring
    if (int rc = scalar_flush(e->scalar, sgrid, e->q.st, e->ring_fill, batch_first, active)) return rc;
    batch_first += e->ring_fill;
    e->ring_fill = 0;
    return LBM_OK;
  };
  // the ring of segment sums and its flushes carry across the cuts
  auto enqueue_piece = [&](int len) -> int {
    // prologue: accelerate_flow of the first step on the current grids (kernels.cl:9-53); later steps get theirs fused
    // into the previous launch's write of row ny-2.  Open boundaries: no accelerate_flow anywhere.
    if (!e->flow.open) {
      hipLaunchKernelGGL(dp_accelerate_row, dim3(div_up(e->nx, 128), e->n), dim3(128), 0, e->q.st, e->cells[e->cur], e->plane_stride,
                         e->member_stride, (const uint8_t *)e->mask, (const DpMember *)e->members, e->nx, e->ny, active);
      HIP_TRY(hipGetLastError());
    }
    int i = 0;
    while (i < len) {
      // the remaining steps in as few launches as possible, of equal depth (8 steps at 3 a launch: 3 + 3 + 2)
      const int rem = len - i;
      const int adv = scalar ? 1 : equal_depth(rem, kDensTMax);
      if (e->ring_fill + adv > scalar_ring_limit(e->scalar, e->ring))
        if (int rc = flush()) return rc;
      // scalar step n before flow step n, on the state that flow step streams
      if (scalar)
        if (int rc = scalar_step(e->scalar, sgrid, e->q.st, e->cells[e->cur], e->mask, e->flow.open, buoy ? e->buoy.table : nullptr,
                                 e->ring_fill, active))
          return rc;
      if (buoy) {
        // flow step n reads the scalar array that scalar step n has just written
        DpBuoyArgs b{};
        b.src = e->cells[e->cur];
        b.dst = e->cells[e->cur ^ 1];
        b.mask = e->mask;
        b.scalar = e->scalar.g[e->scalar.cur];
        b.members = e->buoy.table;
        b.wall_u = e->flow.wall_dev;
        b.seg = e->seg + (size_t)e->ring_fill * slot;
        b.plane_stride = e->plane_stride;
        b.member_stride = e->member_stride;
        b.nx = e->nx;
        b.ny = e->ny;
        b.lanes_per_row = e->nseg * 8;
        b.accel_row = (!e->flow.open && i + adv < len) ? e->ny - 2 : -1;
        if (int rc = buoy_launch(e->q.st, e->flow.force, e->flow.trt, e->flow.open, e->flow.wall, e->flow.les, b, e->n, active)) return rc;
        e->cur ^= 1;
        e->ring_fill += adv;
        i += adv;
        continue;
      }
      DensArgs a{};
      a.src = e->cells[e->cur];
      a.dst = e->cells[e->cur ^ 1];
      a.mask = e->mask;
      a.members = e->members;
      a.seg = e->seg + (size_t)e->ring_fill * slot;
      a.plane_stride = e->plane_stride;
      a.member_stride = e->member_stride;
      a.seg_step = slot;
      a.nx = e->nx;
      a.ny = e->ny;
      a.nseg = e->nseg;
      a.tiles_x = e->tiles_x;
      a.T = adv;
      a.accel_next = (!e->flow.open && i + adv < len) ? 1 : 0;
      launch_dens(e, a, active);
      HIP_TRY(hipGetLastError());
      e->cur ^= 1;
      e->ring_fill += adv;
      i += adv;
    }
    return LBM_OK;
  };
  for (const StatsPiece &piece : pieces) {
    if (int rc = enqueue_piece(piece.len)) return rc;
    // the sample behind a piece that ends on a sample point: the state lbm_dens_final_state would read here
    if (piece.sample)
      if (int rc = stats_sample(e->stats, sgrid, e->q.st, e->cells[e->cur], e->mask, e->members, drive_dev(e),
                                buoy ? e->scalar.g[e->scalar.cur] : nullptr, buoy ? e->buoy.table : nullptr))
        return rc;
  }
  return flush();
}

int refuse_steady_scalar(const char *what) {
  return lbm_fail(LBM_ERR_ARG, "%s: the members carry a scalar (lbm_dscalar_ens_set): a member that stops would need a gated scalar "
                  "kernel, which is out of scope; switch the scalar off for a steady run", what);
}

int refuse_ragged(const lbm_dens *e) {
  return lbm_fail(LBM_ERR_STATE, "the members of this ensemble stopped at different step counts (lbm_dsteady_run; %d is the "
                  "largest): download them, then lbm_dens_upload before the next run", e->steps_done);
}

int run_dens_impl(lbm_dens *e, int nsteps, bool timed, double *ms, bool *launched) {
  if (int rc = check_runnable(nsteps, e->failed, "ensemble")) return rc;
  if (e->ragged) return refuse_ragged(e);
  if (int rc = check_record(e->max_iters, e->steps_done, nsteps, "")) return rc;
  if (timed && ms) *ms = 0.0;
  if (nsteps == 0) return LBM_OK;
  HIP_TRY(hipSetDevice(e->q.dev));
  *launched = true;
  if (int rc = timed_begin(e->q, timed)) return rc;
  if (int rc = enqueue_steps(e, nsteps, e->steps_done, nullptr)) return rc;
  e->steps_done += nsteps;
  return timed_end(e->q, timed, ms);
}

int run_dens(lbm_dens *e, int nsteps, bool timed, double *ms) {
  bool launched = false;
  const int rc = run_dens_impl(e, nsteps, timed, ms, &launched);
  return latch_failure(rc, launched, e->q.st, &e->failed);
}

SteadyWords steady_words(const lbm_dens *e) { return steady_words_at(e->steady_words, (size_t)e->n); }

// which array holds member m, for the kernels that read a state: the members' own words while the ensemble is ragged
const int *member_parity(const lbm_dens *e) { return e->ragged ? steady_words(e).par : nullptr; }

// what a steady run needs beyond an ordinary one, allocated by the first
int steady_alloc(lbm_dens *e) {
  if (e->steady_words) return LBM_OK;
  const size_t n = (size_t)e->n;
  if (!e->steady_count_host)
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->steady_count_host), sizeof(int), hipHostMallocDefault));
  if (!e->steady_inv) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->steady_inv), n * sizeof(double)));
  std::vector<double> inv(n);
  for (size_t m = 0; m < n; m++) inv[m] = e->p[m].free_cells_inv;
  HIP_TRY(hipMemcpy(e->steady_inv, inv.data(), n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->steady_words), (kSteadyWordCount * n + 1) * sizeof(int)));
  return LBM_OK;
}

// drag_rec: NULL for the av_vels criterion; the members' F_x records for the drag criterion, or one value of the scalar's record
// for lbm_drecord_steady_run (dens_steady_check without a factor); everything else is one loop
int steady_impl(lbm_dens *e, int max_steps, int window, double rel_tol, const double *drag_rec, bool *launched) {
  if (int rc = check_runnable(max_steps, e->failed, "ensemble")) return rc;  // max_steps >= 0 here (lbm_dsteady_run)
  if (e->ragged) return refuse_ragged(e);
  if (int rc = check_record(e->max_iters, e->steps_done, max_steps, "up to ")) return rc;
  if (max_steps == 0) return LBM_OK;
  HIP_TRY(hipSetDevice(e->q.dev));
  if (int rc = steady_alloc(e)) return rc;
  const int n = e->n, s0 = e->steps_done;
  const int scalar_off = e->cur ^ e->scalar.cur;
  const SteadyWords w = steady_words(e);
  const dim3 mgrid((unsigned)div_up(n, 256)), mblock(256);
  *launched = true;
  hipLaunchKernelGGL(ens_steady_begin, mgrid, mblock, 0, e->q.st, w, n, e->cur, s0);
  HIP_TRY(hipGetLastError());
  int done = 0, checks = 0;
  while (done < max_steps) {
    const int leg = std::min(window, max_steps - done);
    if (int rc = enqueue_steps(e, leg, s0 + done, w.active)) return rc;
    done += leg;
    const int s = s0 + done;
    // a check point: a whole leg, with a record entry one window back (step counts start at 1)
    const int check = (leg == window && s - window >= 1) ? 1 : 0;
    // enqueue_steps ended with its flush: the leg's reductions into av_sum and the force records are on the stream already
    hipLaunchKernelGGL(dens_steady_check, mgrid, mblock, 0, e->q.st, w, n, drag_rec ? drag_rec : (const double *)e->av_sum,
                       (unsigned long long)e->max_iters, drag_rec ? (const double *)nullptr : (const double *)e->steady_inv, s, window,
                       rel_tol, check, e->cur);
    HIP_TRY(hipGetLastError());
    // Every few checks: is anyone left?  Only how much is enqueued depends on the answer; what a member computes does not,
    // the workgroups of a stopped member return at once.
    if (check && ++checks % kSteadyPollChecks == 0 && done < max_steps) {
      HIP_TRY(hipMemcpyAsync(e->steady_count_host, w.count, sizeof(int), hipMemcpyDeviceToHost, e->q.st));
      HIP_TRY(hipStreamSynchronize(e->q.st));
      if (*e->steady_count_host == 0) break;
    }
  }
  if (int rc = steady_read_back(e->q, w.par, n, e->m_steps, e->m_conv, &e->steps_done, &e->ragged, &e->cur)) return rc;
  // the scalar's arrays in the order of the flow's: a member's scalar lies where its flow parity and the run's offset say
  e->scalar_off = scalar_off;
  if (e->scalar.on && !e->ragged) e->scalar.cur = e->cur ^ scalar_off;
  return LBM_OK;
}

// where a ragged ensemble's scalars lie and where their output is staged (dp_host.h); a default place while it is not ragged
int scalar_place(lbm_dens *e, ScalarPlace *at) {
  *at = ScalarPlace{};
  if (!e->ragged) return LBM_OK;
  if (!e->scalar_stage)
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->scalar_stage), (size_t)e->n * 5 * e->nx * e->ny * sizeof(double)));
  at->par = steady_words(e).par;
  at->off = e->scalar_off;
  at->stage = e->scalar_stage;
  return LBM_OK;
}

// Where downloads and the output stage put their results on the device: the grid array that is not current is scratch
// between runs; a ragged ensemble has no scratch array (both hold members' states) and gets a staging array of its own
int stage_of(lbm_dens *e, double **stage) {
  *stage = e->cells[e->cur ^ 1];
  if (!e->ragged) return LBM_OK;
  if (!e->stage) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->stage), (size_t)e->n * 9 * e->nx * e->ny * sizeof(double)));
  *stage = e->stage;
  return LBM_OK;
}

// the output stage of all members, each from the array that holds it, into `d[0..3]` (any may be NULL) and the per-block
// sums of u
int final_fields_dens(lbm_dens *e, double *const (&d)[4]) {
  // buoyancy: the half-force of the scalar state that is current, per cell; while the ensemble is ragged each member's scalar
  // from the array that holds it, the scalar's two arrays in the order of the flow's
  const bool buoy = e->scalar.on && e->buoy.on;
  if (buoy)
    if (int rc = buoy_sync(e->buoy, e->flow, flow_grid(e))) return rc;
  hipLaunchKernelGGL(dp_final_fields, dim3(e->fin_blocks, e->n), dim3(kBlock), 0, e->q.st,
                     (const double *)e->cells[e->ragged ? 0 : e->cur], (const double *)e->cells[1], member_parity(e), e->plane_stride,
                     e->member_stride, e->nx, (const uint8_t *)e->mask, (size_t)e->nx * e->ny, (const DpMember *)e->members,
                     drive_dev(e),
                     buoy ? (const double *)e->scalar.g[e->ragged ? e->scalar_off : e->scalar.cur] : (const double *)nullptr,
                     buoy ? (const double *)e->scalar.g[e->ragged ? e->scalar_off ^ 1 : e->scalar.cur ^ 1] : (const double *)nullptr,
                     buoy ? (const DpBuoyMember *)e->buoy.table : (const DpBuoyMember *)nullptr, d[0], d[1], d[2], d[3], e->fin_partials);
  HIP_TRY(hipGetLastError());
  return LBM_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

int lbm_dens_create(lbm_dens **out, const lbm_dparams *params, const int32_t *obstacles, int n) {
  // every argument error is reported before a device is touched
  if (!out) return lbm_fail(LBM_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (!params) return lbm_fail(LBM_ERR_ARG, "params is NULL");
  if (!obstacles) return lbm_fail(LBM_ERR_ARG, "obstacles is NULL");
  if (n < 1 || n > kDensMaxMembers) return lbm_fail(LBM_ERR_ARG, "an ensemble has 1 to %d members (got %d)", kDensMaxMembers, n);
  const lbm_dparams &p0 = params[0];
  if (p0.nx < 3 || p0.ny < 3) return lbm_fail(LBM_ERR_ARG, "grid must be at least 3x3 (got %dx%d)", p0.nx, p0.ny);
  if (p0.max_iters < 1) return lbm_fail(LBM_ERR_ARG, "max_iters must be >= 1 (got %d)", p0.max_iters);
  if (int rc = check_members_alike(params, n)) return rc;
  for (int i = 0; i < n; i++) {
    const lbm_dparams &p = params[i];
    if (!positive_finite(p.omega)) return lbm_fail(LBM_ERR_ARG, "member %d: omega must be finite and positive (got %g)", i, p.omega);
    if (!positive_finite(p.density))
      return lbm_fail(LBM_ERR_ARG, "member %d: density must be finite and positive (got %g)", i, p.density);
    if (!std::isfinite(p.accel)) return lbm_fail(LBM_ERR_ARG, "member %d: accel must be finite (got %g)", i, p.accel);
  }
  if ((long)p0.nx * p0.ny > kDensMaxCells)
    return lbm_fail(LBM_ERR_ARG, "a member of %dx%d cells is not launch-bound (the ensemble path takes members of at most %ld cells): "
                    "use double-precision contexts (lbm_dp_create)", p0.nx, p0.ny, kDensMaxCells);
  int ndev_visible = 0;
  HIP_TRY(hipGetDeviceCount(&ndev_visible));
  if (ndev_visible < 1) return lbm_fail(LBM_ERR_HIP, "no HIP device visible");

  lbm_dens *e = new lbm_dens();
  e->n = n;
  e->nx = p0.nx;
  e->ny = p0.ny;
  e->max_iters = p0.max_iters;
  e->p.assign(params, params + n);
  if (int rc = build_dens(e, obstacles)) {
    const std::string keep = lbm_last_error();
    free_dens(e);
    return fail_again(rc, keep);
  }
  *out = e;
  return LBM_OK;
}

int lbm_dens_upload(lbm_dens *e, const double *cells) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = queue_sync(e->q)) return rc;
  const size_t per = (size_t)e->nx * e->ny;
  const dim3 grid((unsigned)std::min(div_up((long)per, 256), 1024L), e->n);
  if (cells) {
    // one transfer of the caller's double[n][9][ny][nx] into the second grid array (9 nx ny <= member_stride), then one
    // launch that scatters every member's planes into the first (d2q9-bgk.c:200-203 for all members)
    HIP_TRY(hipMemcpyAsync(e->cells[1], cells, (size_t)e->n * 9 * per * sizeof(double), hipMemcpyHostToDevice, e->q.st));
    hipLaunchKernelGGL(dp_pack_planes<true>, grid, dim3(256), 0, e->q.st, e->cells[0], (double *)nullptr, (const int *)nullptr,
                       e->plane_stride, e->member_stride, e->nx, per, e->cells[1]);
  } else {
    hipLaunchKernelGGL(dp_init_cells, grid, dim3(256), 0, e->q.st, e->cells[0], e->plane_stride, e->member_stride,
                       (const DpMember *)e->members, e->nx, per);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->q.st));
  // the scalar survives an upload of the flow: after a ragged run every member's state comes onto one array, unchanged
  if (e->ragged && e->scalar.on)
    if (int rc = scalar_gather(e->scalar, scalar_grid(e), e->q.st, steady_words(e).par, e->scalar_off)) return rc;
  e->cur = 0;
  e->steps_done = 0;
  e->ring_fill = 0;
  e->ragged = false;
  e->m_steps.clear();
  e->m_conv.clear();
  // the statistics keep their setting and start anew
  return stats_restart(e->stats, scalar_grid(e), e->q.st, e->steps_done);
}

int lbm_dens_run(lbm_dens *e, int nsteps) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  return run_dens(e, nsteps, false, nullptr);
}

int lbm_dens_run_timed(lbm_dens *e, int nsteps, double *ms) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  return run_dens(e, nsteps, true, ms);
}

int lbm_dens_sync(lbm_dens *e) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  return queue_sync(e->q);
}

int lbm_dens_steps_done(const lbm_dens *e) { return e ? e->steps_done : -1; }
int lbm_dens_members(const lbm_dens *e) { return e ? e->n : -1; }

int lbm_dens_download(lbm_dens *e, double *cells_out, double *av_vels_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = queue_sync(e->q)) return rc;
  const size_t per = (size_t)e->nx * e->ny;
  if (cells_out) {
    // repack every member, from the array that holds it, into the caller's layout in the staging array, then one
    // contiguous transfer
    double *stage = nullptr;
    if (int rc = stage_of(e, &stage)) return rc;
    hipLaunchKernelGGL(dp_pack_planes<false>, dim3((unsigned)std::min(div_up((long)per, 256), 1024L), e->n), dim3(256), 0, e->q.st,
                       e->cells[e->ragged ? 0 : e->cur], e->cells[1], member_parity(e), e->plane_stride, e->member_stride, e->nx,
                       per, stage);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cells_out, stage, (size_t)e->n * 9 * per * sizeof(double), hipMemcpyDeviceToHost, e->q.st));
    HIP_TRY(hipStreamSynchronize(e->q.st));
  }
  if (av_vels_out && e->steps_done > 0) {
    const int T = e->steps_done;
    std::vector<double> sums((size_t)e->n * T);
    HIP_TRY(hipMemcpy2D(sums.data(), (size_t)T * sizeof(double), e->av_sum, (size_t)e->max_iters * sizeof(double),
                        (size_t)T * sizeof(double), e->n, hipMemcpyDeviceToHost));
    // kernels.cl:202: sum * FREE_CELLS_INV, the member's own, in double
    for (int m = 0; m < e->n; m++)
      for (int t = 0; t < T; t++) av_vels_out[(size_t)m * T + t] = sums[(size_t)m * T + t] * e->p[m].free_cells_inv;
    // a member that stopped earlier has no record from its own count on
    if (e->ragged)
      for (int m = 0; m < e->n; m++)
        for (int t = e->m_steps[m]; t < T; t++) av_vels_out[(size_t)m * T + t] = 0.0;
  }
  return LBM_OK;
}

int lbm_dens_final_state(lbm_dens *e, double *u_x, double *u_y, double *u, double *pressure) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = queue_sync(e->q)) return rc;
  const size_t all = (size_t)e->nx * e->ny * e->n;
  double *outs[4] = {u_x, u_y, u, pressure};
  // the four columns of all members go to the staging array (4 n nx ny doubles of its 9 n nx ny)
  double *d[4] = {nullptr, nullptr, nullptr, nullptr};
  double *stage = nullptr;
  if (int rc = stage_of(e, &stage)) return rc;
  for (int i = 0; i < 4; i++)
    if (outs[i]) d[i] = stage + (size_t)i * all;
  if (int rc = final_fields_dens(e, d)) return rc;
  for (int i = 0; i < 4; i++)
    if (outs[i]) HIP_TRY(hipMemcpyAsync(outs[i], d[i], all * sizeof(double), hipMemcpyDeviceToHost, e->q.st));
  HIP_TRY(hipStreamSynchronize(e->q.st));
  return LBM_OK;
}

int lbm_dens_reynolds(lbm_dens *e, double *reynolds_out) {
  if (!e || !reynolds_out) return lbm_fail(LBM_ERR_ARG, "NULL argument");
  if (int rc = queue_sync(e->q)) return rc;
  double *none[4] = {nullptr, nullptr, nullptr, nullptr};
  if (int rc = final_fields_dens(e, none)) return rc;
  std::vector<double> part((size_t)e->n * e->fin_blocks);
  HIP_TRY(hipMemcpyAsync(part.data(), e->fin_partials, part.size() * sizeof(double), hipMemcpyDeviceToHost, e->q.st));
  HIP_TRY(hipStreamSynchronize(e->q.st));
  for (int m = 0; m < e->n; m++) {
    double tot = 0.0;
    for (int b = 0; b < e->fin_blocks; b++) tot += part[(size_t)m * e->fin_blocks + b];
    // av_velocity + calc_reynolds, d2q9-bgk.c:396-442, 747-752, in double (the statements of lbm_dp_reynolds)
    const lbm_dparams &p = e->p[m];
    const double viscosity = 1.0 / 6.0 * (2.0 / p.omega - 1.0);
    reynolds_out[m] = tot * p.free_cells_inv * (double)p.reynolds_dim / viscosity;
  }
  return LBM_OK;
}

int lbm_dsteady_run(lbm_dens *e, int max_steps, int window, double rel_tol) {
  // every argument error is reported before the ensemble or a device is touched
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = check_steady_args(max_steps, window, rel_tol)) return rc;
  if (e->stats.every) return stats_refuse_steady("lbm_dsteady_run");
  if (e->scalar.on) return refuse_steady_scalar("lbm_dsteady_run");
  bool launched = false;
  const int rc = steady_impl(e, max_steps, window, rel_tol, nullptr, &launched);
  return latch_failure(rc, launched, e->q.st, &e->failed);
}

int lbm_dsteady_steps(lbm_dens *e, int *steps_out, int *converged_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  steady_steps_out(e->n, e->ragged, e->steps_done, e->m_steps, e->m_conv, steps_out, converged_out);
  return LBM_OK;
}

int lbm_dforce_ens_set_option(lbm_dens *e, const char *key, long value) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!key) return lbm_fail(LBM_ERR_ARG, "key is NULL");
  if (strcmp(key, "force")) return lbm_fail(LBM_ERR_ARG, "unknown option '%s' (a double-precision ensemble has \"force\")", key);
  if (int rc = force_check(value)) return rc;
  return force_set(e->flow, flow_grid(e), value, true, e->force_rec, e->failed);
}

int lbm_dforce_ens_get_option(const lbm_dens *e, const char *key, long *value) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!key) return lbm_fail(LBM_ERR_ARG, "key is NULL");
  if (!value) return lbm_fail(LBM_ERR_ARG, "value is NULL");
  if (strcmp(key, "force")) return lbm_fail(LBM_ERR_ARG, "unknown option '%s' (a double-precision ensemble has \"force\")", key);
  *value = e->flow.force ? 1 : 0;
  return LBM_OK;
}

int lbm_dforce_ens_record(lbm_dens *e, double *fx_out, double *fy_out) {
  // argument errors before a device is touched
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!fx_out && !fy_out) return lbm_fail(LBM_ERR_ARG, "fx_out and fy_out are both NULL");
  if (!e->flow.force)
    return lbm_fail(LBM_ERR_STATE, "no force record: option \"force\" is off (lbm_dforce_ens_set_option before the first step)");
  if (int rc = queue_sync(e->q)) return rc;
  const int T = e->steps_done;
  double *outs[2] = {fx_out, fy_out};
  for (int c = 0; c < 2; c++) {
    if (!outs[c] || T == 0) continue;
    HIP_TRY(hipMemcpy2D(outs[c], (size_t)T * sizeof(double), e->force_rec + (size_t)c * e->n * e->max_iters,
                        (size_t)e->max_iters * sizeof(double), (size_t)T * sizeof(double), e->n, hipMemcpyDeviceToHost));
    // a member that stopped earlier has no record from its own count on (lbm_dens_download's av_vels)
    if (e->ragged)
      for (int m = 0; m < e->n; m++)
        for (int t = e->m_steps[m]; t < T; t++) outs[c][(size_t)m * T + t] = 0.0;
  }
  return LBM_OK;
}

int lbm_dforce_ens(lbm_dens *e, double *fx, double *fy) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!fx && !fy) return lbm_fail(LBM_ERR_ARG, "fx and fy are both NULL");
  if (int rc = queue_sync(e->q)) return rc;
  const size_t n = (size_t)e->n;
  if (!e->force_now) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->force_now), 2 * n * sizeof(double)));
  // each member from the array that holds it
  DpForceArgs a{};
  a.cells = e->cells[e->ragged ? 0 : e->cur];
  a.cells_alt = e->cells[1];
  a.par = member_parity(e);
  a.mask = e->mask;
  a.members = e->members;
  a.plane_stride = e->plane_stride;
  a.member_stride = e->member_stride;
  a.nx = e->nx;
  a.ny = e->ny;
  a.no_accel = e->flow.open ? 1 : 0;
  if (int rc = force_state(e->q.st, a, e->nseg, e->n, e->seg, e->red, e->red_blocks, e->force_now)) return rc;
  std::vector<double> f(2 * n);
  HIP_TRY(hipMemcpyAsync(f.data(), e->force_now, f.size() * sizeof(double), hipMemcpyDeviceToHost, e->q.st));
  HIP_TRY(hipStreamSynchronize(e->q.st));
  for (size_t m = 0; m < n; m++) {
    if (fx) fx[m] = f[m];
    if (fy) fy[m] = f[n + m];
  }
  return LBM_OK;
}

int lbm_dbody_ens_set(lbm_dens *e, const int32_t *body) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (e->flow.force && e->steps_done != 0)
    return lbm_fail(LBM_ERR_STATE, "with \"force\" on, a body map is set before the first step (%d done): one record holds one body",
                    e->steps_done);
  if (int rc = queue_sync(e->q)) return rc;
  return body_apply(e->body, e->mask, body, e->n, e->ny, e->nx, true, e->flow.open);
}

int lbm_dbody_ens_get(lbm_dens *e, int32_t *body_out) {
  // argument errors before anything of the ensemble is read
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!body_out) return lbm_fail(LBM_ERR_ARG, "body_out is NULL");
  body_read(e->body, body_out);
  return LBM_OK;
}

int lbm_dbody_steady_run(lbm_dens *e, int max_steps, int window, double rel_tol) {
  // every argument error is reported before the ensemble or a device is touched
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = check_steady_args(max_steps, window, rel_tol)) return rc;
  if (e->stats.every) return stats_refuse_steady("lbm_dbody_steady_run");
  if (e->scalar.on) return refuse_steady_scalar("lbm_dbody_steady_run");
  if (!e->flow.force)
    return lbm_fail(LBM_ERR_STATE, "the drag criterion reads the force record: option \"force\" is off (lbm_dforce_ens_set_option "
                    "switches it on before the first step)");
  bool launched = false;
  const int rc = steady_impl(e, max_steps, window, rel_tol, e->force_rec, &launched);
  return latch_failure(rc, launched, e->q.st, &e->failed);
}

// The six setters: the NULL checks, the check of every member's values (dp_host.h), then the set.
int lbm_dtrt_ens_set(lbm_dens *e, const double *magic) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = trt_check(e->p.data(), e->n, magic, true)) return rc;
  return trt_set(e->flow, flow_grid(e), magic);
}

int lbm_dtrt_ens_get(const lbm_dens *e, double *magic_out, double *omega_minus_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!magic_out && !omega_minus_out) return lbm_fail(LBM_ERR_ARG, "magic_out and omega_minus_out are both NULL");
  trt_get(e->flow, magic_out, omega_minus_out);
  return LBM_OK;
}

int lbm_dopen_ens_set(lbm_dens *e, const double *u_in, const double *rho_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (u_in && !rho_out) return lbm_fail(LBM_ERR_ARG, "rho_out is NULL (u_in is not: every member needs its outlet density)");
  if (int rc = open_check(e->p.data(), e->n, u_in, rho_out, true)) return rc;
  return open_set(e->flow, flow_grid(e), e->body, e->mask, u_in, rho_out);
}

int lbm_dopen_ens_get(const lbm_dens *e, int *on_out, double *u_in_out, double *rho_out_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!on_out && !u_in_out && !rho_out_out) return lbm_fail(LBM_ERR_ARG, "on_out, u_in_out and rho_out_out are all NULL");
  open_get(e->flow, e->n, e->ny, on_out, u_in_out, rho_out_out);
  return LBM_OK;
}

int lbm_dwall_ens_set(lbm_dens *e, const double *u_x, const double *u_y, const double *rho_wall) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if ((u_x == nullptr) != (u_y == nullptr))
    return lbm_fail(LBM_ERR_ARG, "%s is NULL and %s is not: a wall velocity has two components (both NULL: off)", u_x ? "u_y" : "u_x",
                    u_x ? "u_x" : "u_y");
  if (u_x && !rho_wall) return lbm_fail(LBM_ERR_ARG, "rho_wall is NULL (u_x is not: every member needs its wall density)");
  if (int rc = wall_values_check(e->body, e->p.data(), e->n, u_x, u_y, rho_wall, true)) return rc;
  return wall_set(e->flow, flow_grid(e), u_x, u_y, rho_wall);
}

int lbm_dwall_ens_get(const lbm_dens *e, int *on_out, double *u_x_out, double *u_y_out, double *rho_wall_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!on_out && !u_x_out && !u_y_out && !rho_wall_out)
    return lbm_fail(LBM_ERR_ARG, "on_out, u_x_out, u_y_out and rho_wall_out are all NULL");
  wall_get(e->flow, on_out, u_x_out, u_y_out, rho_wall_out);
  return LBM_OK;
}

int lbm_dles_ens_set(lbm_dens *e, const double *c) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = les_check(e->n, c, true)) return rc;
  return les_set(e->flow, flow_grid(e), c);
}

int lbm_dles_ens_get(const lbm_dens *e, double *c_out, double *les_k_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!c_out && !les_k_out) return lbm_fail(LBM_ERR_ARG, "c_out and les_k_out are both NULL");
  les_get(e->flow, e->p.data(), e->n, c_out, les_k_out);
  return LBM_OK;
}

int lbm_ddrive_ens_set(lbm_dens *e, const double *f) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = drive_check(e->n, f, true)) return rc;
  return drive_set(e->flow, flow_grid(e), f);
}

int lbm_ddrive_ens_get(const lbm_dens *e, int *on_out, double *f_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!on_out && !f_out) return lbm_fail(LBM_ERR_ARG, "on_out and f_out are both NULL");
  drive_get(e->flow, on_out, f_out);
  return LBM_OK;
}

int lbm_dscalar_ens_set(lbm_dens *e, const double *diffusivity, const double *c0, const double *c_wall, const double *c_in) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (diffusivity && !c0) return lbm_fail(LBM_ERR_ARG, "c0 is NULL (diffusivity is not: a scalar starts from a field)");
  // every member is checked before anything changes, on the host or on the device
  const ScalarGrid gr = scalar_grid(e);
  if (diffusivity)
    if (int rc = scalar_check(gr, true, diffusivity, c0, c_wall, c_in)) return rc;
  if (diffusivity && e->ragged) return refuse_ragged(e);
  if (!diffusivity && e->buoy.on) return buoy_refuse_scalar_off();
  if (!diffusivity && e->scalar.on && e->scalar.record) return scalar_record_refuse_scalar_off();
  if (int rc = queue_sync(e->q)) return rc;
  if (!diffusivity) return scalar_off(e->scalar);
  return scalar_set(e->scalar, gr, e->q.st, diffusivity, c0, c_wall, c_in, drive_dev(e));
}

int lbm_dscalar_ens_get(const lbm_dens *e, int *on_out, double *diffusivity_out, double *omega_s_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!on_out && !diffusivity_out && !omega_s_out)
    return lbm_fail(LBM_ERR_ARG, "on_out, diffusivity_out and omega_s_out are all NULL");
  if (on_out) *on_out = e->scalar.on ? 1 : 0;
  for (int m = 0; m < e->n; m++) {
    if (diffusivity_out) diffusivity_out[m] = e->scalar.on ? e->scalar.diffusivity[m] : 0.0;
    if (omega_s_out) omega_s_out[m] = e->scalar.on ? e->scalar.omega_s[m] : 0.0;
  }
  return LBM_OK;
}

int lbm_dscalar_ens_field(lbm_dens *e, double *c_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!c_out) return lbm_fail(LBM_ERR_ARG, "c_out is NULL");
  if (!e->scalar.on) return scalar_refuse_off("lbm_dscalar_ens_field");
  if (int rc = queue_sync(e->q)) return rc;
  ScalarPlace at;
  if (int rc = scalar_place(e, &at)) return rc;
  return scalar_field(e->scalar, scalar_grid(e), e->q.st, e->mask, c_out, at);
}

int lbm_dscalar_ens_download(lbm_dens *e, double *g_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!g_out) return lbm_fail(LBM_ERR_ARG, "g_out is NULL");
  if (!e->scalar.on) return scalar_refuse_off("lbm_dscalar_ens_download");
  if (int rc = queue_sync(e->q)) return rc;
  ScalarPlace at;
  if (int rc = scalar_place(e, &at)) return rc;
  return scalar_download(e->scalar, scalar_grid(e), e->q.st, g_out, at);
}

int lbm_dscalar_ens_upload(lbm_dens *e, const double *g) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!g) return lbm_fail(LBM_ERR_ARG, "g is NULL");
  if (!e->scalar.on) return scalar_refuse_off("lbm_dscalar_ens_upload");
  if (e->ragged) return refuse_ragged(e);
  if (int rc = queue_sync(e->q)) return rc;
  return scalar_upload(e->scalar, scalar_grid(e), e->q.st, g);
}

int lbm_drecord_ens_set(lbm_dens *e, int on) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = scalar_record_check(e->scalar, on, e->steps_done, true)) return rc;
  if (int rc = queue_sync(e->q)) return rc;
  HIP_TRY(hipSetDevice(e->q.dev));
  return scalar_record_set(e->scalar, scalar_grid(e), on);
}

int lbm_drecord_ens_get(const lbm_dens *e, int *on_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!on_out) return lbm_fail(LBM_ERR_ARG, "on_out is NULL");
  *on_out = e->scalar.on && e->scalar.record ? 1 : 0;
  return LBM_OK;
}

int lbm_drecord_ens(lbm_dens *e, double *content_out, double *flux_x_out, double *flux_y_out) {
  // argument errors before a device is touched
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!content_out && !flux_x_out && !flux_y_out) return lbm_fail(LBM_ERR_ARG, "content_out, flux_x_out and flux_y_out are all NULL");
  if (!e->scalar.on || !e->scalar.record) return scalar_record_refuse_off("lbm_drecord_ens", true);
  if (int rc = queue_sync(e->q)) return rc;
  double *const outs[3] = {content_out, flux_x_out, flux_y_out};
  return scalar_record_read(e->scalar, scalar_grid(e), e->steps_done, e->ragged ? e->m_steps.data() : nullptr, outs);
}

int lbm_drecord_steady_run(lbm_dens *e, int max_steps, int window, double rel_tol, int which) {
  // every argument error is reported before the ensemble or a device is touched
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = check_steady_args(max_steps, window, rel_tol)) return rc;
  if (which < 0 || which > 2) return lbm_fail(LBM_ERR_ARG, "which must be 0 (content), 1 (flux_x) or 2 (flux_y) (got %d)", which);
  if (e->stats.every) return stats_refuse_steady("lbm_drecord_steady_run");
  if (!e->scalar.on || !e->scalar.record)
    return lbm_fail(LBM_ERR_ARG, "the scalar criterion reads the scalar's record: it is off (lbm_dscalar_ens_set, then "
                    "lbm_drecord_ens_set before the first step)");
  bool launched = false;
  const int rc = steady_impl(e, max_steps, window, rel_tol, e->scalar.rec + (size_t)which * e->n * e->max_iters, &launched);
  return latch_failure(rc, launched, e->q.st, &e->failed);
}

int lbm_dbuoy_ens_set(lbm_dens *e, const double *b) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  // every member is checked before anything changes, on the host or on the device
  if (b)
    if (int rc = buoy_check_values(b, e->n, true)) return rc;
  if (int rc = buoy_check_state(e->scalar, e->steps_done, b != nullptr)) return rc;
  if (int rc = queue_sync(e->q)) return rc;
  HIP_TRY(hipSetDevice(e->q.dev));
  return buoy_set(e->buoy, b, e->n);
}

int lbm_dbuoy_ens_get(const lbm_dens *e, int *on_out, double *b_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!on_out && !b_out) return lbm_fail(LBM_ERR_ARG, "on_out and b_out are both NULL");
  if (on_out) *on_out = e->buoy.on ? 1 : 0;
  if (b_out) {
    if (e->buoy.on) std::copy(e->buoy.b.begin(), e->buoy.b.end(), b_out);
    else std::fill(b_out, b_out + 3 * (size_t)e->n, 0.0);
  }
  return LBM_OK;
}

int lbm_dstats_ens_set(lbm_dens *e, int every) {
  // argument errors before anything of the ensemble is read
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = stats_check(every)) return rc;
  if (every && e->ragged) return refuse_ragged(e);
  if (int rc = queue_sync(e->q)) return rc;
  return stats_set(e->stats, scalar_grid(e), e->q.st, every, e->steps_done);
}

int lbm_dstats_ens_get(const lbm_dens *e, int *every_out, int *origin_out, int *samples_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!every_out && !origin_out && !samples_out) return lbm_fail(LBM_ERR_ARG, "every_out, origin_out and samples_out are all NULL");
  stats_get(e->stats, every_out, origin_out, samples_out);
  return LBM_OK;
}

int lbm_dstats_ens(lbm_dens *e, double *sums_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (!sums_out) return lbm_fail(LBM_ERR_ARG, "sums_out is NULL");
  if (!e->stats.every) return stats_refuse_off("lbm_dstats_ens", true);
  if (int rc = queue_sync(e->q)) return rc;
  return stats_read(e->stats, scalar_grid(e), sums_out);
}

void lbm_dens_destroy(lbm_dens *e) {
  if (!e) return;
  (void)hipSetDevice(e->q.dev);
  free_dens(e);
}

}  // extern "C"

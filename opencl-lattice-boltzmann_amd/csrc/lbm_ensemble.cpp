// Third translation unit of liblbm_hip.so: the host side of the ensemble entry points (include/lbm.h: lbm_ens_*).
//
// An ensemble is N independent grids of one size on one device, each with its own run constants, obstacle map and
// state.  All members live in one pair of arrays (member m at m * member_stride in the layout of an ordinary context:
// row-interleaved planes padded to 256-B lines), one mask array and one table of per-member constants; every entry
// point is one launch (or one transfer) for all members.  The step loop is the KIND_MULTI case of lbm_hip.cpp reduced to
// one slab: a prologue accelerate_flow, launches of up to 8 steps of d2q9_ensemble with the next step's acceleration
// fused into all but the last, a ring of buffered per-step partial sums flushed by the batched second reduction stage.
// The reference has no counterpart: one grid, one in-order queue (d2q9-bgk.c:221-239).
//
// A steady run (lbm_steady_*) is the same loop cut into legs of `window` steps behind a per-member `active` word that a
// criterion kernel clears on the device (steady_kernels.h).  Members may then stop on different launch parities, so from
// the end of such a run until the next upload the array that holds a member's state is the member's own (`par`).
#include "../../include/lbm.h"
#include "steady_kernels.h"
#include "host_common.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace lbm;
using namespace lbm_host;

namespace {

constexpr int kEnsRingMax = 256;           // most steps of per-tile partial sums buffered between reductions
constexpr long kEnsMaxCells = 300L * 1024; // the library's bound for "launch-bound" (multistep_effective, lbm_hip.cpp)
constexpr int kEnsMaxMembers = 65535;      // member index = blockIdx.y

}  // namespace

struct lbm_ens {
  int n = 0;
  int nx = 0, ny = 0, max_iters = 0;
  std::vector<lbm_params> p;
  Queue q;
  int cus = 256;
  size_t plane_stride = 0, member_stride = 0;  // floats
  float *cells[2] = {nullptr, nullptr};
  uint8_t *mask = nullptr;       // [n][ny][nx]
  EnsMember *members = nullptr;  // [n]
  float *partials = nullptr;     // [ring][n][tiles]
  double *av_sum = nullptr;      // [n][max(1, max_iters)]
  float *fin_partials = nullptr; // [n][fin_blocks]
  int fin_blocks = 1;
  int tx = 16, ty = 16, tiles_x = 1, tiles = 1;
  int ring = 8, ring_fill = 0;
  int cur = 0, steps_done = 0;
  bool failed = false;
  // steady runs (allocated by the first lbm_steady_run)
  int *steady_words = nullptr;       // device: active[n], par[n], steps[n], conv[n], count
  float *steady_inv = nullptr;       // device: free_cells_inv[n]
  int *steady_count_host = nullptr;  // page-locked: where the count of active members is read back to
  float *stage = nullptr;            // device, float[n][9][ny][nx]: staging of downloads while the ensemble is ragged
  std::vector<int> m_steps, m_conv;  // host copies of the words after the last steady run (empty: none since the upload)
  bool ragged = false;               // members stopped at different step counts: download and output only, until an upload
};

namespace {

void free_ens(lbm_ens *e) {
  queue_drain(e->q);
  for (float *c : e->cells)
    if (c) (void)hipFree(c);
  if (e->mask) (void)hipFree(e->mask);
  if (e->members) (void)hipFree(e->members);
  if (e->partials) (void)hipFree(e->partials);
  if (e->av_sum) (void)hipFree(e->av_sum);
  if (e->fin_partials) (void)hipFree(e->fin_partials);
  if (e->steady_words) (void)hipFree(e->steady_words);
  if (e->steady_inv) (void)hipFree(e->steady_inv);
  if (e->steady_count_host) (void)hipHostFree(e->steady_count_host);
  if (e->stage) (void)hipFree(e->stage);
  queue_destroy(e->q);
  delete e;
}

int build_ens(lbm_ens *e, const int32_t *obstacles) {
  const int n = e->n, nx = e->nx, ny = e->ny;
  const size_t cells_per = (size_t)nx * ny;
  HIP_TRY(hipGetDevice(&e->q.dev));
  {
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->q.dev));
    if (cus > 0) e->cus = cus;
  }
  // Tile shape.  d2q9_multi's cost model (lbm_hip.cpp, slab_geometry: ceil(tiles / CUs) x cell updates per tile) holds while
  // every tile has a CU to itself: there the smallest tile wins (one grid, us/step for 32x16 / 16x16 / 16x8: 128x128 1.85 /
  // 1.55 / 1.38).  An ensemble soon has several rounds of tiles per CU, and then the workgroups that fit a CU together
  // decide: two of 16x16 (75 KB of LDS each, 50 VGPRs) or of 16x8 overlap one's loads and stores with the other's sub-steps,
  // one of 32x16 (113 KB) cannot.  Measured (tools/ensemble_ab.py, us/step 32x16 / 16x16 / 16x8): 64 x 128x128 15.05 / 13.26 /
  // 21.50, 16 x 256x256 13.45 / 13.07 / 21.33 - so 16x8 while its tiles fit one per CU, 16x16 from there on, and no 32x16 form.
  {
    const long tiles_16x8 = (long)n * div_up(nx, 16) * div_up(ny, 8);
    e->tx = 16;
    e->ty = tiles_16x8 <= e->cus ? 8 : 16;
  }
  e->tiles_x = (int)div_up(nx, e->tx);
  e->tiles = e->tiles_x * (int)div_up(ny, e->ty);
  e->plane_stride = ((size_t)(nx + 63) / 64) * 64;
  e->member_stride = 9 * e->plane_stride * ny;
  e->fin_blocks = (int)std::max(1L, std::min(div_up((long)cells_per, kBlock), 2048L));
  // ring of per-step partial sums: at most 16 MiB, at least 8 steps (one launch)
  const size_t per_step = (size_t)n * e->tiles;
  e->ring = (int)std::max<size_t>(kMultiMaxT, std::min<size_t>(kEnsRingMax, ((size_t)4 << 20) / per_step));

  // what the ensemble needs against what the device has free: refuse here rather than fail half-way through
  const size_t cells_bytes = ((size_t)n * e->member_stride + 64) * sizeof(float);
  const size_t need = 2 * cells_bytes + (size_t)n * cells_per + (size_t)n * sizeof(EnsMember) +
                      (size_t)e->ring * per_step * sizeof(float) + (size_t)n * std::max(1, e->max_iters) * sizeof(double) +
                      (size_t)n * e->fin_blocks * sizeof(float);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b)
    return lbm_fail(LBM_ERR_HIP, "an ensemble of %d members of %dx%d with max_iters=%d needs %.1f MiB of device memory, %.1f MiB are free",
                    n, nx, ny, e->max_iters, (double)need / 1048576.0, (double)free_b / 1048576.0);

  if (int rc = queue_create(e->q)) return rc;
  for (int i = 0; i < 2; i++) {
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->cells[i]), cells_bytes));
    HIP_TRY(hipMemset(e->cells[i], 0, cells_bytes));
  }
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->mask), (size_t)n * cells_per + 64));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->members), (size_t)n * sizeof(EnsMember)));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->partials), (size_t)e->ring * per_step * sizeof(float)));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->av_sum), (size_t)n * std::max(1, e->max_iters) * sizeof(double)));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->fin_partials), (size_t)n * e->fin_blocks * sizeof(float)));
  // the members' byte masks from the caller's int32[n][ny][nx]
  if (int rc = upload_mask(e->mask, obstacles, (size_t)n * cells_per)) return rc;
  std::vector<EnsMember> t(n);
  for (int i = 0; i < n; i++) t[i] = member_constants<EnsMember>(e->p[i]);
  HIP_TRY(hipMemcpy(e->members, t.data(), t.size() * sizeof(EnsMember), hipMemcpyHostToDevice));
  return LBM_OK;
}

// active: NULL for an ordinary run, the members' words for a leg of a steady run
void launch_ensemble(const lbm_ens *e, const EnsArgs &a, const int *active) {
  const dim3 grid(e->tiles, e->n), block(kMultiThreads);
  if (!active) {
    if (e->ty == 16) hipLaunchKernelGGL((d2q9_ensemble<16, 16>), grid, block, 0, e->q.st, a);
    else hipLaunchKernelGGL((d2q9_ensemble<16, 8>), grid, block, 0, e->q.st, a);
  } else {
    if (e->ty == 16) hipLaunchKernelGGL((d2q9_ensemble_gated<16, 16>), grid, block, 0, e->q.st, a, active);
    else hipLaunchKernelGGL((d2q9_ensemble_gated<16, 8>), grid, block, 0, e->q.st, a, active);
  }
}

// nsteps steps from step count `first` on, enqueued: the prologue, the launches, the reductions into the record.  Flips
// e->cur per launch; the caller counts the steps.  active: as launch_ensemble.
int enqueue_steps(lbm_ens *e, int nsteps, int first, const int *active) {
  // prologue: accelerate_flow of the first step on the current grids (kernels.cl:9-53); later steps get theirs fused
  // into the previous launch's write of row ny-2
  hipLaunchKernelGGL(ens_accelerate_row, dim3(div_up(e->nx, 128), e->n), dim3(128), 0, e->q.st, e->cells[e->cur], e->plane_stride,
                     e->member_stride, e->mask, e->members, e->nx, e->ny, active);
  HIP_TRY(hipGetLastError());

  int batch_first = first;
  // second reduction stage over the buffered steps (kernels.cl:234-290 counterpart)
  auto flush = [&]() -> int {
    if (e->ring_fill == 0) return LBM_OK;
    hipLaunchKernelGGL(ens_reduce_partials, dim3(e->n, e->ring_fill), dim3(kBlock), 0, e->q.st, e->partials, e->tiles, e->av_sum,
                       (unsigned long long)std::max(1, e->max_iters), batch_first, active);
    HIP_TRY(hipGetLastError());
    batch_first += e->ring_fill;
    e->ring_fill = 0;
    return LBM_OK;
  };
  int i = 0;
  while (i < nsteps) {
    // the remaining steps in as few launches as possible, of equal depth (20 steps = 7 + 7 + 6)
    const int rem = nsteps - i;
    const int adv = equal_depth(rem, kMultiMaxT);
    if (e->ring_fill + adv > e->ring)
      if (int rc = flush()) return rc;
    EnsArgs a{};
    a.src = e->cells[e->cur];
    a.dst = e->cells[e->cur ^ 1];
    a.mask = e->mask;
    a.members = e->members;
    a.partials = e->partials + (size_t)e->ring_fill * e->n * e->tiles;
    a.plane_stride = e->plane_stride;
    a.member_stride = e->member_stride;
    a.nx = e->nx;
    a.ny = e->ny;
    a.tiles_x = e->tiles_x;
    a.T = adv;
    a.accel_next = (i + adv < nsteps) ? 1 : 0;
    launch_ensemble(e, a, active);
    HIP_TRY(hipGetLastError());
    e->cur ^= 1;
    e->ring_fill += adv;
    i += adv;
  }
  return flush();
}

int refuse_ragged(const lbm_ens *e) {
  return lbm_fail(LBM_ERR_STATE, "the members of this ensemble stopped at different step counts (lbm_steady_run; %d is the "
                  "largest): download them, then lbm_ens_upload before the next run", e->steps_done);
}

int run_ens_impl(lbm_ens *e, int nsteps, bool timed, double *ms, bool *launched) {
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

int run_ens(lbm_ens *e, int nsteps, bool timed, double *ms) {
  bool launched = false;
  const int rc = run_ens_impl(e, nsteps, timed, ms, &launched);
  return latch_failure(rc, launched, e->q.st, &e->failed);
}

SteadyWords steady_words(const lbm_ens *e) { return steady_words_at(e->steady_words, (size_t)e->n); }

// which array holds member m, for the kernels that read a state: the members' own words while the ensemble is ragged
const int *member_parity(const lbm_ens *e) { return e->ragged ? steady_words(e).par : nullptr; }

// what a steady run needs beyond an ordinary one, allocated by the first
int steady_alloc(lbm_ens *e) {
  if (e->steady_words) return LBM_OK;
  const size_t n = (size_t)e->n;
  if (!e->steady_count_host)
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->steady_count_host), sizeof(int), hipHostMallocDefault));
  if (!e->steady_inv) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->steady_inv), n * sizeof(float)));
  std::vector<float> inv(n);
  for (size_t m = 0; m < n; m++) inv[m] = e->p[m].free_cells_inv;
  HIP_TRY(hipMemcpy(e->steady_inv, inv.data(), n * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->steady_words), (kSteadyWordCount * n + 1) * sizeof(int)));
  return LBM_OK;
}

int steady_impl(lbm_ens *e, int max_steps, int window, double rel_tol, bool *launched) {
  if (int rc = check_runnable(max_steps, e->failed, "ensemble")) return rc;  // max_steps >= 0 here (lbm_steady_run)
  if (e->ragged) return refuse_ragged(e);
  if (int rc = check_record(e->max_iters, e->steps_done, max_steps, "up to ")) return rc;
  if (max_steps == 0) return LBM_OK;
  HIP_TRY(hipSetDevice(e->q.dev));
  if (int rc = steady_alloc(e)) return rc;
  const int n = e->n, s0 = e->steps_done;
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
    hipLaunchKernelGGL(ens_steady_check, mgrid, mblock, 0, e->q.st, w, n, e->av_sum, (unsigned long long)std::max(1, e->max_iters),
                       e->steady_inv, s, window, rel_tol, check, e->cur);
    HIP_TRY(hipGetLastError());
    // Every few checks: is anyone left?  Only how much is enqueued depends on the answer; what a member computes does not,
    // the workgroups of a stopped member return at once.
    if (check && ++checks % kSteadyPollChecks == 0 && done < max_steps) {
      HIP_TRY(hipMemcpyAsync(e->steady_count_host, w.count, sizeof(int), hipMemcpyDeviceToHost, e->q.st));
      HIP_TRY(hipStreamSynchronize(e->q.st));
      if (*e->steady_count_host == 0) break;
    }
  }
  return steady_read_back(e->q, w.par, n, e->m_steps, e->m_conv, &e->steps_done, &e->ragged, &e->cur);
}

// the staging array of downloads while both grid arrays hold members' states
int stage_alloc(lbm_ens *e) {
  if (e->stage) return LBM_OK;
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->stage), (size_t)e->n * 9 * e->nx * e->ny * sizeof(float)));
  return LBM_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

int lbm_ens_create(lbm_ens **out, const lbm_params *params, const int32_t *obstacles, int n) {
  // every argument error is reported before a device is touched
  if (!out) return lbm_fail(LBM_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (!params) return lbm_fail(LBM_ERR_ARG, "params is NULL");
  if (!obstacles) return lbm_fail(LBM_ERR_ARG, "obstacles is NULL");
  if (n < 1 || n > kEnsMaxMembers) return lbm_fail(LBM_ERR_ARG, "an ensemble has 1 to %d members (got %d)", kEnsMaxMembers, n);
  const lbm_params &p0 = params[0];
  if (p0.nx < 3 || p0.ny < 3) return lbm_fail(LBM_ERR_ARG, "grid must be at least 3x3 (got %dx%d)", p0.nx, p0.ny);
  if (p0.max_iters < 0) return lbm_fail(LBM_ERR_ARG, "max_iters must be >= 0");
  if (int rc = check_members_alike(params, n)) return rc;
  if ((long)p0.nx * p0.ny > kEnsMaxCells)
    return lbm_fail(LBM_ERR_ARG, "a member of %dx%d cells is not launch-bound (the ensemble path takes members of at most %ld cells): "
                    "use ordinary contexts (lbm_create)", p0.nx, p0.ny, kEnsMaxCells);
  int ndev_visible = 0;
  HIP_TRY(hipGetDeviceCount(&ndev_visible));
  if (ndev_visible < 1) return lbm_fail(LBM_ERR_HIP, "no HIP device visible");

  lbm_ens *e = new lbm_ens();
  e->n = n;
  e->nx = p0.nx;
  e->ny = p0.ny;
  e->max_iters = p0.max_iters;
  e->p.assign(params, params + n);
  if (int rc = build_ens(e, obstacles)) {
    const std::string keep = lbm_last_error();
    free_ens(e);
    return fail_again(rc, keep);
  }
  *out = e;
  return LBM_OK;
}

int lbm_ens_upload(lbm_ens *e, const float *cells) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = queue_sync(e->q)) return rc;
  const size_t per = (size_t)e->nx * e->ny;
  const dim3 grid((unsigned)std::min(div_up((long)per, 256), 1024L), e->n);
  if (cells) {
    // one transfer of the caller's float[n][9][ny][nx] into the second grid array (9 nx ny <= member_stride), then one
    // launch that scatters every member's planes into the first (d2q9-bgk.c:200-203 for all members)
    HIP_TRY(hipMemcpyAsync(e->cells[1], cells, (size_t)e->n * 9 * per * sizeof(float), hipMemcpyHostToDevice, e->q.st));
    hipLaunchKernelGGL(ens_pack_planes<true>, grid, dim3(256), 0, e->q.st, e->cells[0], (float *)nullptr, (const int *)nullptr,
                       e->plane_stride, e->member_stride, e->nx, per, e->cells[1]);
  } else {
    hipLaunchKernelGGL(ens_init_cells, grid, dim3(256), 0, e->q.st, e->cells[0], e->plane_stride, e->member_stride, e->members, e->nx,
                       per);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->q.st));
  e->cur = 0;
  e->steps_done = 0;
  e->ring_fill = 0;
  e->ragged = false;
  e->m_steps.clear();
  e->m_conv.clear();
  return LBM_OK;
}

int lbm_ens_run(lbm_ens *e, int nsteps) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  return run_ens(e, nsteps, false, nullptr);
}

int lbm_ens_run_timed(lbm_ens *e, int nsteps, double *ms) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  return run_ens(e, nsteps, true, ms);
}

int lbm_ens_sync(lbm_ens *e) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  return queue_sync(e->q);
}

int lbm_ens_steps_done(const lbm_ens *e) { return e ? e->steps_done : -1; }
int lbm_ens_members(const lbm_ens *e) { return e ? e->n : -1; }

int lbm_ens_download(lbm_ens *e, float *cells_out, float *av_vels_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = queue_sync(e->q)) return rc;
  const size_t per = (size_t)e->nx * e->ny;
  if (cells_out) {
    // the grid array that is not current is scratch between runs: repack every member into the caller's layout there,
    // then one contiguous transfer.  A ragged ensemble has no scratch array: every member from the array that holds it,
    // into a staging array of its own
    float *stage = e->cells[e->cur ^ 1];
    if (e->ragged) {
      if (int rc = stage_alloc(e)) return rc;
      stage = e->stage;
    }
    hipLaunchKernelGGL(ens_pack_planes<false>, dim3((unsigned)std::min(div_up((long)per, 256), 1024L), e->n), dim3(256), 0, e->q.st,
                       e->cells[e->ragged ? 0 : e->cur], e->cells[1], member_parity(e), e->plane_stride, e->member_stride, e->nx,
                       per, stage);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cells_out, stage, (size_t)e->n * 9 * per * sizeof(float), hipMemcpyDeviceToHost, e->q.st));
    HIP_TRY(hipStreamSynchronize(e->q.st));
  }
  if (av_vels_out && e->steps_done > 0) {
    const int T = e->steps_done;
    std::vector<double> sums((size_t)e->n * T);
    HIP_TRY(hipMemcpy2D(sums.data(), (size_t)T * sizeof(double), e->av_sum, (size_t)std::max(1, e->max_iters) * sizeof(double),
                        (size_t)T * sizeof(double), e->n, hipMemcpyDeviceToHost));
    // kernels.cl:202: sum * FREE_CELLS_INV, the member's own
    for (int m = 0; m < e->n; m++)
      for (int t = 0; t < T; t++)
        av_vels_out[(size_t)m * T + t] = (float)(sums[(size_t)m * T + t] * (double)e->p[m].free_cells_inv);
    // a member that stopped earlier has no record from its own count on
    if (e->ragged)
      for (int m = 0; m < e->n; m++)
        for (int t = e->m_steps[m]; t < T; t++) av_vels_out[(size_t)m * T + t] = 0.0f;
  }
  return LBM_OK;
}

int lbm_ens_final_state(lbm_ens *e, float *u_x, float *u_y, float *u, float *pressure) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = queue_sync(e->q)) return rc;
  const size_t per = (size_t)e->nx * e->ny, all = per * e->n;
  float *outs[4] = {u_x, u_y, u, pressure};
  // the four columns of all members go to the grid array that is not current (4 n nx ny floats of its 9 n nx ny)
  // (a ragged ensemble: to its staging array, as lbm_ens_download)
  float *d[4] = {nullptr, nullptr, nullptr, nullptr};
  float *stage = e->cells[e->cur ^ 1];
  if (e->ragged) {
    if (int rc = stage_alloc(e)) return rc;
    stage = e->stage;
  }
  for (int i = 0; i < 4; i++)
    if (outs[i]) d[i] = stage + (size_t)i * all;
  hipLaunchKernelGGL(ens_final_fields, dim3(e->fin_blocks, e->n), dim3(kBlock), 0, e->q.st, e->cells[e->ragged ? 0 : e->cur],
                     e->cells[1], member_parity(e), e->plane_stride, e->member_stride, e->nx, e->mask, per, e->members, d[0], d[1],
                     d[2], d[3], e->fin_partials);
  HIP_TRY(hipGetLastError());
  for (int i = 0; i < 4; i++)
    if (outs[i]) HIP_TRY(hipMemcpyAsync(outs[i], d[i], all * sizeof(float), hipMemcpyDeviceToHost, e->q.st));
  HIP_TRY(hipStreamSynchronize(e->q.st));
  return LBM_OK;
}

int lbm_ens_reynolds(lbm_ens *e, float *reynolds_out) {
  if (!e || !reynolds_out) return lbm_fail(LBM_ERR_ARG, "NULL argument");
  if (int rc = queue_sync(e->q)) return rc;
  const size_t per = (size_t)e->nx * e->ny;
  hipLaunchKernelGGL(ens_final_fields, dim3(e->fin_blocks, e->n), dim3(kBlock), 0, e->q.st, e->cells[e->ragged ? 0 : e->cur],
                     e->cells[1], member_parity(e), e->plane_stride, e->member_stride, e->nx, e->mask, per, e->members,
                     (float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr, e->fin_partials);
  HIP_TRY(hipGetLastError());
  std::vector<float> part((size_t)e->n * e->fin_blocks);
  HIP_TRY(hipMemcpyAsync(part.data(), e->fin_partials, part.size() * sizeof(float), hipMemcpyDeviceToHost, e->q.st));
  HIP_TRY(hipStreamSynchronize(e->q.st));
  for (int m = 0; m < e->n; m++) {
    double tot = 0.0;
    for (int b = 0; b < e->fin_blocks; b++) tot += part[(size_t)m * e->fin_blocks + b];
    // d2q9-bgk.c:747-752
    const lbm_params &p = e->p[m];
    const float viscosity = 1.0f / 6.0f * (2.0f / p.omega - 1.0f);
    const float av = (float)(tot * (double)p.free_cells_inv);
    reynolds_out[m] = av * p.reynolds_dim / viscosity;
  }
  return LBM_OK;
}

int lbm_steady_run(lbm_ens *e, int max_steps, int window, double rel_tol) {
  // every argument error is reported before the ensemble or a device is touched
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  if (int rc = check_steady_args(max_steps, window, rel_tol)) return rc;
  bool launched = false;
  const int rc = steady_impl(e, max_steps, window, rel_tol, &launched);
  return latch_failure(rc, launched, e->q.st, &e->failed);
}

int lbm_steady_steps(lbm_ens *e, int *steps_out, int *converged_out) {
  if (!e) return lbm_fail(LBM_ERR_ARG, "ensemble is NULL");
  steady_steps_out(e->n, e->ragged, e->steps_done, e->m_steps, e->m_conv, steps_out, converged_out);
  return LBM_OK;
}

void lbm_ens_destroy(lbm_ens *e) {
  if (!e) return;
  (void)hipSetDevice(e->q.dev);
  free_ens(e);
}

}  // extern "C"

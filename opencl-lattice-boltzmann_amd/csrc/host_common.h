// What the host sides of the ensembles, the double-precision contexts and the double-precision ensembles share
// (lbm_ensemble.cpp, lbm_dp.cpp, lbm_dens.cpp): plain inline helpers over the fields they need, no knowledge of who calls.
// The steady-run helpers are shared by the two ensemble units.
// Whatever differs between those units in more than a scalar type - sizes, argument structs, launches, reductions - is theirs.
#pragma once
#include "../../include/lbm.h"
#include "lbm_error.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess)                                                                           \
      return lbm_fail(LBM_ERR_HIP, "HIP error during '%s' (%s:%d): %s", #expr, __FILE__, __LINE__, \
                      hipGetErrorString(e_));                                                       \
  } while (0)

namespace lbm_host {

inline long div_up(long a, long b) { return (a + b - 1) / b; }

inline bool positive_finite(double v) { return std::isfinite(v) && v > 0.0; }

// `rem` steps in as few launches of at most T steps as possible, of equal depth: the depth of the next one (20 at T = 8: 7 + 7 + 6)
inline int equal_depth(int rem, int T) { return (int)div_up(rem, div_up(rem, T)); }

// Steps a ring of per-step segment sums holds: as many as fit `ring_bytes` at `step_bytes` a step, at least `least` (the
// most steps one launch advances), at most `most`
inline int ring_steps(size_t step_bytes, int least, int most, size_t ring_bytes) {
  return (int)std::max<size_t>((size_t)least, std::min<size_t>((size_t)most, ring_bytes / step_bytes));
}

// hipMalloc for callers that undo something on failure instead of returning at once
inline int hip_alloc(void **ptr, size_t bytes) {
  HIP_TRY(hipMalloc(ptr, bytes));
  return LBM_OK;
}

// ---- the device, its stream and the two events of a timed run ----
struct Queue {
  int dev = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
};

// the stream and the events on the current device (`dev` is the owner's to record, before its first query of the device)
inline int queue_create(Queue &q) {
  HIP_TRY(hipStreamCreateWithFlags(&q.st, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&q.ev_t0));
  HIP_TRY(hipEventCreate(&q.ev_t1));
  return LBM_OK;
}

// Teardown in two halves around the owner's frees: what is enqueued finishes before its memory goes, the events and the
// stream go last.  Both take a queue that was never (or only partly) created.
inline void queue_drain(const Queue &q) {
  if (q.st) (void)hipStreamSynchronize(q.st);
}

inline void queue_destroy(Queue &q) {
  if (q.ev_t0) (void)hipEventDestroy(q.ev_t0);
  if (q.ev_t1) (void)hipEventDestroy(q.ev_t1);
  if (q.st) (void)hipStreamDestroy(q.st);
}

inline int queue_sync(const Queue &q) {
  HIP_TRY(hipSetDevice(q.dev));
  HIP_TRY(hipStreamSynchronize(q.st));
  return LBM_OK;
}

// The bracket of a timed run around its enqueues; both are no-ops when `timed` is false.  The end waits for the run.
inline int timed_begin(const Queue &q, bool timed) {
  if (timed) HIP_TRY(hipEventRecord(q.ev_t0, q.st));
  return LBM_OK;
}

inline int timed_end(const Queue &q, bool timed, double *ms) {
  if (!timed) return LBM_OK;
  HIP_TRY(hipEventRecord(q.ev_t1, q.st));
  HIP_TRY(hipEventSynchronize(q.ev_t1));
  float t = 0.0f;
  HIP_TRY(hipEventElapsedTime(&t, q.ev_t0, q.ev_t1));
  if (ms) *ms = t;
  return LBM_OK;
}

// ---- what a run checks before it touches the device ----
// noun: what the caller is asked to destroy ("context", "ensemble")
inline int check_runnable(int nsteps, bool failed, const char *noun) {
  if (nsteps < 0) return lbm_fail(LBM_ERR_ARG, "nsteps must be >= 0");
  if (failed) return lbm_fail(LBM_ERR_STATE, "an earlier run failed after its launches had begun; destroy the %s", noun);
  return LBM_OK;
}

// upto: "" for a run of exactly `more` steps, "up to " for one that may stop earlier
inline int check_record(int max_iters, int steps_done, int more, const char *upto) {
  if (steps_done + more > max_iters)
    return lbm_fail(LBM_ERR_STATE, "av_vels record holds max_iters=%d steps; %d done, %s%d more requested", max_iters, steps_done,
                    upto, more);
  return LBM_OK;
}

// ---- failures ----
// `keep` (lbm_last_error() at the failure) once more under `rc`, after a cleanup whose own HIP calls may have replaced the
// message; clears the runtime's sticky error
inline int fail_again(int rc, const std::string &keep) {
  (void)hipGetLastError();
  return lbm_fail(rc, "%s", keep.c_str());
}

// A failure after launches have begun: let what was enqueued finish and refuse further work (lbm_hip.cpp's run_steps does
// the same for ordinary contexts)
inline int latch_failure(int rc, bool launched, hipStream_t st, bool *failed) {
  if (rc != LBM_OK && launched) {
    const std::string keep = lbm_last_error();
    (void)hipStreamSynchronize(st);
    *failed = true;
    fail_again(rc, keep);
  }
  return rc;
}

// ---- steady runs (lbm_steady_run, lbm_dsteady_run) ----
constexpr int kSteadyPollChecks = 4;  // a steady run reads the count of active members back after every so many checks

// what a steady run refuses before it dereferences its ensemble
inline int check_steady_args(int max_steps, int window, double rel_tol) {
  if (max_steps < 0) return lbm_fail(LBM_ERR_ARG, "max_steps must be >= 0 (got %d)", max_steps);
  if (window < 1) return lbm_fail(LBM_ERR_ARG, "window must be >= 1 (got %d)", window);
  if (!std::isfinite(rel_tol) || rel_tol < 0.0) return lbm_fail(LBM_ERR_ARG, "rel_tol must be finite and >= 0 (got %g)", rel_tol);
  return LBM_OK;
}

// End of a steady run: the members' words par[n], steps[n], conv[n] (one after the other on the device, from `par`) say on
// which parity each member is, at which count, and whether it met the criterion.  The ensemble is at the largest count and
// ragged if the counts differ; if they do not, all members stopped after the same launch and the ensemble is an ordinary
// one on that parity.
inline int steady_read_back(const Queue &q, const int *par, int n, std::vector<int> &m_steps, std::vector<int> &m_conv,
                            int *steps_done, bool *ragged, int *cur) {
  std::vector<int> words(3 * (size_t)n);
  HIP_TRY(hipMemcpyAsync(words.data(), par, words.size() * sizeof(int), hipMemcpyDeviceToHost, q.st));
  HIP_TRY(hipStreamSynchronize(q.st));
  m_steps.assign(words.begin() + n, words.begin() + 2 * (size_t)n);
  m_conv.assign(words.begin() + 2 * (size_t)n, words.end());
  *steps_done = *std::max_element(m_steps.begin(), m_steps.end());
  *ragged = *std::min_element(m_steps.begin(), m_steps.end()) != *steps_done;
  if (!*ragged) *cur = words[0];
  return LBM_OK;
}

// lbm_steady_steps / lbm_dsteady_steps: the members of an ensemble that is not ragged are all at its count, whatever ran
// since the last steady run
inline void steady_steps_out(int n, bool ragged, int steps_done, const std::vector<int> &m_steps, const std::vector<int> &m_conv,
                             int *steps_out, int *converged_out) {
  for (int m = 0; m < n; m++) {
    if (steps_out) steps_out[m] = ragged ? m_steps[m] : steps_done;
    if (converged_out) converged_out[m] = m_conv.empty() ? 0 : m_conv[m];
  }
}

// ---- creation ----
// the byte mask of `count` cells from the caller's int32 map (d2q9-bgk.c:205-209: the obstacle transfer)
inline int upload_mask(uint8_t *mask, const int32_t *obstacles, size_t count) {
  std::vector<uint8_t> m(count);
  for (size_t i = 0; i < count; i++) m[i] = obstacles[i] != 0;
  HIP_TRY(hipMemcpy(mask, m.data(), count, hipMemcpyHostToDevice));
  return LBM_OK;
}

// P: lbm_params or lbm_dparams
template <typename P>
int check_members_alike(const P *params, int n) {
  const P &p0 = params[0];
  for (int i = 1; i < n; i++)
    if (params[i].nx != p0.nx || params[i].ny != p0.ny || params[i].max_iters != p0.max_iters)
      return lbm_fail(LBM_ERR_ARG, "member %d is %dx%d with max_iters=%d, member 0 %dx%d with max_iters=%d: the members of an ensemble "
                      "share nx, ny and max_iters", i, params[i].nx, params[i].ny, params[i].max_iters, p0.nx, p0.ny, p0.max_iters);
  return LBM_OK;
}

// A member's constants from its parameters (EnsMember from lbm_params, DensMember from lbm_dparams), every operation in the
// table's own scalar type R: the fp32 ensemble divides floats by 9.0f, the fp64 one doubles by 9.0, as a context of that
// precision does
template <typename M, typename P>
M member_constants(const P &p) {
  using R = decltype(M::omega);
  M m{};
  m.omega = p.omega;
  m.aw1 = p.density * p.accel / R(9);   // kernels.cl:14-15
  m.aw2 = p.density * p.accel / R(36);
  m.density = p.density;
  m.w0 = p.density * R(4) / R(9);       // d2q9-bgk.c:529-531
  m.w1 = p.density / R(9);
  m.w2 = p.density / R(36);
  m.pad = R(0);
  return m;
}

}  // namespace lbm_host

// Device side of a STEADY RUN of an ensemble (include/lbm.h: lbm_steady_*): every member advances until its own av_vels
// record has settled, and the decision is taken on the device, so a run is enqueued without a host round trip per leg.
//
// The per-member words (`active`, `par`, `steps`, `conv`, the counter of active members) and the kernel that starts a run
// are steady_words.h's, shared with the double-precision ensembles.  d2q9_ensemble_gated is d2q9_ensemble behind a test of
// `active`: the workgroups of a stopped member return before they touch its cells or its partial sums.  After the reduction
// of every leg ens_steady_check compares two entries of each active member's record and clears the word of those that have
// settled.
#pragma once
#include "ensemble_kernels.h"
#include "steady_words.h"

namespace lbm {

template <int TX, int TY>
__global__ __launch_bounds__(kMultiThreads) void d2q9_ensemble_gated(const EnsArgs a, const int *active) {
  if (active[blockIdx.y] == 0) return;  // uniform over the workgroup, before the first barrier
  ens_tile<TX, TY>(a);
}

// After a leg that ended at step count s on parity cur: the members that were active during it are now at s.  With
// `check`, a member stops if |A(s) - A(s - window)| <= rel_tol |A(s)|, where A(t) is the float lbm_ens_download returns
// for step t, (float)(av_sum[t - 1] * (double)free_cells_inv).  Evaluated in IEEE double, difference and bound as separate
// statements with contraction off, so that the host reproduces every decision from the downloaded record.  A NaN on either
// side compares false: such a member runs on.
static __global__ void ens_steady_check(SteadyWords w, int n, const double *av_sum, unsigned long long record,
                                        const float *free_cells_inv, int s, int window, double rel_tol, int check, int cur) {
#pragma clang fp contract(off)
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n || w.active[m] == 0) return;
  w.steps[m] = s;
  w.par[m] = cur;
  if (!check) return;
  const double *av = av_sum + (size_t)m * record;
  const double inv = (double)free_cells_inv[m];
  const float a_now = (float)(av[s - 1] * inv);
  const float a_then = (float)(av[s - window - 1] * inv);
  const double diff = fabs((double)a_now - (double)a_then);
  const double bound = rel_tol * fabs((double)a_now);
  if (diff <= bound) {
    w.active[m] = 0;
    w.conv[m] = 1;
    atomicSub(w.count, 1);
  }
}

}  // namespace lbm

// What the steady runs of the two ensemble families share on the device (include/lbm.h: lbm_steady_*, lbm_dsteady_*): the
// per-member words and the kernel that starts a run.  Nothing here depends on the precision of the cells; the gated tile
// kernel and the criterion kernel of each family are its own (steady_kernels.h, dp_steady_kernels.h).
//
// Per member there are four words in device memory: `active` (1 while the member still advances), `par` (which of the two
// grid arrays holds its state), `steps` (steps applied) and `conv` (it met the criterion), and one counter of active members
// for the host to poll.  The members that are still active have all been advanced by the same launches, so they share one
// parity, the host's; a stopped member keeps the parity it had when it stopped.  The words are written with ordinary
// stores, one lane per member, and the counter with atomicSub.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace lbm {

struct SteadyWords {
  int *active, *par, *steps, *conv;  // [members] each
  int *count;                        // members with active != 0
};

constexpr size_t kSteadyWordCount = 4;  // arrays of one word per member, then the counter

// the words of n members in one allocation of kSteadyWordCount * n + 1 ints
inline SteadyWords steady_words_at(int *w, size_t n) { return SteadyWords{w, w + n, w + 2 * n, w + 3 * n, w + 4 * n}; }

// start of a steady run: every member active, on the ensemble's parity, at the ensemble's step count
static __global__ void ens_steady_begin(SteadyWords w, int n, int cur, int s0) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m == 0) *w.count = n;
  if (m >= n) return;
  w.active[m] = 1;
  w.par[m] = cur;
  w.steps[m] = s0;
  w.conv[m] = 0;
}

}  // namespace lbm

// Device side of a STEADY RUN of a double-precision ensemble (include/lbm.h: lbm_dsteady_*): steady_kernels.h for the fp64
// members of dp_ensemble_kernels.h.  The per-member words and the kernel that starts a run are steady_words.h's, one copy for
// both families.  d2q9_dp_ensemble_gated is d2q9_dp_ensemble behind a test of `active`: one copy of the arithmetic
// (dp_tile, dp_tile.h), so the forcing guard and every bit-identity property of the plain kernel carry over; the workgroups of a
// stopped member return before they touch its cells or its segment sums.  dp_reduce and dp_accelerate_row skip the
// same members, so a stopped member's cells, and its record beyond its count, are never written again.
//
// A step's segment sums are added in one fixed order whatever the depth of the launch that computed it (store_segments,
// dp_reduce), so the record of a steady run does not depend on how its legs cut the launches: a member stopped at count c
// holds the bits of an lbm_dens_run(e, c) in one piece, av_vels included.
#pragma once
#include "dp_ensemble_kernels.h"
#include "steady_words.h"

namespace lbm {

template <int TX, int TY, int TMAX, int NT, bool FORCE, bool TRT, bool OPEN, bool WALL = false, bool LES = false, bool DRIVE = false>
__global__ __launch_bounds__(NT, (dens_waves_per_simd<NT, FORCE, TRT, OPEN, WALL, LES, DRIVE>())) void d2q9_dp_ensemble_gated(
    const DensArgsOf<WALL> a, const int *active) {
  if (active[blockIdx.y] == 0) return;  // uniform over the workgroup, before the first barrier or LDS access
  dp_tile<TX, TY, TMAX, NT, FORCE, TRT, OPEN, WALL, LES, DRIVE, DensGrid<WALL>>(a);
}

// After a leg that ended at step count s on parity cur: the members that were active during it are now at s.  With
// `check`, a member stops if fabs(A(s) - A(s - window)) <= rel_tol * fabs(A(s)) on its record rec[m][t - 1] of step t:
//   inv != NULL (lbm_dsteady_run): rec is av_sum and A(t) the double lbm_dens_download returns for step t,
//     av_sum[t - 1] * free_cells_inv: one multiplication by the member's own inv[m].
//   inv == NULL (lbm_dbody_steady_run): rec is the members' F_x record and A(t) the entry of the member's t-th step as
//     lbm_dforce_ens_record returns it, nothing multiplied into it.
// Entirely in double, difference and bound as separate statements with contraction off, so that the host reproduces every
// decision from the downloaded record.  The reductions that write the leg's entries precede this launch on the stream
// (enqueue_steps' flush).  A NaN on either side compares false: such a member runs on (0 * inf of a member without a free
// cell).  A record of exact zeros (an empty body) gives 0 <= 0: such a member stops at its first check point.
static __global__ void dens_steady_check(SteadyWords w, int n, const double *rec, unsigned long long record, const double *inv,
                                         int s, int window, double rel_tol, int check, int cur) {
#pragma clang fp contract(off)
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n || w.active[m] == 0) return;
  w.steps[m] = s;
  w.par[m] = cur;
  if (!check) return;
  const double *r = rec + (size_t)m * record;
  double a_now = r[s - 1], a_then = r[s - window - 1];
  if (inv) {
    a_now = a_now * inv[m];
    a_then = a_then * inv[m];
  }
  const double diff = fabs(a_now - a_then);
  const double bound = rel_tol * fabs(a_now);
  if (diff <= bound) {
    w.active[m] = 0;
    w.conv[m] = 1;
    atomicSub(w.count, 1);
  }
}

}  // namespace lbm

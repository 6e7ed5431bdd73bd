// Where lbm_dp.cpp and lbm_dens.cpp drive the helper kernels of dp_kernels.h with the same statements: the second reduction
// stage and the force of the current state, for `members` grids (a context: 1).  Plain functions over the fields they need,
// as host_common.h's; static, because the kernels they launch are each unit's own copies.
#pragma once
#include "dp_kernels.h"
#include "host_common.h"

namespace lbm_host {

// Second reduction stage (kernels.cl:234-290 counterpart), all members in one launch per stage: the per_step segment sums of
// each member (per_step apart) and each of `steps` steps (`in_stride` apart from `in`) into out[m * out_member + r], in one
// stage or, where a step has many segments (red_blocks > 1), in two through red[steps][members][red_blocks].  active: NULL,
// or the members' words during a leg of a steady run (dp_reduce).
static inline int reduce_steps(hipStream_t st, const double *in, size_t in_stride, size_t per_step, int steps, int members,
                               double *red, int red_blocks, double *out, unsigned long long out_member, const int *active) {
  using lbm::dp_reduce;
  using lbm::kBlock;
  if (red_blocks > 1) {
    hipLaunchKernelGGL(dp_reduce, dim3(red_blocks, steps, members), dim3(kBlock), 0, st, in, (unsigned long long)in_stride,
                       (unsigned long long)per_step, (long)per_step, red, (unsigned long long)members * red_blocks,
                       (unsigned long long)red_blocks, active);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dp_reduce, dim3(1, steps, members), dim3(kBlock), 0, st, (const double *)red,
                       (unsigned long long)members * red_blocks, (unsigned long long)red_blocks, (long)red_blocks, out, 1ull,
                       out_member, active);
  } else {
    hipLaunchKernelGGL(dp_reduce, dim3(1, steps, members), dim3(kBlock), 0, st, in, (unsigned long long)in_stride,
                       (unsigned long long)per_step, (long)per_step, out, 1ull, out_member, active);
  }
  HIP_TRY(hipGetLastError());
  return LBM_OK;
}

// lbm_dforce / lbm_dforce_ens between their checks and their read-back: a.cells, cells_alt, par, mask, members, the strides,
// nx, ny and no_accel are the caller's.  Between runs the ring is empty (every run ends with its reduction): the first two
// blocks of members * ny * nseg of `seg` take the segment sums of F_x and F_y, which then go the way a step's go, into
// force_now[2][members].
static inline int force_state(hipStream_t st, lbm::DpForceArgs a, int nseg, int members, double *seg, double *red, int red_blocks,
                              double *force_now) {
  const size_t per_step = (size_t)a.ny * nseg, all_step = (size_t)members * per_step;
  a.seg_x = seg;
  a.seg_y = seg + all_step;
  a.lanes_per_row = nseg * 8;
  hipLaunchKernelGGL(lbm::dp_force_state, dim3((unsigned)div_up((long)a.lanes_per_row * a.ny, lbm::kBlock), members), dim3(lbm::kBlock),
                     0, st, a);
  HIP_TRY(hipGetLastError());
  for (int c = 0; c < 2; c++)
    if (int rc = reduce_steps(st, seg + (size_t)c * all_step, all_step, per_step, 1, members, red, red_blocks,
                              force_now + (size_t)c * members, 1ull, nullptr))
      return rc;
  return LBM_OK;
}

}  // namespace lbm_host

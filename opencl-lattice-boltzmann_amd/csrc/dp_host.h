// Where lbm_dp.cpp and lbm_dens.cpp drive the helper kernels of dp_kernels.h with the same statements: the second reduction
// stage, the force of the current state, the scalar (dp_scalar_kernels.h) and buoyancy (dp_buoyant_kernels.h), for `members` grids
// (a context: 1).  Plain functions over the fields they need,
// as host_common.h's; static, because the kernels they launch are each unit's own copies.
#pragma once
#include "dp_buoyant_kernels.h"
#include "dp_kernels.h"
#include "dp_scalar_kernels.h"
#include "host_common.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

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

// ---- passive scalar (include/lbm.h, "Scalar transport"; lbm_dscalar_*) -------------------------------------------------------
// What a handle holds of its scalar, and the grid it rides on as both families describe theirs.  Everything the two hosts say
// alike is here: the checks, the set, the step launch, the output stage and the transfers.
struct ScalarState {
  bool on = false;
  int cur = 0;
  std::vector<double> diffusivity, omega_s;   // [members], empty while off
  double *g[2] = {nullptr, nullptr};          // [members][ny][5][plane_stride] each (allocated by the first set that switches on)
  double *c_wall = nullptr;                   // [members][ny][nx]
  double *c_in = nullptr;                     // [members][ny]
  lbm::DpScalarMember *table = nullptr;       // [members]
  const double *table_drive = nullptr;        // the body-force table the device table was written for
  unsigned long long table_drive_stride = 0;
};

struct ScalarGrid {
  int members, nx, ny;
  size_t plane_stride, flow_member_stride;   // doubles
  size_t cells() const { return (size_t)nx * ny; }
  size_t member_stride() const { return 5 * plane_stride * (size_t)ny; }
  int lanes_per_row() const { return (int)(div_up(div_up(nx, 2), 8) * 8); }
  dim3 helper_grid() const { return dim3((unsigned)std::min(div_up((long)cells(), 256), 1024L), members); }
};

static inline void scalar_free(ScalarState &s) {
  for (double *g : s.g)
    if (g) (void)hipFree(g);
  if (s.c_wall) (void)hipFree(s.c_wall);
  if (s.c_in) (void)hipFree(s.c_in);
  if (s.table) (void)hipFree(s.table);
}

// What lbm_dscalar_set / lbm_dscalar_ens_set refuse: everything is checked before anything changes.  ens: the message names the
// member, and a diffusivity of 0 is refused too (a context's caller has taken 0 as "off" before it comes here).
static inline int scalar_check(const ScalarGrid &gr, bool ens, const double *diffusivity, const double *c0, const double *c_wall,
                               const double *c_in) {
  const size_t n = gr.cells();
  char who[32] = "";
  for (int m = 0; m < gr.members; m++) {
    if (ens) snprintf(who, sizeof(who), "member %d: ", m);
    const double D = diffusivity[m];
    if (!std::isfinite(D) || D < 0.0 || (ens && D == 0.0))
      return lbm_fail(LBM_ERR_ARG, "%sthe diffusivity must be finite and %s (got %g)%s", who, ens ? "positive" : "positive, or 0 (off)", D,
                      ens ? "; an ensemble has the scalar on for all members or, with a NULL array, off" : "");
  }
  if (!c0) return lbm_fail(LBM_ERR_ARG, "c0 is NULL (the diffusivity is positive: a scalar starts from a field)");
  for (int m = 0; m < gr.members; m++) {
    if (ens) snprintf(who, sizeof(who), "member %d: ", m);
    for (size_t i = 0; i < n; i++)
      if (!std::isfinite(c0[m * n + i]))
        return lbm_fail(LBM_ERR_ARG, "%sc0 of cell (%d, %d) must be finite (got %g)", who, (int)(i % gr.nx), (int)(i / gr.nx), c0[m * n + i]);
    if (c_wall)
      for (size_t i = 0; i < n; i++)
        if (std::isinf(c_wall[m * n + i]))
          return lbm_fail(LBM_ERR_ARG, "%sc_wall of cell (%d, %d) is infinite: a wall is held at a finite value or, with NaN, insulating", who,
                          (int)(i % gr.nx), (int)(i / gr.nx));
    if (c_in)
      for (int y = 0; y < gr.ny; y++)
        if (!std::isfinite(c_in[(size_t)m * gr.ny + y]))
          return lbm_fail(LBM_ERR_ARG, "%sc_in of row %d must be finite (got %g)", who, y, c_in[(size_t)m * gr.ny + y]);
  }
  return LBM_OK;
}

// The device table for these rates: member m's offsets, and its body force at drive + m * drive_stride (drive NULL: none)
static inline int scalar_table(ScalarState &s, const ScalarGrid &gr, const std::vector<double> &omega_s, const double *drive,
                               unsigned long long drive_stride) {
  std::vector<lbm::DpScalarMember> t(gr.members);
  for (int m = 0; m < gr.members; m++) {
    t[m] = lbm::DpScalarMember{};
    t[m].omega_s = omega_s[m];
    t[m].state_off = (unsigned long long)m * gr.member_stride();
    t[m].flow_off = (unsigned long long)m * gr.flow_member_stride;
    t[m].cell_off = (unsigned long long)m * gr.cells();
    t[m].in_off = (unsigned long long)m * gr.ny;
    t[m].drive = drive ? drive + (size_t)m * drive_stride : nullptr;
  }
  HIP_TRY(hipMemcpy(s.table, t.data(), t.size() * sizeof(lbm::DpScalarMember), hipMemcpyHostToDevice));
  s.table_drive = drive;
  s.table_drive_stride = drive_stride;
  return LBM_OK;
}

// Behind scalar_check and the caller's synchronisation: the scalar of every member on, from c0.  The arrays are allocated by the
// first call; c_wall NULL: all insulating (NaN), c_in NULL: zeros.
static inline int scalar_set(ScalarState &s, const ScalarGrid &gr, hipStream_t st, const double *diffusivity, const double *c0,
                             const double *c_wall, const double *c_in, const double *drive, unsigned long long drive_stride) {
  const size_t n = gr.cells(), all = (size_t)gr.members * n;
  const size_t g_bytes = ((size_t)gr.members * gr.member_stride() + 32) * sizeof(double);
  for (double *&g : s.g)
    if (!g) {
      HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g), g_bytes));
      HIP_TRY(hipMemset(g, 0, g_bytes));
    }
  if (!s.c_wall) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.c_wall), all * sizeof(double)));
  if (!s.c_in) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.c_in), (size_t)gr.members * gr.ny * sizeof(double)));
  if (!s.table) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.table), (size_t)gr.members * sizeof(lbm::DpScalarMember)));
  std::vector<double> omega_s(gr.members);
  for (int m = 0; m < gr.members; m++) omega_s[m] = lbm::dp_scalar_omega(diffusivity[m]);
  if (int rc = scalar_table(s, gr, omega_s, drive, drive_stride)) return rc;
  if (c_wall) {
    HIP_TRY(hipMemcpy(s.c_wall, c_wall, all * sizeof(double), hipMemcpyHostToDevice));
  } else {
    const std::vector<double> nan(all, std::numeric_limits<double>::quiet_NaN());
    HIP_TRY(hipMemcpy(s.c_wall, nan.data(), all * sizeof(double), hipMemcpyHostToDevice));
  }
  if (c_in) HIP_TRY(hipMemcpy(s.c_in, c_in, (size_t)gr.members * gr.ny * sizeof(double), hipMemcpyHostToDevice));
  else HIP_TRY(hipMemset(s.c_in, 0, (size_t)gr.members * gr.ny * sizeof(double)));
  // c0 staged in the second array (members nx ny <= its size), the rest state into the first
  HIP_TRY(hipMemcpyAsync(s.g[1], c0, all * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(lbm::dp_scalar_init, gr.helper_grid(), dim3(256), 0, st, s.g[0], (unsigned long long)gr.plane_stride,
                     (unsigned long long)gr.member_stride(), gr.nx, n, (const double *)s.g[1]);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  s.cur = 0;
  s.on = true;
  s.diffusivity.assign(diffusivity, diffusivity + gr.members);
  s.omega_s = omega_s;
  return LBM_OK;
}

// One scalar step of all members on the flow state `flow` (the array the flow's next launch streams), enqueued; flips s.cur.
// buoy: NULL (the passive scalar), or the members' buoyant constants (dp_scalar_step<true>)
static inline int scalar_step(ScalarState &s, const ScalarGrid &gr, hipStream_t st, const double *flow, const uint8_t *mask, bool open,
                              const lbm::DpBuoyMember *buoy = nullptr) {
  lbm::DpScalarBuoyArgs a{};
  a.flow = flow;
  a.src = s.g[s.cur];
  a.dst = s.g[s.cur ^ 1];
  a.mask = mask;
  a.c_wall = s.c_wall;
  a.c_in = s.c_in;
  a.members = s.table;
  a.plane_stride = gr.plane_stride;
  a.nx = gr.nx;
  a.ny = gr.ny;
  a.lanes_per_row = gr.lanes_per_row();
  a.open = open ? 1 : 0;
  a.buoy = buoy;
  const dim3 grid((unsigned)div_up((long)a.lanes_per_row * gr.ny, lbm::kBlock), gr.members);
  if (buoy) hipLaunchKernelGGL(lbm::dp_scalar_step<true>, grid, dim3(lbm::kBlock), 0, st, a);
  else hipLaunchKernelGGL(lbm::dp_scalar_step<false>, grid, dim3(lbm::kBlock), 0, st, static_cast<const lbm::DpScalarArgs &>(a));
  HIP_TRY(hipGetLastError());
  s.cur ^= 1;
  return LBM_OK;
}

// Before the first scalar step of a run: the device table names the body force as it is set now
static inline int scalar_begin_run(ScalarState &s, const ScalarGrid &gr, const double *drive, unsigned long long drive_stride) {
  if (s.table_drive == drive && s.table_drive_stride == drive_stride) return LBM_OK;
  return scalar_table(s, gr, s.omega_s, drive, drive_stride);
}

static inline int scalar_refuse_off(const char *what) {
  return lbm_fail(LBM_ERR_ARG, "%s: the scalar is off (lbm_dscalar_set / lbm_dscalar_ens_set with a positive diffusivity switches it on)", what);
}

// The output stage and the two transfers, behind the caller's checks and synchronisation.  The array that is not current is
// scratch between runs (5 members nx ny doubles at most).
static inline int scalar_field(ScalarState &s, const ScalarGrid &gr, hipStream_t st, const uint8_t *mask, double *c_out) {
  double *stage = s.g[s.cur ^ 1];
  hipLaunchKernelGGL(lbm::dp_scalar_field, gr.helper_grid(), dim3(256), 0, st, (const double *)s.g[s.cur], (unsigned long long)gr.plane_stride,
                     (unsigned long long)gr.member_stride(), gr.nx, mask, gr.cells(), stage);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c_out, stage, (size_t)gr.members * gr.cells() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return LBM_OK;
}

static inline int scalar_download(ScalarState &s, const ScalarGrid &gr, hipStream_t st, double *g_out) {
  double *stage = s.g[s.cur ^ 1];
  hipLaunchKernelGGL(lbm::dp_scalar_pack<false>, gr.helper_grid(), dim3(256), 0, st, s.g[s.cur], (unsigned long long)gr.plane_stride,
                     (unsigned long long)gr.member_stride(), gr.nx, gr.cells(), stage);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(g_out, stage, 5 * (size_t)gr.members * gr.cells() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return LBM_OK;
}

static inline int scalar_upload(ScalarState &s, const ScalarGrid &gr, hipStream_t st, const double *g) {
  double *stage = s.g[s.cur ^ 1];
  HIP_TRY(hipMemcpyAsync(stage, g, 5 * (size_t)gr.members * gr.cells() * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(lbm::dp_scalar_pack<true>, gr.helper_grid(), dim3(256), 0, st, s.g[s.cur], (unsigned long long)gr.plane_stride,
                     (unsigned long long)gr.member_stride(), gr.nx, gr.cells(), stage);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return LBM_OK;
}

// ---- buoyancy (include/lbm.h, "Buoyancy"; lbm_dbuoy_*) -----------------------------------------------------------------------
// What a handle holds of it, and what the two hosts say alike: the checks, the device table and the buoyant flow launch.
struct BuoyState {
  bool on = false;
  std::vector<double> b;                     // [members][3]: b_x, b_y, c_ref; empty while off
  lbm::DpBuoyMember *table = nullptr;        // device, [members] (allocated by the first set that switches on)
  std::vector<lbm::DpBuoyMember> uploaded;   // what the device table holds
};

static inline void buoy_free(BuoyState &s) {
  if (s.table) (void)hipFree(s.table);
}

// What lbm_dbuoy_set / lbm_dbuoy_ens_set refuse of their values, before the handle is read: b = double[members][3].  ens: the
// message names the member, and a member whose b is (0, 0) is refused too (its context twin would run the passive path).
static inline int buoy_check_values(const double *b, int members, bool ens) {
  char who[32] = "";
  for (int m = 0; m < members; m++) {
    if (ens) snprintf(who, sizeof(who), "member %d: ", m);
    const double *v = b + 3 * (size_t)m;
    if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2]))
      return lbm_fail(LBM_ERR_ARG, "%sthe buoyancy must be finite (got b_x = %g, b_y = %g, c_ref = %g)", who, v[0], v[1], v[2]);
    if (ens && !lbm::dp_drive_on(v[0], v[1]))
      return lbm_fail(LBM_ERR_ARG, "%sthe buoyancy is (0, 0); an ensemble has buoyancy on for all members or, with a NULL array, off", who);
  }
  return LBM_OK;
}

// What they refuse of the handle's state; switching_on: the call sets a b other than (0, 0)
static inline int buoy_check_state(const ScalarState &scalar, int steps_done, bool switching_on) {
  if (switching_on && !scalar.on)
    return lbm_fail(LBM_ERR_STATE, "buoyancy needs a scalar: the scalar is off (lbm_dscalar_set / lbm_dscalar_ens_set switches it on first)");
  if (steps_done != 0)
    return lbm_fail(LBM_ERR_STATE, "buoyancy is set before the first step (%d done): one record holds one flow", steps_done);
  return LBM_OK;
}

static inline int buoy_refuse_scalar_off() {
  return lbm_fail(LBM_ERR_STATE, "the scalar cannot be switched off while buoyancy is on: the flow reads it (lbm_dbuoy_set / "
                  "lbm_dbuoy_ens_set switches buoyancy off first)");
}

// Behind the checks and the caller's synchronisation.  b NULL: off.
static inline int buoy_set(BuoyState &s, const double *b, int members) {
  if (!b) {
    s.on = false;
    s.b.clear();
    return LBM_OK;
  }
  if (!s.table) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.table), (size_t)members * sizeof(lbm::DpBuoyMember)));
  s.on = true;
  s.b.assign(b, b + 3 * (size_t)members);
  s.uploaded.clear();
  return LBM_OK;
}

// The device table as the handle's settings stand now: t holds every member's flow constants and body force (the caller's),
// b and c_ref come from s.  Written only where it differs from what the device holds, behind a synchronisation of the stream.
static inline int buoy_table(BuoyState &s, hipStream_t st, std::vector<lbm::DpBuoyMember> &t) {
  for (size_t m = 0; m < t.size(); m++) {
    t[m].buoy.b_x = s.b[3 * m];
    t[m].buoy.b_y = s.b[3 * m + 1];
    t[m].buoy.c_ref = s.b[3 * m + 2];
    t[m].pad = 0.0;
  }
  if (s.uploaded.size() == t.size() && !memcmp(s.uploaded.data(), t.data(), t.size() * sizeof(lbm::DpBuoyMember))) return LBM_OK;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(s.table, t.data(), t.size() * sizeof(lbm::DpBuoyMember), hipMemcpyHostToDevice));
  s.uploaded = t;
  return LBM_OK;
}

// One buoyant flow step of all members, enqueued: the instance the five options choose
static inline int buoy_launch(hipStream_t st, bool force, bool trt, bool open, bool wall, bool les, const lbm::DpBuoyArgs &a, int members) {
  const dim3 grid((unsigned)div_up((long)a.lanes_per_row * a.ny, lbm::kBlock), members);
  lbm::dp_with_flags(force, trt, open, wall, les, false, [&](auto fo, auto tr, auto op, auto wa, auto le, auto) {
    hipLaunchKernelGGL((lbm::d2q9_dp_buoyant<decltype(fo)::value, decltype(tr)::value, decltype(op)::value, decltype(wa)::value,
                                            decltype(le)::value>), grid, dim3(lbm::kBlock), 0, st, a);
  });
  HIP_TRY(hipGetLastError());
  return LBM_OK;
}

}  // namespace lbm_host

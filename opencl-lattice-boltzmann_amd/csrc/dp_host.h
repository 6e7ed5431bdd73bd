// Where lbm_dp.cpp and lbm_dens.cpp drive the helper kernels of dp_kernels.h with the same statements: the second reduction
// stage, the force of the current state, the settings of the six flow options with their device tables, the scalar
// (dp_scalar_kernels.h), buoyancy (dp_buoyant_kernels.h) and the running statistics (dp_stats_kernels.h, stats_plan.h), for `members`
// grids (a context: 1).  Plain functions over the fields
// they need, as host_common.h's; static, because the kernels they launch are each unit's own copies.
#pragma once
#include "body_map.h"
#include "dp_buoyant_kernels.h"
#include "dp_kernels.h"
#include "dp_scalar_kernels.h"
#include "dp_stats_kernels.h"
#include "host_common.h"
#include "stats_plan.h"

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

// ---- the six flow options ("force", lbm_dtrt_*, lbm_dopen_*, lbm_dwall_*, lbm_dles_*, lbm_ddrive_*) ---------------------------
// What a handle holds of them for its `members` grids.  The per-member constants lie on the device in the tables behind the
// handle's DpMember table (dp_kernels.h: dens_*_table), a context's as an ensemble's of one member; the host copies here are
// what the getters return and what a context's step kernels take as arguments (element 0).  "Off" is one spelling, a NULL
// array: a context's entry point turns its 0 into that before it comes here.
struct FlowState {
  bool force = false;              // option "force": the kernels' FORCE instances, three values per segment
  bool trt = false;                // the TRT instances, for all members
  bool open = false;               // the OPEN instances for all members, no accelerate_flow
  bool wall = false;               // the WALL instances for all members
  bool les = false;                // the LES instances, for all members
  bool drive = false;              // the DRIVE instances, for all members
  std::vector<double> magic;       // [members]: every member's magic parameter, 0 while BGK
  std::vector<double> omega_m;     // [members]: the host's copy of DpMember::omega_m (BGK: the member's omega)
  std::vector<double> open_host;   // [members][ny + 1]: per member u_in[ny], then rho_out (zeros while off); dens_open_table
  std::vector<double> wall_u;      // [2][members][ny][nx]: the host's copy of the wall velocities, u_x then u_y (empty while off)
  std::vector<double> rho_wall;    // [members]: the wall densities, 0 while off; dens_wall_table
  double *wall_dev = nullptr;      // [2][members][ny][nx] (allocated by the first wall_set that switches on)
  std::vector<double> les_c;       // [members]: every member's Smagorinsky constant, 0 while off; DpLes in dens_les_table
  std::vector<double> drive_f;     // [members][2]: every member's force density, 0 while off; dens_drive_table
};

// The grids a state belongs to, as both handles describe theirs when a setter is called, and their ring of segment sums: the
// handle's own three fields, and the sizes that fix them
struct FlowGrid {
  int members;
  const lbm_dparams *p;   // [members]; nx, ny and max_iters are those of p[0]
  lbm::DpMember *table;   // the device table and the four behind it
  const Queue &q;
  int steps_done;
  double *&seg, *&red;
  int &ring;
  size_t per_step;        // one member's segments of one step (ny * nseg)
  int red_blocks, tmax;   // blocks of the first reduction stage a member and step; the steps of the unit's deepest launch
};

static inline size_t flow_table_bytes(int members, int ny) {
  return (size_t)members * (sizeof(lbm::DpMember) + (size_t)(ny + 2) * sizeof(double) + sizeof(lbm::DpLes) + sizeof(lbm::DpDrive));
}

// The table of per-member constants with these second relaxation rates, to the device
static inline int upload_members(lbm::DpMember *table, const lbm_dparams *p, int members, const std::vector<double> &omega_m) {
  std::vector<lbm::DpMember> t(members);
  for (int i = 0; i < members; i++) {
    t[i] = member_constants<lbm::DpMember>(p[i]);
    t[i].omega_m = omega_m[i];
  }
  HIP_TRY(hipMemcpy(table, t.data(), t.size() * sizeof(lbm::DpMember), hipMemcpyHostToDevice));
  return LBM_OK;
}

// The table of per-member subgrid constants for these Smagorinsky constants and magic parameters, to the device: tau0 and
// les_k by the header's host statements.  Written by les_set and again by trt_set, so that the two may be set in either order.
static inline int upload_les(const FlowGrid &g, const std::vector<double> &c, const std::vector<double> &magic) {
  std::vector<lbm::DpLes> t(g.members);
  for (int i = 0; i < g.members; i++) t[i] = lbm::dp_les_constants(g.p[i].omega, c[i], magic[i]);
  HIP_TRY(hipMemcpy(const_cast<lbm::DpLes *>(lbm::dens_les_table(g.table, g.members, g.p[0].ny)), t.data(), t.size() * sizeof(lbm::DpLes),
                    hipMemcpyHostToDevice));
  return LBM_OK;
}

// At creation: the device tables, every option off.  In double the member constants are lbm_dp.cpp's own statements of old
// (run_dp_impl, lbm_dp_upload): a member's constants are a context's.
static inline int flow_create(FlowState &s, lbm::DpMember **table, const lbm_dparams *p, int members) {
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(table), flow_table_bytes(members, p[0].ny)));
  s.magic.assign(members, 0.0);
  s.open_host.assign((size_t)members * (p[0].ny + 1), 0.0);
  s.rho_wall.assign(members, 0.0);
  s.les_c.assign(members, 0.0);
  s.drive_f.assign(2 * (size_t)members, 0.0);
  s.omega_m.resize(members);
  for (int i = 0; i < members; i++) s.omega_m[i] = p[i].omega;
  return upload_members(*table, p, members, s.omega_m);
}

// Every setter below is two functions.  *_check refuses the caller's values, every member before anything changes, and reads
// of the handle no more than p (a context's entry point is called with a handle of zero bytes: tests/test_*_abi.py); ens: the
// message names the member, and words "off" as an ensemble's caller spells it.  *_set refuses the handle's state, then
// synchronises, writes the device, and changes the host copies last: after a refusal or a failed upload nothing has changed.

// values per segment and step: |u|, and F_x, F_y with the option "force"
static inline int seg_values(const FlowState &s) { return s.force ? 3 : 1; }

// The ring of per-step segment sums of all members and the first reduction stage's partials, (re)allocated for the values a
// segment carries: the ring holds as many steps as fit kRingBytes, at least the tmax steps of the unit's deepest launch.
// How many steps lie between two reductions decides no sum.
constexpr size_t kRingBytes = 32u << 20;
constexpr int kRingMax = 256;
static inline int ring_steps_of(int members, size_t per_step, int nval, int tmax) {
  return ring_steps((size_t)members * per_step * nval * sizeof(double), tmax, kRingMax, kRingBytes);
}
static inline int alloc_ring(const FlowGrid &r, int nval) {
  r.ring = ring_steps_of(r.members, r.per_step, nval, r.tmax);
  if (r.seg) HIP_TRY(hipFree(r.seg));
  r.seg = nullptr;
  if (r.red) HIP_TRY(hipFree(r.red));
  r.red = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&r.seg), (size_t)r.ring * r.members * r.per_step * nval * sizeof(double)));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&r.red), (size_t)r.ring * r.members * r.red_blocks * sizeof(double)));
  return LBM_OK;
}

// Option "force" (the key is the entry point's to match): the ring for three values a segment, and the record
// [2][members][max_iters], allocated by the first call that switches on.  failed: the handle's latch, set where the ring could
// not be put back.
static inline int force_check(long value) {
  if (value != 0 && value != 1) return lbm_fail(LBM_ERR_ARG, "force must be 0 or 1 (got %ld)", value);
  return LBM_OK;
}

static inline int force_set(FlowState &s, const FlowGrid &g, long value, bool ens, double *&force_rec, bool &failed) {
  if (g.steps_done != 0)
    return lbm_fail(LBM_ERR_STATE, "\"force\" is set before the first step (%d done): the record holds every step since %s",
                    g.steps_done, ens ? "lbm_dens_upload" : "lbm_dp_upload");
  if ((value != 0) == s.force) return LBM_OK;
  if (int rc = queue_sync(g.q)) return rc;
  const bool before = s.force;
  s.force = value != 0;
  int rc = alloc_ring(g, seg_values(s));
  if (rc == LBM_OK && s.force && !force_rec)
    rc = hip_alloc(reinterpret_cast<void **>(&force_rec), 2 * (size_t)g.members * g.p[0].max_iters * sizeof(double));
  if (rc != LBM_OK) {
    // back to a ring that fits the option as it was
    const std::string keep = lbm_last_error();
    s.force = before;
    if (alloc_ring(g, seg_values(s)) != LBM_OK) failed = true;
    return fail_again(rc, keep);
  }
  return LBM_OK;
}

// Two relaxation times.  magic: double[members], or NULL for BGK.
static inline int trt_check(const lbm_dparams *p, int members, const double *magic, bool ens) {
  char who[32] = "";
  for (int m = 0; magic && m < members; m++) {
    if (ens) snprintf(who, sizeof(who), "member %d: ", m);
    if (!(magic[m] > 0.0) || !std::isfinite(magic[m]))
      return lbm_fail(LBM_ERR_ARG, "%smagic must be %sfinite and positive (got %g)%s", who, ens ? "" : "0 (BGK) or ", magic[m],
                      ens ? "; an ensemble is all TRT or, with a NULL array, all BGK" : "");
    if (!(1.0 / p[m].omega - 0.5 > 0.0))
      return lbm_fail(LBM_ERR_ARG, "%sthe two-relaxation-time operator needs 1/omega - 1/2 > 0: omega is %g", who, p[m].omega);
  }
  return LBM_OK;
}

static inline int trt_set(FlowState &s, const FlowGrid &g, const double *magic) {
  if (g.steps_done != 0)
    return lbm_fail(LBM_ERR_STATE, "the collision operator is set before the first step (%d done): one record holds one operator",
                    g.steps_done);
  std::vector<double> omega_m(g.members);
  for (int m = 0; m < g.members; m++) omega_m[m] = magic ? lbm::dp_trt_omega_minus(g.p[m].omega, magic[m]) : g.p[m].omega;
  if (int rc = queue_sync(g.q)) return rc;
  if (int rc = upload_members(g.table, g.p, g.members, omega_m)) return rc;
  s.trt = magic != nullptr;
  if (magic) s.magic.assign(magic, magic + g.members);
  else s.magic.assign(g.members, 0.0);
  s.omega_m = omega_m;
  // the subgrid table carries the magic parameter: the TRT + LES instances recompute the second rate per cell
  if (s.les) return upload_les(g, s.les_c, s.magic);
  return LBM_OK;
}

static inline void trt_get(const FlowState &s, double *magic_out, double *omega_minus_out) {
  if (magic_out) std::copy(s.magic.begin(), s.magic.end(), magic_out);
  if (omega_minus_out) std::copy(s.omega_m.begin(), s.omega_m.end(), omega_minus_out);
}

// Open boundaries.  u_in: double[members][ny] with rho_out: double[members], or NULL for periodic.
static inline int open_check(const lbm_dparams *p, int members, const double *u_in, const double *rho_out, bool ens) {
  char who[32] = "";
  for (int m = 0; u_in && m < members; m++) {
    if (ens) snprintf(who, sizeof(who), "member %d: ", m);
    if (!positive_finite(rho_out[m])) return lbm_fail(LBM_ERR_ARG, "%srho_out must be finite and positive (got %g)", who, rho_out[m]);
    const int ny = p[0].ny;
    for (int y = 0; y < ny; y++) {
      const double u = u_in[(size_t)m * ny + y];
      if (!std::isfinite(u) || !(u < 1.0)) return lbm_fail(LBM_ERR_ARG, "%su_in of row %d must be finite and below 1 (got %g)", who, y, u);
    }
  }
  return LBM_OK;
}

// body, mask: the handle's, rewritten under the column rule (body_map.h), or without it again
static inline int open_set(FlowState &s, const FlowGrid &g, const BodyMap &body, uint8_t *mask, const double *u_in, const double *rho_out) {
  if (g.steps_done != 0)
    return lbm_fail(LBM_ERR_STATE, "open boundaries are set before the first step (%d done): one record holds one flow", g.steps_done);
  if (!u_in && !s.open) return LBM_OK;
  if (int rc = queue_sync(g.q)) return rc;
  HIP_TRY(hipSetDevice(g.q.dev));
  const size_t ny = (size_t)g.p[0].ny;
  std::vector<double> table((size_t)g.members * (ny + 1), 0.0);
  if (u_in) {
    for (int m = 0; m < g.members; m++) {
      std::copy(u_in + (size_t)m * ny, u_in + (size_t)(m + 1) * ny, table.begin() + (size_t)m * (ny + 1));
      table[(size_t)m * (ny + 1) + ny] = rho_out[m];
    }
    HIP_TRY(hipMemcpy(const_cast<double *>(lbm::dens_open_table(g.table, g.members)), table.data(), table.size() * sizeof(double),
                      hipMemcpyHostToDevice));
  }
  if (int rc = body_rewrite(body, mask, g.p[0].nx, u_in != nullptr)) return rc;
  s.open = u_in != nullptr;
  s.open_host.swap(table);
  return LBM_OK;
}

static inline void open_get(const FlowState &s, int members, int ny, int *on_out, double *u_in_out, double *rho_out_out) {
  if (on_out) *on_out = s.open ? 1 : 0;
  if (!s.open) return;
  for (int m = 0; m < members; m++) {
    const double *row = s.open_host.data() + (size_t)m * (ny + 1);
    if (u_in_out) std::copy(row, row + ny, u_in_out + (size_t)m * ny);
    if (rho_out_out) rho_out_out[m] = row[ny];
  }
}

// Moving walls.  u_x, u_y: double[members][ny][nx] each with rho_wall: double[members], or both NULL for walls at rest (the
// entry points have refused one without the other).
static inline int wall_values_check(const BodyMap &body, const lbm_dparams *p, int members, const double *u_x, const double *u_y,
                                    const double *rho_wall, bool ens) {
  if (!u_x) return LBM_OK;
  char who[32] = "";
  for (int m = 0; m < members; m++) {
    if (ens) snprintf(who, sizeof(who), "member %d: ", m);
    if (!positive_finite(rho_wall[m])) return lbm_fail(LBM_ERR_ARG, "%srho_wall must be finite and positive (got %g)", who, rho_wall[m]);
  }
  return wall_check(body, u_x, u_y, members, p[0].ny, p[0].nx, ens);
}

static inline int wall_set(FlowState &s, const FlowGrid &g, const double *u_x, const double *u_y, const double *rho_wall) {
  if (g.steps_done != 0)
    return lbm_fail(LBM_ERR_STATE, "wall velocities are set before the first step (%d done): one record holds one flow", g.steps_done);
  if (!u_x) {
    s.wall = false;
    s.wall_u.clear();
    s.rho_wall.assign(g.members, 0.0);
    return LBM_OK;
  }
  if (int rc = queue_sync(g.q)) return rc;
  HIP_TRY(hipSetDevice(g.q.dev));
  const size_t all = (size_t)g.members * g.p[0].nx * g.p[0].ny;
  if (!s.wall_dev) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.wall_dev), 2 * all * sizeof(double)));
  std::vector<double> u(2 * all);
  std::copy(u_x, u_x + all, u.begin());
  std::copy(u_y, u_y + all, u.begin() + all);
  HIP_TRY(hipMemcpy(s.wall_dev, u.data(), u.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(const_cast<double *>(lbm::dens_wall_table(g.table, g.members, g.p[0].ny)), rho_wall, (size_t)g.members * sizeof(double),
                    hipMemcpyHostToDevice));
  s.wall = true;
  s.wall_u.swap(u);
  s.rho_wall.assign(rho_wall, rho_wall + g.members);
  return LBM_OK;
}

static inline void wall_get(const FlowState &s, int *on_out, double *u_x_out, double *u_y_out, double *rho_wall_out) {
  if (on_out) *on_out = s.wall ? 1 : 0;
  if (!s.wall) return;
  const size_t all = s.wall_u.size() / 2;
  if (u_x_out) std::copy(s.wall_u.begin(), s.wall_u.begin() + all, u_x_out);
  if (u_y_out) std::copy(s.wall_u.begin() + all, s.wall_u.end(), u_y_out);
  if (rho_wall_out) std::copy(s.rho_wall.begin(), s.rho_wall.end(), rho_wall_out);
}

// Subgrid viscosity.  c: double[members], or NULL for off.
static inline int les_check(int members, const double *c, bool ens) {
  char who[32] = "";
  for (int m = 0; c && m < members; m++) {
    if (ens) snprintf(who, sizeof(who), "member %d: ", m);
    if (!(c[m] > 0.0) || !std::isfinite(c[m]))
      return lbm_fail(LBM_ERR_ARG, "%sthe Smagorinsky constant c must be %sfinite and positive (got %g)%s", who, ens ? "" : "0 (off) or ", c[m],
                      ens ? "; an ensemble has the subgrid viscosity on for all members or, with a NULL array, off" : "");
  }
  return LBM_OK;
}

static inline int les_set(FlowState &s, const FlowGrid &g, const double *c) {
  if (g.steps_done != 0)
    return lbm_fail(LBM_ERR_STATE, "the subgrid viscosity is set before the first step (%d done): one record holds one operator",
                    g.steps_done);
  if (!c) {
    s.les = false;
    s.les_c.assign(g.members, 0.0);
    return LBM_OK;
  }
  if (int rc = queue_sync(g.q)) return rc;
  HIP_TRY(hipSetDevice(g.q.dev));
  const std::vector<double> cs(c, c + g.members);
  if (int rc = upload_les(g, cs, s.magic)) return rc;
  s.les = true;
  s.les_c = cs;
  return LBM_OK;
}

// the constants a member's LES instances run with, from its omega and the two settings as they stand (either order)
static inline lbm::DpLes les_constants(const FlowState &s, const lbm_dparams *p, int m) {
  return lbm::dp_les_constants(p[m].omega, s.les_c[m], s.magic[m]);
}

static inline void les_get(const FlowState &s, const lbm_dparams *p, int members, double *c_out, double *les_k_out) {
  for (int m = 0; m < members; m++) {
    if (c_out) c_out[m] = s.les_c[m];
    if (les_k_out) les_k_out[m] = les_constants(s, p, m).les_k;
  }
}

// Body force.  f: double[members][2], or NULL for off.  ens: a member whose force is (0, 0) is refused too (a context's caller
// has taken that as "off" before the set).
static inline int drive_check(int members, const double *f, bool ens) {
  char who[32] = "";
  for (int m = 0; f && m < members; m++) {
    if (ens) snprintf(who, sizeof(who), "member %d: ", m);
    const double f_x = f[2 * (size_t)m], f_y = f[2 * (size_t)m + 1];
    if (!std::isfinite(f_x) || !std::isfinite(f_y))
      return lbm_fail(LBM_ERR_ARG, "%sthe body force must be finite (got f_x = %g, f_y = %g)", who, f_x, f_y);
    if (ens && !lbm::dp_drive_on(f_x, f_y))
      return lbm_fail(LBM_ERR_ARG, "%sthe body force is (0, 0); an ensemble has the body force on for all members or, "
                      "with a NULL array, off", who);
  }
  return LBM_OK;
}

static inline int drive_set(FlowState &s, const FlowGrid &g, const double *f) {
  if (g.steps_done != 0)
    return lbm_fail(LBM_ERR_STATE, "the body force is set before the first step (%d done): one record holds one flow", g.steps_done);
  if (!f) {
    s.drive = false;
    s.drive_f.assign(2 * (size_t)g.members, 0.0);
    return LBM_OK;
  }
  if (int rc = queue_sync(g.q)) return rc;
  HIP_TRY(hipSetDevice(g.q.dev));
  // the copy the ensemble's step kernels, the output stage and the scalar read
  HIP_TRY(hipMemcpy(const_cast<double *>(lbm::dens_drive_table(g.table, g.members, g.p[0].ny)), f, 2 * (size_t)g.members * sizeof(double),
                    hipMemcpyHostToDevice));
  s.drive = true;
  s.drive_f.assign(f, f + 2 * (size_t)g.members);
  return LBM_OK;
}

static inline void drive_get(const FlowState &s, int *on_out, double *f_out) {
  if (on_out) *on_out = s.drive ? 1 : 0;
  if (f_out) std::copy(s.drive_f.begin(), s.drive_f.end(), f_out);
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
  // the record (include/lbm.h, "Scalar record"; lbm_drecord_*), off by default; allocated by the first call that switches on
  bool record = false;
  double *rec = nullptr;                      // [3][members][max_iters]: content, flux_x, flux_y per member and step
  double *rec_seg = nullptr;                  // [rec_ring][3][members][ny][nseg]: the scalar's own ring of segment sums
  double *rec_red = nullptr;                  // [rec_ring][members][red_blocks]: first reduction stage
  int rec_ring = 0;                           // steps the ring holds
};

struct ScalarGrid {
  int members, nx, ny;
  size_t plane_stride, flow_member_stride;   // doubles
  int red_blocks = 1, max_iters = 0;         // the record: the flow's blocks of the first reduction stage, and its record's length
  size_t cells() const { return (size_t)nx * ny; }
  size_t member_stride() const { return 5 * plane_stride * (size_t)ny; }
  int lanes_per_row() const { return (int)(div_up(div_up(nx, 2), 8) * 8); }
  size_t per_step() const { return (size_t)ny * (lanes_per_row() / 8); }   // one member's segments of one step
  dim3 helper_grid() const { return dim3((unsigned)std::min(div_up((long)cells(), 256), 1024L), members); }
};

static inline void scalar_free(ScalarState &s) {
  for (double *g : s.g)
    if (g) (void)hipFree(g);
  if (s.c_wall) (void)hipFree(s.c_wall);
  if (s.c_in) (void)hipFree(s.c_in);
  if (s.table) (void)hipFree(s.table);
  if (s.rec) (void)hipFree(s.rec);
  if (s.rec_seg) (void)hipFree(s.rec_seg);
  if (s.rec_red) (void)hipFree(s.rec_red);
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

// The device table for these rates: member m's offsets, and its body force at entry m of drive, double[members][2] (the table
// behind the handle's members, dens_drive_table; NULL: none)
static inline int scalar_table(ScalarState &s, const ScalarGrid &gr, const std::vector<double> &omega_s, const double *drive) {
  std::vector<lbm::DpScalarMember> t(gr.members);
  for (int m = 0; m < gr.members; m++) {
    t[m] = lbm::DpScalarMember{};
    t[m].omega_s = omega_s[m];
    t[m].state_off = (unsigned long long)m * gr.member_stride();
    t[m].flow_off = (unsigned long long)m * gr.flow_member_stride;
    t[m].cell_off = (unsigned long long)m * gr.cells();
    t[m].in_off = (unsigned long long)m * gr.ny;
    t[m].drive = drive ? drive + 2 * (size_t)m : nullptr;
  }
  HIP_TRY(hipMemcpy(s.table, t.data(), t.size() * sizeof(lbm::DpScalarMember), hipMemcpyHostToDevice));
  s.table_drive = drive;
  return LBM_OK;
}

// Behind scalar_check and the caller's synchronisation: the scalar of every member on, from c0.  The arrays are allocated by the
// first call; c_wall NULL: all insulating (NaN), c_in NULL: zeros.
static inline int scalar_set(ScalarState &s, const ScalarGrid &gr, hipStream_t st, const double *diffusivity, const double *c0,
                             const double *c_wall, const double *c_in, const double *drive) {
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
  if (int rc = scalar_table(s, gr, omega_s, drive)) return rc;
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

// Off, behind the caller's synchronisation: the arrays stay until the handle goes; it runs as one that never had a scalar
static inline int scalar_off(ScalarState &s) {
  s.on = false;
  s.diffusivity.clear();
  s.omega_s.clear();
  return LBM_OK;
}

// One scalar step of all members on the flow state `flow` (the array the flow's next launch streams), enqueued; flips s.cur.
// buoy: NULL (the passive scalar), or the members' buoyant constants (dp_scalar_step<true>).  With the record on the kernel is
// dp_scalar_step_rec, which writes the step's segment sums into slot `slot` of the scalar's ring; active: NULL, or the members'
// words during a leg of a steady run (which the callers refuse without the record).
static inline int scalar_step(ScalarState &s, const ScalarGrid &gr, hipStream_t st, const double *flow, const uint8_t *mask, bool open,
                              const lbm::DpBuoyMember *buoy, int slot, const int *active) {
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
  if (s.record) {
    double *seg = s.rec_seg + (size_t)slot * 3 * gr.members * gr.per_step();
    if (buoy) hipLaunchKernelGGL(lbm::dp_scalar_step_rec<true>, grid, dim3(lbm::kBlock), 0, st, a, seg, active);
    else hipLaunchKernelGGL(lbm::dp_scalar_step_rec<false>, grid, dim3(lbm::kBlock), 0, st, static_cast<const lbm::DpScalarArgs &>(a), seg,
                            active);
  } else if (buoy) {
    hipLaunchKernelGGL(lbm::dp_scalar_step<true>, grid, dim3(lbm::kBlock), 0, st, a);
  } else {
    hipLaunchKernelGGL(lbm::dp_scalar_step<false>, grid, dim3(lbm::kBlock), 0, st, static_cast<const lbm::DpScalarArgs &>(a));
  }
  HIP_TRY(hipGetLastError());
  s.cur ^= 1;
  return LBM_OK;
}

// Before the first scalar step of a run: the device table names the body force as it is set now
static inline int scalar_begin_run(ScalarState &s, const ScalarGrid &gr, const double *drive) {
  if (s.table_drive == drive) return LBM_OK;
  return scalar_table(s, gr, s.omega_s, drive);
}

// ---- the scalar's record (include/lbm.h, "Scalar record") ----
// How many steps a run may buffer between two flushes: the flow's ring, and with the record on the scalar's as well
static inline int scalar_ring_limit(const ScalarState &s, int flow_ring) { return s.on && s.record ? std::min(flow_ring, s.rec_ring) : flow_ring; }

// Beside the flow's flush, for both hosts: the `fill` buffered steps of the scalar's ring through reduce_steps into entries
// `first` on of the three records, each value's segments by the launches that serve av_vels.  active: as reduce_steps.
static inline int scalar_flush(const ScalarState &s, const ScalarGrid &gr, hipStream_t st, int fill, int first, const int *active) {
  if (!s.on || !s.record || fill == 0) return LBM_OK;
  const size_t per_step = gr.per_step(), all_step = (size_t)gr.members * per_step;
  for (int v = 0; v < 3; v++)
    if (int rc = reduce_steps(st, s.rec_seg + (size_t)v * all_step, 3 * all_step, per_step, fill, gr.members, s.rec_red, gr.red_blocks,
                              s.rec + ((size_t)v * gr.members) * gr.max_iters + first, (unsigned long long)gr.max_iters, active))
      return rc;
  return LBM_OK;
}

// lbm_drecord_set / lbm_drecord_ens_set behind their NULL checks: the buoyancy rule.  The caller synchronises
// between the check and the set.
static inline int scalar_record_check(const ScalarState &s, int on, int steps_done, bool ens) {
  if (on != 0 && on != 1) return lbm_fail(LBM_ERR_ARG, "on must be 0 or 1 (got %d)", on);
  if (!s.on)
    return lbm_fail(LBM_ERR_ARG, "the scalar's record needs a scalar: the scalar is off (%s switches it on first)",
                    ens ? "lbm_dscalar_ens_set" : "lbm_dscalar_set");
  if (steps_done != 0)
    return lbm_fail(LBM_ERR_STATE, "the scalar's record is set before the first step (%d done): it holds every step since %s", steps_done,
                    ens ? "lbm_dens_upload" : "lbm_dp_upload");
  return LBM_OK;
}

static inline int scalar_record_set(ScalarState &s, const ScalarGrid &gr, int on) {
  if (on && !s.rec_seg) {
    const size_t all_step = (size_t)gr.members * gr.per_step();
    const int ring = ring_steps_of(gr.members, gr.per_step(), 3, 1);
    double *rec = nullptr, *seg = nullptr, *red = nullptr;
    int rc = hip_alloc(reinterpret_cast<void **>(&rec), 3 * (size_t)gr.members * gr.max_iters * sizeof(double));
    if (rc == LBM_OK) rc = hip_alloc(reinterpret_cast<void **>(&seg), (size_t)ring * 3 * all_step * sizeof(double));
    if (rc == LBM_OK) rc = hip_alloc(reinterpret_cast<void **>(&red), (size_t)ring * gr.members * gr.red_blocks * sizeof(double));
    if (rc != LBM_OK) {
      const std::string keep = lbm_last_error();
      if (rec) (void)hipFree(rec);
      if (seg) (void)hipFree(seg);
      if (red) (void)hipFree(red);
      return fail_again(rc, keep);
    }
    s.rec = rec;
    s.rec_seg = seg;
    s.rec_red = red;
    s.rec_ring = ring;
  }
  s.record = on != 0;
  return LBM_OK;
}

static inline int scalar_record_refuse_scalar_off() {
  return lbm_fail(LBM_ERR_STATE, "the scalar cannot be switched off while its record is on (lbm_drecord_set / "
                  "lbm_drecord_ens_set switches the record off first)");
}

// lbm_drecord / lbm_drecord_ens behind their NULL checks and the caller's synchronisation: T = steps_done entries a
// member and value; m_steps: NULL, or the members' own counts of a ragged ensemble, beyond which a member holds +0.0
static inline int scalar_record_read(const ScalarState &s, const ScalarGrid &gr, int T, const int *m_steps, double *const (&outs)[3]) {
  for (int v = 0; v < 3; v++) {
    if (!outs[v] || T == 0) continue;
    HIP_TRY(hipMemcpy2D(outs[v], (size_t)T * sizeof(double), s.rec + (size_t)v * gr.members * gr.max_iters,
                        (size_t)gr.max_iters * sizeof(double), (size_t)T * sizeof(double), gr.members, hipMemcpyDeviceToHost));
    if (m_steps)
      for (int m = 0; m < gr.members; m++)
        for (int t = m_steps[m]; t < T; t++) outs[v][(size_t)m * T + t] = 0.0;
  }
  return LBM_OK;
}

static inline int scalar_record_refuse_off(const char *what, bool ens) {
  return lbm_fail(LBM_ERR_STATE, "%s: no scalar record: it is off (%s before the first step)", what,
                  ens ? "lbm_drecord_ens_set" : "lbm_drecord_set");
}

static inline int scalar_refuse_off(const char *what) {
  return lbm_fail(LBM_ERR_ARG, "%s: the scalar is off (lbm_dscalar_set / lbm_dscalar_ens_set with a positive diffusivity switches it on)", what);
}

// The output stage and the two transfers, behind the caller's checks and synchronisation.  The array that is not current is
// scratch between runs (5 members nx ny doubles at most).  ScalarPlace: where a ragged ensemble's members lie and where its
// output is staged instead (both arrays hold states then); a default one is a handle that is not ragged.
struct ScalarPlace {
  const int *par = nullptr;   // the members' flow parities (steady_words.h)
  int off = 0;                // member m's scalar is in g[par[m] ^ off]
  double *stage = nullptr;    // 5 members nx ny doubles
};

static inline int scalar_field(ScalarState &s, const ScalarGrid &gr, hipStream_t st, const uint8_t *mask, double *c_out,
                               const ScalarPlace &at = ScalarPlace{}) {
  double *stage = at.par ? at.stage : s.g[s.cur ^ 1];
  const int cur = at.par ? at.off : s.cur;
  hipLaunchKernelGGL(lbm::dp_scalar_field, gr.helper_grid(), dim3(256), 0, st, (const double *)s.g[cur], (const double *)s.g[cur ^ 1], at.par,
                     (unsigned long long)gr.plane_stride, (unsigned long long)gr.member_stride(), gr.nx, mask, gr.cells(), stage);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c_out, stage, (size_t)gr.members * gr.cells() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return LBM_OK;
}

static inline int scalar_download(ScalarState &s, const ScalarGrid &gr, hipStream_t st, double *g_out, const ScalarPlace &at = ScalarPlace{}) {
  double *stage = at.par ? at.stage : s.g[s.cur ^ 1];
  const int cur = at.par ? at.off : s.cur;
  hipLaunchKernelGGL(lbm::dp_scalar_pack<false>, gr.helper_grid(), dim3(256), 0, st, s.g[cur], s.g[cur ^ 1], at.par,
                     (unsigned long long)gr.plane_stride, (unsigned long long)gr.member_stride(), gr.nx, gr.cells(), stage);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(g_out, stage, 5 * (size_t)gr.members * gr.cells() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return LBM_OK;
}

static inline int scalar_upload(ScalarState &s, const ScalarGrid &gr, hipStream_t st, const double *g) {
  double *stage = s.g[s.cur ^ 1];
  HIP_TRY(hipMemcpyAsync(stage, g, 5 * (size_t)gr.members * gr.cells() * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(lbm::dp_scalar_pack<true>, gr.helper_grid(), dim3(256), 0, st, s.g[s.cur], (double *)nullptr, (const int *)nullptr,
                     (unsigned long long)gr.plane_stride, (unsigned long long)gr.member_stride(), gr.nx, gr.cells(), stage);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return LBM_OK;
}

// The end of raggedness for the scalar (lbm_dens_upload): every member's state, unchanged, onto g[off], which becomes current; one
// copy launch over the members whose flow parity is 1
static inline int scalar_gather(ScalarState &s, const ScalarGrid &gr, hipStream_t st, const int *par, int off) {
  hipLaunchKernelGGL(lbm::dp_scalar_gather, dim3(64, gr.members), dim3(256), 0, st, s.g[off], (const double *)s.g[off ^ 1], par,
                     (unsigned long long)gr.member_stride());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  s.cur = off;
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

// The members' table as the handle's settings stand now, before a run and before the output stage: the flow constants are those
// the tables behind g.table hold, from the host's copies
static inline int buoy_sync(BuoyState &b, const FlowState &s, const FlowGrid &g) {
  std::vector<lbm::DpBuoyMember> t(g.members, lbm::DpBuoyMember{});
  const double *u_in = lbm::dens_open_table(g.table, g.members);
  const size_t row = (size_t)g.p[0].ny + 1;
  for (int i = 0; i < g.members; i++) {
    const lbm::DpMember m = member_constants<lbm::DpMember>(g.p[i]);
    t[i].buoy.f0_x = s.drive_f[2 * (size_t)i];
    t[i].buoy.f0_y = s.drive_f[2 * (size_t)i + 1];
    t[i].omega = g.p[i].omega;
    t[i].omega_m = s.omega_m[i];
    t[i].aw1 = m.aw1;
    t[i].aw2 = m.aw2;
    t[i].rho_out = s.open_host[i * row + row - 1];
    t[i].rho_wall = s.rho_wall[i];
    t[i].les = les_constants(s, g.p, i);
    t[i].u_in = u_in + i * row;
  }
  return buoy_table(b, g.q.st, t);
}

// One buoyant flow step of all members, enqueued: the instance the five options choose
// active: NULL, or the members' words during a leg of a steady run (d2q9_dp_buoyant_gated)
static inline int buoy_launch(hipStream_t st, bool force, bool trt, bool open, bool wall, bool les, const lbm::DpBuoyArgs &a, int members,
                              const int *active = nullptr) {
  const dim3 grid((unsigned)div_up((long)a.lanes_per_row * a.ny, lbm::kBlock), members);
  lbm::dp_with_flags(force, trt, open, wall, les, false, [&](auto fo, auto tr, auto op, auto wa, auto le, auto) {
    constexpr bool FORCE = decltype(fo)::value, TRT = decltype(tr)::value, OPEN = decltype(op)::value, WALL = decltype(wa)::value,
                   LES = decltype(le)::value;
    if (!active) hipLaunchKernelGGL((lbm::d2q9_dp_buoyant<FORCE, TRT, OPEN, WALL, LES>), grid, dim3(lbm::kBlock), 0, st, a);
    else hipLaunchKernelGGL((lbm::d2q9_dp_buoyant_gated<FORCE, TRT, OPEN, WALL, LES>), grid, dim3(lbm::kBlock), 0, st, a, active);
  });
  HIP_TRY(hipGetLastError());
  return LBM_OK;
}

// ---- running statistics (include/lbm.h, "Running statistics"; lbm_dstats_*) --------------------------------------------------
// What a handle holds of them beside its ScalarState, and what the two hosts say alike: the set, the restart behind an upload, the
// sample launch behind a piece of a run (stats_plan.h cuts the run) and the read-back.  The grid is described as for the scalar
// (ScalarGrid: members, nx, ny, plane_stride, the flow's member stride).  The count of samples is the host's: a sample is taken
// where it is enqueued.
struct StatsState {
  int every = 0;            // 0: off
  int origin = 0;           // the step count the sample points are counted from
  int samples = 0;
  double *sums = nullptr;   // [members][6][ny][plane_stride], allocated while on
};

static inline void stats_free(StatsState &s) {
  if (s.sums) (void)hipFree(s.sums);
  s = StatsState{};
}

static inline size_t stats_bytes(const ScalarGrid &gr) { return (size_t)gr.members * 6 * gr.ny * gr.plane_stride * sizeof(double); }

// what lbm_dstats_set / lbm_dstats_ens_set refuse of their value, before the handle is read
static inline int stats_check(int every) {
  if (every < 0) return lbm_fail(LBM_ERR_ARG, "every must be >= 1, or 0 (off) (got %d)", every);
  return LBM_OK;
}

// Zeros, no samples, and the origin at this step count: behind a set and behind the uploads, which keep the setting
static inline int stats_restart(StatsState &s, const ScalarGrid &gr, hipStream_t st, int steps_done) {
  if (!s.sums) return LBM_OK;
  HIP_TRY(hipMemsetAsync(s.sums, 0, stats_bytes(gr), st));
  HIP_TRY(hipStreamSynchronize(st));
  s.samples = 0;
  s.origin = steps_done;
  return LBM_OK;
}

// Behind stats_check and the caller's synchronisation.  every == 0: off, the planes go.  Setting again while on starts anew.
// Where the planes do not fit the device the statistics are off as before and nothing else has changed.
static inline int stats_set(StatsState &s, const ScalarGrid &gr, hipStream_t st, int every, int steps_done) {
  if (every == 0) {
    stats_free(s);
    return LBM_OK;
  }
  const bool fresh = !s.sums;
  if (fresh) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (stats_bytes(gr) > free_b)
      return lbm_fail(LBM_ERR_HIP, "the statistics of %d grid%s of %dx%d need %.1f MiB of device memory (48 B per cell), %.1f MiB are free",
                      gr.members, gr.members == 1 ? "" : "s", gr.nx, gr.ny, (double)stats_bytes(gr) / 1048576.0, (double)free_b / 1048576.0);
    if (int rc = hip_alloc(reinterpret_cast<void **>(&s.sums), stats_bytes(gr))) {
      s.sums = nullptr;
      return rc;
    }
  }
  if (int rc = stats_restart(s, gr, st, steps_done)) {
    const std::string keep = lbm_last_error();
    if (fresh) stats_free(s);
    return fail_again(rc, keep);
  }
  s.every = every;
  return LBM_OK;
}

static inline void stats_get(const StatsState &s, int *every_out, int *origin_out, int *samples_out) {
  if (every_out) *every_out = s.every;
  if (origin_out) *origin_out = s.origin;
  if (samples_out) *samples_out = s.samples;
}

// One sample of all members, enqueued behind a piece of a run that ends on a sample point: the state dp_final_fields would read.
// cells, mask, members, drive: dp_final_fields' arguments of the handle as it stands; scalar and buoy: NULL, or the current scalar
// array and the members' buoyant constants (buoy_sync has written them before the run).
static inline int stats_sample(StatsState &s, const ScalarGrid &gr, hipStream_t st, const double *cells, const uint8_t *mask,
                               const lbm::DpMember *members, const double *drive, const double *scalar, const lbm::DpBuoyMember *buoy) {
  lbm::DpStatsArgs a{};
  a.cells = cells;
  a.mask = mask;
  a.members = members;
  a.drive = drive;
  a.scalar = scalar;
  a.buoy = buoy;
  a.sums = s.sums;
  a.plane_stride = gr.plane_stride;
  a.member_stride = gr.flow_member_stride;
  a.nx = gr.nx;
  a.ny = gr.ny;
  a.xblocks = (int)div_up(div_up(gr.nx, 2), lbm::kStatsLanes);
  // about 2048 blocks at most, eight a CU; a block strides over the rows beyond
  a.rowgroups = (int)std::min(div_up(gr.ny, lbm::kStatsRows), std::max(1L, 2048L / ((long)a.xblocks * gr.members)));
  const dim3 grid((unsigned)(a.xblocks * a.rowgroups), gr.members);
  if (buoy) hipLaunchKernelGGL(lbm::dp_stats_sample<true>, grid, dim3(lbm::kBlock), 0, st, a);
  else hipLaunchKernelGGL(lbm::dp_stats_sample<false>, grid, dim3(lbm::kBlock), 0, st, a);
  HIP_TRY(hipGetLastError());
  s.samples++;
  return LBM_OK;
}

// lbm_dstats / lbm_dstats_ens behind their checks and the caller's synchronisation: one pitched copy into double[members][6][ny][nx]
static inline int stats_read(const StatsState &s, const ScalarGrid &gr, double *sums_out) {
  HIP_TRY(hipMemcpy2D(sums_out, (size_t)gr.nx * sizeof(double), s.sums, gr.plane_stride * sizeof(double), (size_t)gr.nx * sizeof(double),
                      (size_t)gr.members * 6 * gr.ny, hipMemcpyDeviceToHost));
  return LBM_OK;
}

static inline int stats_refuse_off(const char *what, bool ens) {
  return lbm_fail(LBM_ERR_STATE, "%s: no sums: the statistics are off (%s with every >= 1 switches them on)", what,
                  ens ? "lbm_dstats_ens_set" : "lbm_dstats_set");
}

static inline int stats_refuse_steady(const char *what) {
  return lbm_fail(LBM_ERR_ARG, "%s: the running statistics are on (lbm_dstats_ens_set): a member that stops would need a gated sample "
                  "kernel, which is out of scope; lbm_dstats_ens_set(e, 0) switches them off for a steady run", what);
}

static inline int stats_refuse_plan(int first, int origin) {
  return lbm_fail(LBM_ERR_STATE, "the statistics' origin %d lies beyond the step count %d of this run", origin, first);
}

}  // namespace lbm_host

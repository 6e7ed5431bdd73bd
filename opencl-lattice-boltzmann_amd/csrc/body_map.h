// Body maps of the double-precision contexts and ensembles (include/lbm.h: "Drag of a body", lbm_dbody_*): the host side
// of the byte a cell has in the device mask, shared by lbm_dp.cpp and lbm_dens.cpp.
//
//   0  fluid        1  blocked, its links count in the force        2  blocked, outside the body
//
// Every kernel but the four places that decide whether a cell's force counts tests the byte against 0, so 1 and 2 are the
// same cell to collision, acceleration, fields and av_vels.  The host keeps the 0 / 1 map it made of the caller's obstacle
// map (`blocked`) and the map of counted cells (`counted`, empty: every blocked cell); the device mask is rewritten from the
// two, never read back.
//
// Open boundaries (include/lbm.h, "Open boundaries"): while they are on, the blocked cells of columns 0 and nx - 1 are outside
// every body, byte 2, so that no link across the x wrap enters a force.  The host's two maps do not change with the setting:
// lbm_dbody_get returns the caller's body.
#pragma once
#include "host_common.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace lbm_host {

struct BodyMap {
  std::vector<uint8_t> blocked;   // [members][ny][nx], 1 where the obstacle map is non-zero
  std::vector<uint8_t> counted;   // [members][ny][nx], 1 where a blocked cell is in the body; empty: every blocked cell
};

// the obstacle map as uploaded (upload_mask's bytes): every blocked cell counts again
inline void body_reset(BodyMap &b, const int32_t *obstacles, size_t count) {
  b.blocked.resize(count);
  for (size_t i = 0; i < count; i++) b.blocked[i] = obstacles[i] != 0;
  b.counted.clear();
}

// The device bytes of the two maps; `open`: the column rule of open boundaries
inline std::vector<uint8_t> body_bytes(const std::vector<uint8_t> &blocked, const std::vector<uint8_t> &counted, int nx, bool open) {
  std::vector<uint8_t> bytes(blocked.size());
  for (size_t i = 0; i < bytes.size(); i++) {
    const int x = (int)(i % (size_t)nx);
    const bool counts = (counted.empty() || counted[i]) && !(open && (x == 0 || x == nx - 1));
    bytes[i] = blocked[i] ? (counts ? 1 : 2) : 0;
  }
  return bytes;
}

// The device mask once more from the host's maps: open boundaries went on or off, or an obstacle map arrived while they are on
inline int body_rewrite(const BodyMap &b, uint8_t *mask, int nx, bool open) {
  const std::vector<uint8_t> bytes = body_bytes(b.blocked, b.counted, nx, open);
  HIP_TRY(hipMemcpy(mask, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
  return LBM_OK;
}

// lbm_dbody_set / lbm_dbody_ens_set after their own checks: body == NULL is "every blocked cell".  A non-zero entry on a
// fluid cell is refused before anything changes, on the host or on the device.  `members` grids of ny x nx; the message
// names the first such cell, with its member for an ensemble.
inline int body_apply(BodyMap &b, uint8_t *mask, const int32_t *body, int members, int ny, int nx, bool ensemble, bool open) {
  const size_t per = (size_t)nx * ny, count = per * members;
  if (!body) {
    const std::vector<uint8_t> bytes = body_bytes(b.blocked, std::vector<uint8_t>(), nx, open);
    HIP_TRY(hipMemcpy(mask, bytes.data(), count, hipMemcpyHostToDevice));
    b.counted.clear();
    return LBM_OK;
  }
  for (size_t i = 0; i < count; i++)
    if (body[i] != 0 && !b.blocked[i]) {
      const int m = (int)(i / per), y = (int)((i % per) / nx), x = (int)(i % nx);
      if (ensemble)
        return lbm_fail(LBM_ERR_ARG, "body is non-zero on a fluid cell: member %d, y %d, x %d (a body is made of blocked cells)", m,
                        y, x);
      return lbm_fail(LBM_ERR_ARG, "body is non-zero on a fluid cell: y %d, x %d (a body is made of blocked cells)", y, x);
    }
  std::vector<uint8_t> counted(count);
  for (size_t i = 0; i < count; i++) counted[i] = b.blocked[i] && body[i] != 0;
  const std::vector<uint8_t> bytes = body_bytes(b.blocked, counted, nx, open);
  HIP_TRY(hipMemcpy(mask, bytes.data(), count, hipMemcpyHostToDevice));
  b.counted.swap(counted);
  return LBM_OK;
}

// lbm_dwall_set / lbm_dwall_ens_set after their own checks (include/lbm.h, "Moving walls"): every entry of the two velocity
// maps is finite, and zero (of either sign) on a fluid cell, as a body is refused there.  Nothing is changed; the message names
// the first such cell, with its member for an ensemble.
inline int wall_check(const BodyMap &b, const double *u_x, const double *u_y, int members, int ny, int nx, bool ensemble) {
  const size_t per = (size_t)nx * ny, count = per * members;
  for (size_t i = 0; i < count; i++) {
    const bool finite = std::isfinite(u_x[i]) && std::isfinite(u_y[i]);
    if (finite && (b.blocked[i] || (u_x[i] == 0.0 && u_y[i] == 0.0))) continue;
    const int m = (int)(i / per), y = (int)((i % per) / nx), x = (int)(i % nx);
    const char *what = finite ? "is non-zero on a fluid cell" : "is not finite";
    const char *why = finite ? " (a wall is made of blocked cells)" : "";
    if (ensemble)
      return lbm_fail(LBM_ERR_ARG, "the wall velocity %s: member %d, y %d, x %d, (%g, %g)%s", what, m, y, x, u_x[i], u_y[i], why);
    return lbm_fail(LBM_ERR_ARG, "the wall velocity %s: y %d, x %d, (%g, %g)%s", what, y, x, u_x[i], u_y[i], why);
  }
  return LBM_OK;
}

// lbm_dbody_get / lbm_dbody_ens_get: 1 where a blocked cell counts, else 0
inline void body_read(const BodyMap &b, int32_t *body_out) {
  for (size_t i = 0; i < b.blocked.size(); i++) body_out[i] = b.counted.empty() ? b.blocked[i] : b.counted[i];
}

}  // namespace lbm_host

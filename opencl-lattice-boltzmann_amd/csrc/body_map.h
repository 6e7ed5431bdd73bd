// Body maps of the double-precision contexts and ensembles (include/lbm.h: "Drag of a body", lbm_dbody_*): the host side
// of the byte a cell has in the device mask, shared by lbm_dp.cpp and lbm_dens.cpp.
//
//   0  fluid        1  blocked, its links count in the force        2  blocked, outside the body
//
// Every kernel but the four places that decide whether a cell's force counts tests the byte against 0, so 1 and 2 are the
// same cell to collision, acceleration, fields and av_vels.  The host keeps the 0 / 1 map it made of the caller's obstacle
// map (`blocked`) and the map of counted cells (`counted`, empty: every blocked cell); the device mask is rewritten from the
// two, never read back.
#pragma once
#include "host_common.h"

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

// lbm_dbody_set / lbm_dbody_ens_set after their own checks: body == NULL is "every blocked cell".  A non-zero entry on a
// fluid cell is refused before anything changes, on the host or on the device.  `members` grids of ny x nx; the message
// names the first such cell, with its member for an ensemble.
inline int body_apply(BodyMap &b, uint8_t *mask, const int32_t *body, int members, int ny, int nx, bool ensemble) {
  const size_t per = (size_t)nx * ny, count = per * members;
  if (!body) {
    b.counted.clear();
    HIP_TRY(hipMemcpy(mask, b.blocked.data(), count, hipMemcpyHostToDevice));
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
  std::vector<uint8_t> counted(count), bytes(count);
  for (size_t i = 0; i < count; i++) {
    counted[i] = b.blocked[i] && body[i] != 0;
    bytes[i] = b.blocked[i] ? (counted[i] ? 1 : 2) : 0;
  }
  HIP_TRY(hipMemcpy(mask, bytes.data(), count, hipMemcpyHostToDevice));
  b.counted.swap(counted);
  return LBM_OK;
}

// lbm_dbody_get / lbm_dbody_ens_get: 1 where a blocked cell counts, else 0
inline void body_read(const BodyMap &b, int32_t *body_out) {
  for (size_t i = 0; i < b.blocked.size(); i++) body_out[i] = b.counted.empty() ? b.blocked[i] : b.counted[i];
}

}  // namespace lbm_host

// The CORE stretch of a sweep of the deep window kernels (d2q9_deep / d2q9_deep_twin, see deep_sweep in d2q9_kernels.h) —
// free of HIP types, so that a wave computes it once per sweep on the device and tests/cpu/core_interval_test.cpp checks it
// by brute force on a CPU-only box.
//
// Level 0 of a sweep over the chunk [ys, ye) works on row r0 + k*d in iteration k, level l on row r0 + (k-l)*d.  What the
// steady row loop decides per level and per row — is the level's row one of the chunk's own, is it the accelerated row, do
// the rows it loads and stores wrap — is the same for a whole range of iterations in a chunk's interior: the CORE form of
// the loop runs that range without the tests.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LBM_CORE_HD __host__ __device__ inline
#else
#define LBM_CORE_HD inline
#endif

namespace lbm {

struct CoreInterval {
  int kc0, kc1;  // row iterations [kc0, kc1); kc0 == kc1: none
};

// The longest interval [kc0, kc1) of row iterations k of the sweep (up: rows ascending; twinned: the wave starts at its own
// first row, see deep_sweep) over the chunk [ys, ye) at depth L on a grid of ny stored rows in which
//  (a) every level l < L works on one of the chunk's own rows: ys <= r0 + (k-l)*d < ye;
//  (b) no level's row is accel_row or accel_row_b — the last level counts only with accel_next (its output is the stored
//      state; deep_sweep's accmask);
//  (c) nothing wraps: the row loaded for iteration k+1, r0 + (k+1)*d, and its south and north neighbours lie in [0, ny),
//      and so does the row stored in iteration k, r0 + (k-L)*d;
//  (d) k >= k_steady = sf*(L-1) + 1: every level is running.
// Of several longest intervals the first.  Empty unless it has at least two iterations.
LBM_CORE_HD CoreInterval core_interval(int ys, int ye, int L, int ny, bool up, bool twinned, int accel_row, int accel_row_b,
                                       bool accel_next) {
  const int n = ye - ys, d = up ? 1 : -1;
  const int lead = twinned ? 0 : L - 1, sf = twinned ? 1 : 2;
  const int r0 = up ? ys - lead : ye - 1 + lead;
  const CoreInterval none = {0, 0};
  if (n <= 0 || L < 2) return none;
  // (a): lead <= k - (L-1) and k <= n + lead - 1; (d)
  int lo = lead + L - 1, hi = n + lead - 1;  // inclusive
  const int k_steady = sf * (L - 1) + 1;
  if (lo < k_steady) lo = k_steady;
  // (c): the stored row r0 + (k-L)*d is one of the chunk's own from k = lead + L on, which is k_steady for a lone wave
  // (2L - 1) and for a twin (L) alike, and the own rows lie in [0, ny).  The loaded row r = r0 + (k+1)*d needs
  // 1 <= r <= ny - 2: sweeping up r grows, sweeping down it falls.
  if (up) {
    const int kmax = (ny - 2 - r0) - 1;  // r0 + (k+1) <= ny - 2
    if (hi > kmax) hi = kmax;
    const int kmin = 1 - r0 - 1;         // r0 + (k+1) >= 1
    if (lo < kmin) lo = kmin;
  } else {
    const int kmax = (r0 - 1) - 1;       // r0 - (k+1) >= 1
    if (hi > kmax) hi = kmax;
    const int kmin = r0 - (ny - 2) - 1;  // r0 - (k+1) <= ny - 2
    if (lo < kmin) lo = kmin;
  }
  if (hi - lo + 1 < 2) return none;
  // (b): level l meets row A in iteration kA + l, where r0 + kA*d == A (inside [lo, hi] every level's row is an own row, so
  // the wrapped row is the row): iterations kA .. kA + Lacc - 1 are out.  Two such stretches at the most cut [lo, hi] into
  // three pieces.
  const int Lacc = accel_next ? L : L - 1;
  int c0[2], c1[2], nc = 0;  // excluded [c0, c1], sorted by c0
  const int arows[2] = {accel_row, accel_row_b};
  for (int i = 0; i < 2; i++) {
    const int A = arows[i];
    if (A < 0 || A >= ny || Lacc <= 0) continue;
    const int kA = (A - r0) * d;
    if (kA + Lacc - 1 < lo || kA > hi) continue;
    int j = nc++;
    if (j == 1 && kA < c0[0]) { c0[1] = c0[0]; c1[1] = c1[0]; j = 0; }
    c0[j] = kA;
    c1[j] = kA + Lacc - 1;
  }
  int best0 = 0, best1 = 0;  // [best0, best1)
  int start = lo;
  for (int i = 0; i <= nc; i++) {
    const int end = i < nc ? c0[i] : hi + 1;  // the piece [start, end)
    if (end - start > best1 - best0) { best0 = start; best1 = end; }
    if (i < nc && c1[i] + 1 > start) start = c1[i] + 1;
  }
  if (best1 - best0 < 2) return none;
  const CoreInterval r = {best0, best1};
  return r;
}

}  // namespace lbm

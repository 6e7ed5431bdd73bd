// Brute-force check of lbm::core_interval (csrc/core_interval.h): for every case, every iteration of the returned interval
// satisfies the four conditions the CORE form of deep_sweep's row loop relies on, stated here row by row as the kernel's
// general form states them, and no longer run of such iterations exists.  Plain g++, no HIP; tests/test_core_interval.py
// builds it with and without sanitizers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../opencl-lattice-boltzmann_amd/csrc/core_interval.h"

namespace {

long g_cases = 0, g_nonempty = 0, g_fail = 0;

int wrap_row(int r, int ny) {
  r %= ny;
  return r < 0 ? r + ny : r;
}

// the conditions for ONE iteration, as deep_sweep's general form evaluates them
bool core_ok(int k, int ys, int ye, int L, int ny, bool up, bool twinned, int A, int B, bool accel_next) {
  const int n = ye - ys, d = up ? 1 : -1;
  const int lead = twinned ? 0 : L - 1, sf = twinned ? 1 : 2;
  const int r0 = up ? ys - lead : ye - 1 + lead;
  const int last = n + lead + (L - 1) - 1;
  if (k < sf * (L - 1) + 1 || k + 1 > last) return false;  // (d); and the row of iteration k+1 is loaded
  for (int l = 0; l < L; l++) {
    const int row = r0 + (k - l) * d;
    if (row < ys || row >= ye) return false;                                 // (a)
    if (!(k - l >= lead && k - l <= n + lead - 1)) return false;             // (a) as ownbits has it
    if (l == L - 1 && !accel_next) continue;
    const int w = wrap_row(row, ny);
    if (w == A || w == B) return false;                                      // (b)
  }
  const int r = r0 + (k + 1) * d;
  if (r - 1 < 0 || r + 1 > ny - 1) return false;                             // (c) loads
  const int st = r0 + (k - L) * d;
  if (st < 0 || st >= ny) return false;                                      // (c) store
  return true;
}

void check(int ys, int ye, int L, int ny, bool up, bool twinned, int A, int B, bool accel_next) {
  g_cases++;
  const lbm::CoreInterval ci = lbm::core_interval(ys, ye, L, ny, up, twinned, A, B, accel_next);
  const int n = ye - ys, lead = twinned ? 0 : L - 1, last = n + lead + (L - 1) - 1;
  int best = 0, best0 = 0, run = 0;
  for (int k = 0; k <= last + 1; k++) {
    if (k <= last && core_ok(k, ys, ye, L, ny, up, twinned, A, B, accel_next)) {
      run++;
      if (run > best) { best = run; best0 = k - run + 1; }
    } else {
      run = 0;
    }
  }
  if (best < 2) best = 0;
  bool ok = ci.kc1 >= ci.kc0 && (ci.kc1 - ci.kc0) == best && (best == 0 || ci.kc0 == best0);
  for (int k = ci.kc0; ok && k < ci.kc1; k++) ok = core_ok(k, ys, ye, L, ny, up, twinned, A, B, accel_next);
  if (ci.kc1 > ci.kc0) g_nonempty++;
  if (!ok && g_fail++ < 20)
    std::printf("FAIL ys %d ye %d L %d ny %d up %d twinned %d accel %d %d next %d: got [%d, %d), longest valid run %d from %d\n", ys, ye, L,
                ny, (int)up, (int)twinned, A, B, (int)accel_next, ci.kc0, ci.kc1, best, best0);
}

}  // namespace

int main() {
  const int nys[] = {16, 17, 23, 64, 131, 300, 400};
  for (int ny : nys) {
    for (int L = 5; L <= 8; L++) {
      std::vector<int> lens;
      for (int n = 1; n <= 160 && n <= ny; n++) {
        // every length up to 2L + 2 (L-1, L, L+1 among them), then a thinning set that keeps odd and even ones, and the ends
        if (n <= 2 * L + 2 || n % 23 == 0 || n % 16 == 1 || n == 160 || n == ny) lens.push_back(n);
      }
      for (int n : lens) {
        const int starts[] = {0, 1, 2, (ny - n) / 2, ny - n - 2, ny - n - 1, ny - n};
        int prev = -1;
        for (int ys : starts) {
          if (ys < 0 || ys + n > ny || ys == prev) continue;
          prev = ys;
          const int ye = ys + n;
          // accelerated rows: none, the grid's ends, the usual ny-2, and every place relative to the chunk that matters
          const int acc[] = {-1, 0, 1, ny - 2, ny - 1, ys - L, ys - 1, ys, ys + 1, ys + L - 1, ys + L, ys + n / 2, ye - L - 1, ye - L,
                             ye - 2, ye - 1, ye, ye + L - 1, ny, ny + 3};
          for (int up = 0; up < 2; up++) {
            for (int tw = 0; tw < 2; tw++) {
              for (int nx = 0; nx < 2; nx++) {
                for (int A : acc) {
                  if (A < -1) continue;
                  check(ys, ye, L, ny, up != 0, tw != 0, A, -1, nx != 0);
                  // two copies: with every other place on chunks of 2L .. 2L + 2 rows, with three places on the others
                  for (int B : acc) {
                    if (B < 0 || B == A || ((n < 2 * L || n > 2 * L + 2) && B != ys + n / 2 && B != ye - 2 && B != ys + 1)) continue;
                    check(ys, ye, L, ny, up != 0, tw != 0, A, B, nx != 0);
                  }
                }
              }
            }
          }
        }
      }
    }
  }
  // the headline grid's chunks: 8192 rows, eight levels, row 8190 accelerated
  for (int n : {96, 64, 32, 24, 8}) {
    for (int ys : {0, 1024, 8192 - 2 * n, 8192 - n}) {
      for (int up = 0; up < 2; up++) {
        for (int tw = 0; tw < 2; tw++) check(ys, ys + n, 8, 8192, up != 0, tw != 0, 8190, -1, true);
      }
    }
  }
  {
    // an interior chunk of a pair: every iteration from lead + L - 1 to n + lead - 1
    const lbm::CoreInterval ci = lbm::core_interval(1024, 1120, 8, 8192, true, true, 8190, -1, true);
    if (ci.kc0 != 8 || ci.kc1 != 96) { std::printf("FAIL interior twin: [%d, %d)\n", ci.kc0, ci.kc1); g_fail++; }
    const lbm::CoreInterval cl = lbm::core_interval(1024, 1120, 8, 8192, false, false, 8190, -1, true);
    if (cl.kc0 != 15 || cl.kc1 != 103) { std::printf("FAIL interior lone: [%d, %d)\n", cl.kc0, cl.kc1); g_fail++; }
  }
  std::printf("core_interval_test: %ld cases, %ld with an interval, %ld failures\n", g_cases, g_nonempty, g_fail);
  if (g_fail || g_nonempty == 0 || g_nonempty == g_cases) return 1;
  std::printf("core_interval_test: ok\n");
  return 0;
}

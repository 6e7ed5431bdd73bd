// Planner of the strips x chunks schedules of the window kernels (d2q9_step2 ... d2q9_deep_twin) — free of HIP types so
// that the tables can be checked on a CPU-only box (tests/cpu/chunk_schedule_test.cpp).  fuse_schedule (lbm_hip.cpp)
// uploads what plan_chunks returns.
//
// A unit's cost is proportional to its rows + its start-up iterations, and all units of a launch finish at about the same
// time, so equal chunks leave the chip partly idle during the last round of units (17 % of the launch with 32-row chunks
// on 8192x8192).  The schedule therefore tapers: every band (the share of one XCD) starts with chunks of `cmax` rows and
// ends with ever shorter ones (guided self-scheduling), down to `cmin`.  (R full rounds of equal chunks instead of the
// taper: within +-2 % on 8192x1024 ... 8192x8192, no consistent sign — not adopted.)
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

namespace lbm {

// Taper of a multi-round PAIR schedule, in 1/32: a pair takes rem / (kPairTaper32 / 32 * resident pair workgroups per band
// and strip) rows.  37/32 x the headline grid's 1.73 resident pairs = 2: each chunk a quarter of what is left, which is
// what the chunk-by-chunk rule gave the FIRST chunk of every pair.  Alternating sweep on one 8192x8192 context, us/step, mean
// of five rounds (profiles/pair_taper_ab.txt): chunk by chunk 155.7; taper 28 / 37 / 48 with first chunks <= 96 and a floor of
// 24 rows 153.1 / 153.2 / 155.1, floor 16 153.4 / 154.0 / 155.4, first chunks <= 128 156.2 / 154.1 / 155.0, <= 160 156.4 /
// 154.9 / 157.1 -> 37 with the 96 / 24 rows the schedules had (28 is not told apart from it).  bench.py, five alternating
// runs: 467.2-471.5 -> 472.0-481.7 GLUPS (400 steps), 429.2-438.2 -> 439.4-447.3 (20 steps); 6144x6144 432.7-436.2 -> 439.3-448.1.
constexpr int kPairTaper32 = 37;

struct ChunkPlan {
  int nbands = 1;
  int chunks_per_band = 0;
  bool single_round = false;  // all units of the launch are resident at once (equal chunks)
  std::vector<int> starts;    // [nbands * chunks_per_band + 1], first r0, last r0 + rows
};

inline void split_rows(int ny, int P, int idx, int *y0, int *rows) {
  const int base = ny / P, rem = ny % P;
  *y0 = idx * base + std::min(idx, rem);
  *rows = base + (idx < rem ? 1 : 0);
}

// The chunk-pair kernels (d2q9_step3p / d2q9_step4p / d2q9_deep_twin) hold the LDS of BOTH chunks of a pair until the
// longer one is done, so a one-round schedule needs an EVEN number of chunks per band that still fits the wave slots: 7.3
// slots per band means 6 chunks with 8 bands (82 % of the slots) but 14 with 4 bands (96 %) — take the band count that
// keeps most waves busy, preferring more bands (neighbouring strips then share an XCD's L2).
// (the same choice for d2q9_deep, unpaired: 4096x4096 has 6.9 slots per band and strip with 8 bands — 6 chunks, 87 % of
// the slots, 85 rows + 14 start-up iterations each — but 55 per strip with one band: 75 rows + 14)
inline int plan_bands(int rows, int strips, int waves_resident, int cmax_one, bool pairs) {
  int best_nb = 8;
  double best = -1.0;
  for (int nb = 8; nb >= 1; nb /= 2) {
    const int fl = pairs ? std::max(2, (int)std::floor((double)waves_resident / nb / strips) & ~1)
                         : std::max(1, (int)std::floor((double)waves_resident / nb / strips));
    const int nrows = (rows + nb - 1) / nb;
    if ((int)std::ceil((double)nrows / fl) > cmax_one) continue;  // not a one-round schedule with this band count
    const double busy = (double)std::min(fl, nrows) * nb * (1.0 + 0.01 * nb);
    if (busy > best) { best = busy; best_nb = nb; }
  }
  return best_nb;
}

// Chunk table over rows [r0, r0 + rows) for `strips` strips on `waves_resident` wave slots.  cmax / cmin bound a chunk of a
// tapered (multi-round) table, cmax_one the equal chunks of a one-round table; flex_bands: search the band count also for an
// unpaired schedule (d2q9_deep); pair_taper32: see kPairTaper32, 0 = size a pair schedule's chunks one by one (the rule of the
// unpaired schedules, which pair schedules had too before the pair taper).
inline ChunkPlan plan_chunks(int rows, bool allow_bands, int strips, int waves_resident, int cmax, int cmin, int cmax_one,
                             bool pairs, bool flex_bands = false, int r0 = 0, int pair_taper32 = kPairTaper32) {
  ChunkPlan g;
  if (cmax_one < cmax) cmax_one = cmax;  // longest chunk of a ONE-round schedule (d2q9_deep: longer than the tapered schedules' first chunks)
  g.nbands = (allow_bands && rows >= 8 * 4 * cmin) ? 8 : 1;
  if ((pairs || flex_bands) && g.nbands == 8) g.nbands = plan_bands(rows, strips, waves_resident, cmax_one, pairs);
  double slots = std::max(1.0, (double)waves_resident / g.nbands / strips);  // concurrent chunks per band
  if (pairs) slots = std::max(2.0, (double)((int)std::floor(slots) & ~1));
  for (int b = 0; b < g.nbands; b++) {
    int y0, n;
    split_rows(rows, g.nbands, b, &y0, &n);
    std::vector<int> sizes;
    int rem = n;
    // a grid small enough to be done in ONE round of units (all of them resident at once) gets equal chunks
    // that just fill the wave slots: every extra unit costs two redundant rows, and a second, partly filled
    // round costs more than it balances (1024x1024: 3-row chunks = 1720 units: 10.2 us/step; 2-row chunks =
    // 2560 units: 12.1; 4-row chunks = 1280 units: 11.6 — tools/ab.py)
    const int one_round = (int)std::ceil(n / std::max(1.0, std::floor(slots)));
    // (one round only if the units really are resident at once: a pair schedule needs two slots per band and strip —
    // with fewer, "one round" of 64-row chunks was 2192 units on 1500 free slots and the last workgroups started when the
    // first had finished: compact 8192x1024 slab 212 instead of 220 GLUPS)
    const bool fits = (double)waves_resident / g.nbands / strips >= (pairs ? 2.0 : 1.0);
    const bool single_round = one_round <= cmax_one && fits;
    if (b == 0) g.single_round = single_round;
    if (pairs && !single_round && pair_taper32 > 0) {
      // Several rounds of chunk PAIRS: a pair workgroup lasts as long as its longer chunk, whatever the shorter one is, and
      // nothing takes the retired wave's slot (the LDS is held for both).  So the guided rule sizes the PAIR — from the
      // resident pair workgroups per band and strip as they are, not floored to an even wave count — and both chunks get
      // half of it; a band ends with a whole pair.  8192x8192, per band: (96,96) x4, (64,64), (32,32), (24,24), (8,8) = 568
      // workgroup-iterations instead of the 591 of (96,96) x3, (96,88), (66,50), (37,28), (24,24), (24,11).
      const long num = 64L * g.nbands * strips, den = (long)waves_resident * pair_taper32;
      while (rem > 0) {
        long two = (rem * num + den - 1) / den;
        two = std::max(2L * cmin, std::min(2L * cmax, two));
        two = std::min<long>(two, rem);
        sizes.push_back((int)((two + 1) / 2));
        sizes.push_back((int)(two / 2));
        rem -= (int)two;
      }
    } else {
      while (rem > 0) {
        int sz = single_round ? std::max(2, one_round) : (int)std::ceil(rem / (2.0 * slots));
        if (!single_round) sz = std::max(cmin, std::min(cmax, sz));
        sz = std::min(sz, rem);
        sizes.push_back(sz);
        rem -= sz;
      }
    }
    // all bands need the same number of chunks (unit arithmetic in the kernel): band 0 is never
    // shorter than the others (split_rows); pad with empty chunks / merge surplus into the last one
    // (an even count for the chunk-pair kernels, which pair chunks 2p and 2p+1)
    if (b == 0) g.chunks_per_band = pairs ? ((int)sizes.size() + 1) / 2 * 2 : (int)sizes.size();
    while ((int)sizes.size() < g.chunks_per_band) sizes.push_back(0);
    int extra = 0;
    while ((int)sizes.size() > g.chunks_per_band) { extra += sizes.back(); sizes.pop_back(); }
    if (extra) {
      sizes.back() += extra;
      if (pairs && !single_round && pair_taper32 > 0) {  // keep the last pair's halves equal
        const int k = (int)sizes.size(), two = sizes[k - 2] + sizes[k - 1];
        sizes[k - 2] = (two + 1) / 2;
        sizes[k - 1] = two / 2;
      }
    }
    int y = r0 + y0;
    for (int sz : sizes) { g.starts.push_back(y); y += sz; }
  }
  g.starts.push_back(r0 + rows);
  return g;
}

}  // namespace lbm

// CPU-side test of csrc/chunk_schedule.h (tests/test_chunk_schedule.py compiles and runs it with g++, once plain and once
// under AddressSanitizer + UBSan; no HIP).  Without arguments it checks the invariants of the chunk tables over a fixed set of
// cases; with `--table rows allow_bands strips waves_resident cmax cmin cmax_one pairs flex_bands r0 pair_taper32` it prints
// one table as a JSON line, which the Python side compares with the recorded tables under tests/golden/schedule/.
#include "../../opencl-lattice-boltzmann_amd/csrc/chunk_schedule.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using lbm::ChunkPlan;

static int failures = 0;
static const char *g_case = "";
#define EXPECT(cond)                                                                        \
  do {                                                                                      \
    if (!(cond)) { printf("FAILED line %d [%s]: %s\n", __LINE__, g_case, #cond); failures++; } \
  } while (0)

// sum over the pairs of band 0 of what a pair workgroup lasts: its longer chunk + the L - 1 = 7 start-up iterations of the
// eight-step kernel
static int pair_cost(const ChunkPlan &g) {
  int sum = 0;
  for (int k = 0; k + 1 < g.chunks_per_band; k += 2) {
    const int n0 = g.starts[k + 1] - g.starts[k], n1 = g.starts[k + 2] - g.starts[k + 1];
    if (n0 + n1 > 0) sum += std::max(n0, n1) + 7;
  }
  return sum;
}

static void check(int rows, int strips, int waves, int cmax, int cmin, int cmax_one, bool pairs, bool flex, int r0, int taper) {
  static char name[160];
  snprintf(name, sizeof name, "%d rows x %d strips, %d waves, chunks %d/%d one-round %d, pairs %d flex %d r0 %d taper %d", rows, strips,
           waves, cmax, cmin, cmax_one, pairs, flex, r0, taper);
  g_case = name;
  const ChunkPlan g = lbm::plan_chunks(rows, true, strips, waves, cmax, cmin, cmax_one, pairs, flex, r0, taper);
  const int one = std::max(cmax, cmax_one), cpb = g.chunks_per_band;
  EXPECT(g.nbands == 1 || g.nbands == 2 || g.nbands == 4 || g.nbands == 8);
  EXPECT(cpb >= 1);
  // every band has the same chunk count (an even one for pairs), and the table covers [r0, r0 + rows) exactly
  EXPECT((int)g.starts.size() == g.nbands * cpb + 1);
  if ((int)g.starts.size() != g.nbands * cpb + 1) return;
  if (pairs) EXPECT(cpb % 2 == 0);
  EXPECT(g.starts.front() == r0 && g.starts.back() == r0 + rows);
  for (size_t i = 0; i + 1 < g.starts.size(); i++) EXPECT(g.starts[i] <= g.starts[i + 1]);
  const bool tapered_pairs = pairs && !g.single_round && taper > 0;
  for (int b = 0; b < g.nbands; b++) {
    int y0, n;
    lbm::split_rows(rows, g.nbands, b, &y0, &n);
    const int *st = &g.starts[(size_t)b * cpb];
    EXPECT(st[0] == r0 + y0 && st[cpb] == r0 + y0 + n);
    int prev_pair = 1 << 30;
    for (int k = 0; k < cpb; k++) {
      const int sz = st[k + 1] - st[k], left = r0 + y0 + n - st[k];
      EXPECT(sz <= (g.single_round ? one : cmax));
      // the floor belongs to the tapered tables (a one-round table has equal chunks of rows / slots, whatever cmin is); the
      // last pair of a band (the last chunk of an unpaired one) takes what is left
      const bool last = pairs ? st[k / 2 * 2 + 2] == st[cpb] : st[k + 1] == st[cpb];
      if (!g.single_round && !last) EXPECT(sz >= std::min(cmin, left));
      if (pairs && k % 2 == 0) {
        const int n0 = sz, n1 = st[k + 2] - st[k + 1];
        EXPECT(n0 + n1 <= prev_pair);  // pair sizes do not increase along a band
        prev_pair = n0 + n1;
        if (tapered_pairs) {
          EXPECT(std::abs(n0 - n1) <= 1);
          if ((n0 == 0) != (n1 == 0)) EXPECT(n0 + n1 < 2);  // one empty chunk only where fewer than 2 rows were left
        }
      }
    }
  }
}

static int table(char **a) {
  const ChunkPlan g = lbm::plan_chunks(atoi(a[0]), atoi(a[1]) != 0, atoi(a[2]), atoi(a[3]), atoi(a[4]), atoi(a[5]), atoi(a[6]), atoi(a[7]) != 0,
                                       atoi(a[8]) != 0, atoi(a[9]), atoi(a[10]));
  printf("{\"nbands\": %d, \"chunks_per_band\": %d, \"single_round\": %s, \"starts\": [", g.nbands, g.chunks_per_band,
         g.single_round ? "true" : "false");
  for (size_t i = 0; i < g.starts.size(); i++) printf("%s%d", i ? ", " : "", g.starts[i]);
  printf("]}\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 13 && std::string(argv[1]) == "--table") return table(argv + 2);
  if (argc != 1) {
    printf("usage: %s [--table rows allow_bands strips waves_resident cmax cmin cmax_one pairs flex_bands r0 pair_taper32]\n", argv[0]);
    return 2;
  }
  struct Case { int rows, strips, cmax, cmin; };
  const Case cases[] = {{8192, 74, 96, 24}, {8191, 74, 96, 24}, {4104, 5, 8, 4}, {8192, 78, 96, 24}, {600, 5, 8, 4}, {7, 1, 8, 4}};
  for (const Case &c : cases)
    for (int waves : {2048, 1024})
      for (int pairs = 0; pairs < 2; pairs++)
        for (int flex = 0; flex < 2; flex++)
          for (int cmax_one : {0, 160})          // 0: as long as a tapered schedule's first chunks
            for (int r0 : {0, 8})
              for (int taper : {lbm::kPairTaper32, 0, 24, 32, 48, 64})
                check(c.rows, c.strips, waves, c.cmax, c.cmin, cmax_one && c.cmax < 96 ? 0 : cmax_one, pairs != 0, flex != 0, r0, taper);

  // the headline grid (8192x8192: 74 strips, 2048 wave slots, chunks of 96 ... 24 rows, one-round chunks up to 160) stays a
  // tapered schedule of 8 bands, and its pairs cost fewer workgroup-iterations than the chunk-by-chunk table
  g_case = "headline";
  const ChunkPlan now = lbm::plan_chunks(8192, true, 74, 2048, 96, 24, 160, true, true);
  const ChunkPlan was = lbm::plan_chunks(8192, true, 74, 2048, 96, 24, 160, true, true, 0, 0);
  EXPECT(!now.single_round && now.nbands == 8 && !was.single_round && was.nbands == 8);
  const int was_sizes[16] = {96, 96, 96, 96, 96, 96, 96, 88, 66, 50, 37, 28, 24, 24, 24, 11};
  EXPECT(was.chunks_per_band == 16);
  for (int k = 0; k < 16 && was.chunks_per_band == 16; k++) EXPECT(was.starts[k + 1] - was.starts[k] == was_sizes[k]);
  EXPECT(pair_cost(was) == 591);
  EXPECT(pair_cost(now) < pair_cost(was));
  printf("headline: %d chunks per band, pair cost %d (chunk by chunk: %d chunks, %d)\n", now.chunks_per_band, pair_cost(now),
         was.chunks_per_band, pair_cost(was));
  if (failures) {
    printf("chunk_schedule_test: %d FAILED\n", failures);
    return 1;
  }
  printf("chunk_schedule_test: ok\n");
  return 0;
}

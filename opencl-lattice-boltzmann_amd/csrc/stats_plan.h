// Running statistics (include/lbm.h, "Running statistics"): where a run is cut.  No HIP in here: lbm_dp.cpp and lbm_dens.cpp call
// it, and tests/cpu/stats_plan_test.cpp compiles it with g++ alone.
//
// A run of `nsteps` steps from step count `first` is cut at the sample points s = origin + j * every, j >= 1, that lie in
// (first, first + nsteps]: each piece ends on a sample point, but for the last one, which ends where the run ends.  A sample
// point at `first` itself belongs to the run that reached it.  Every piece is enqueued the way a run of its length is.
#pragma once
#include <vector>

namespace lbm_host {

struct StatsPiece {
  int len;       // steps, >= 1
  bool sample;   // the piece ends on a sample point
};

// The pieces in order; they sum to nsteps.  every == 0 (statistics off): one piece without a sample, the run as it is without
// statistics; nsteps == 0: no piece.  false, and no pieces: first, nsteps or every negative, or statistics on with an origin
// beyond `first` (an origin is the step count at which the statistics started, which no later run starts before).
inline bool stats_plan(int first, int nsteps, int origin, int every, std::vector<StatsPiece> &pieces) {
  pieces.clear();
  if (first < 0 || nsteps < 0 || every < 0) return false;
  if (every > 0 && (origin < 0 || origin > first)) return false;
  if (nsteps == 0) return true;
  if (every == 0) {
    pieces.push_back(StatsPiece{nsteps, false});
    return true;
  }
  const long end = (long)first + nsteps;
  long next = origin + ((long)(first - origin) / every + 1) * every;   // the first sample point beyond `first`
  for (long at = first; at < end;) {
    const long to = next < end ? next : end;
    pieces.push_back(StatsPiece{(int)(to - at), to == next});
    if (to == next) next += every;
    at = to;
  }
  return true;
}

}  // namespace lbm_host

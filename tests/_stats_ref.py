"""The running statistics (include/lbm.h, "Running statistics") restated in Python: where a run is cut (csrc/stats_plan.h) and
what a sample adds.  The accumulation is `acc = acc + v` per sample in numpy float64, one IEEE operation per written operator, on
fields that come from final_state() of a handle WITHOUT statistics: the output stage that the existing tests pin, not the code
under test."""
import numpy as np


def sample_points(first, nsteps, origin, every):
    """the step counts s = origin + j * every, j >= 1, in (first, first + nsteps]"""
    if every == 0:
        return []
    return [s for s in range(first + 1, first + nsteps + 1) if s > origin and (s - origin) % every == 0]


def plan(first, nsteps, origin, every):
    """[(length, ends_on_a_sample)] of a run of nsteps from step count first, or None where the plan is refused: a negative
    argument, or statistics on with an origin beyond first"""
    if first < 0 or nsteps < 0 or every < 0:
        return None
    if every > 0 and (origin < 0 or origin > first):
        return None
    pieces, at = [], first
    for s in sample_points(first, nsteps, origin, every):
        pieces.append((s - at, True))
        at = s
    if at < first + nsteps:
        pieces.append((first + nsteps - at, False))
    return pieces


def plan_text(first, nsteps, origin, every):
    """the line tests/cpu/stats_plan_test.cpp prints for this row of its table"""
    pieces = plan(first, nsteps, origin, every)
    body = "refused" if pieces is None else " ".join("%d%s" % (n, "*" if mark else "") for n, mark in pieces)
    return ("%d %d %d %d: %s" % (first, nsteps, origin, every, body)).rstrip()


class Sums:
    """six planes of sums and a count, of any leading shape"""

    def __init__(self, shape):
        self.S = np.zeros((6,) + tuple(shape), dtype=np.float64)
        self.samples = 0

    def add(self, u_x, u_y, pressure):
        """one sample: the header's six statements"""
        S = self.S
        S[0] = S[0] + u_x
        S[1] = S[1] + u_y
        S[2] = S[2] + pressure
        S[3] = S[3] + u_x * u_x
        S[4] = S[4] + u_y * u_y
        S[5] = S[5] + u_x * u_y
        self.samples += 1

    def sums(self):
        """in the layout of stats_sums(): [6, ny, nx], an ensemble's [n, 6, ny, nx]"""
        return self.S if self.S.ndim == 3 else np.ascontiguousarray(np.moveaxis(self.S, 0, 1))


def twin_sums(twin, runs, origin, every):
    """`twin`: a handle of the settings under test with statistics OFF, at step count `origin`.  Advances it through `runs`
    (the lengths of the runs under test) piece by piece, reads final_state() at every sample point and accumulates.  The twin
    ends where the handle under test ends."""
    fields = twin.final_state()
    acc = Sums(np.shape(fields[0]))
    first = twin.steps_done
    for nsteps in runs:
        for length, mark in plan(first, nsteps, origin, every):
            twin.run(length)
            if mark:
                u_x, u_y, _, pressure = twin.final_state()
                acc.add(u_x, u_y, pressure)
        first += nsteps
    return acc

#!/usr/bin/env python3
"""tools/schedule_model.py — what a chunk table of the window kernels costs, before a GPU run.

    python tools/schedule_model.py tests/golden/schedule/deep_8192x8192_pairs.json
    chunk_schedule_test --table 8192 1 74 2048 96 24 160 1 1 0 37 | python tools/schedule_model.py - --strips 74 --pairs 1

Reads one table as tests/cpu/chunk_schedule_test.cpp --table prints it (or a record of tests/golden/schedule/, which also
names its strips and whether it is a pair schedule) and list-schedules the workgroups of ONE band, in launch order (chunk
or chunk pair major, strip minor: select_unit in csrc/d2q9_kernels.h), onto the slots one XCD offers: a unit lasts its rows +
start-up iterations, a pair workgroup as long as its longer chunk (the LDS of both is held).  Prints the summed
workgroup-iterations per band and strip, the makespan in iterations and the floor (no start-up rows, perfect balance).

A model of issue-bound waves that all run at one speed: it ignores that a wave speeds up a little when its SIMD neighbour
retires and what the caches do.  Good for ranking tables (profiles/pair_taper_ab.txt sets it against measurements), not
for predicting a time."""
import argparse
import heapq
import json
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("table", help="JSON file, or - for stdin")
    ap.add_argument("--strips", type=int, default=0, help="strips per row (default: the record's args.strips)")
    ap.add_argument("--pairs", type=int, default=-1, help="1: chunks 2p / 2p+1 are one workgroup (default: the record's args.pairs)")
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--levels", type=int, default=8, help="timesteps per launch L: start-up L-1 iterations for a pair, 2(L-1) for a lone chunk")
    ap.add_argument("--wall", type=float, default=1.3, help="cost per row of the first and the last strip (a cavity's wall strips)")
    ap.add_argument("--dispatch", type=float, default=0.0, help="fixed iterations every workgroup pays on top")
    a = ap.parse_args()
    rec = json.load(sys.stdin if a.table == "-" else open(a.table))
    args = rec.get("args", {})
    strips = a.strips or args.get("strips", 0)
    pairs = bool(a.pairs if a.pairs >= 0 else args.get("pairs", 0))
    if strips <= 0:
        sys.exit("--strips is needed for a bare table")
    nb, cpb, st = rec["nbands"], rec["chunks_per_band"], rec["starts"]
    sizes = [st[k + 1] - st[k] for k in range(cpb)]   # band 0 (never shorter than the others)
    # a CU holds 8 waves of these kernels (2 per SIMD) = 4 pair workgroups; the bands of a launch share the device evenly
    slots = a.cus * (4 if pairs else 8) // nb
    if pairs:
        wgs = [(max(sizes[k], sizes[k + 1]), sizes[k] + sizes[k + 1]) for k in range(0, cpb, 2)]
        start = a.levels - 1
    else:
        wgs = [(n, n) for n in sizes]
        start = 2 * (a.levels - 1)
    wgs = [w for w in wgs if w[1] > 0]
    per_strip = sum(n + start for n, _ in wgs)
    free = []   # times at which slots become free
    t_end, started = 0.0, 0
    for n, _ in wgs:
        for s in range(strips):
            cost = (n + start) * (a.wall if s in (0, strips - 1) else 1.0) + a.dispatch
            t0 = heapq.heappop(free) if started >= slots else 0.0
            started += 1
            heapq.heappush(free, t0 + cost)
            t_end = max(t_end, t0 + cost)
    rows = sum(sizes)
    floor = rows * (strips - 2 + 2 * a.wall) / (slots * (2 if pairs else 1))
    print("%d band(s), %d chunks per band%s, %d strips, %d slots per band: chunks of band 0 %s" % (
        nb, cpb, " (pairs)" if pairs else "", strips, slots, sizes))
    print("workgroup-iterations per band and strip %d, makespan %.0f iterations, floor %.0f" % (per_strip, t_end, floor))


if __name__ == "__main__":
    main()

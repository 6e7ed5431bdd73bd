#!/usr/bin/env python3
"""tools/isa_stats.py [--path] [file.s] [name-filter ...] — instruction mix of the step kernels from the gfx950 assembly.

Without a file it compiles the library's two translation units to assembly first (hipcc -S --cuda-device-only, ~1 min).  For every
kernel whose mangled name contains one of the filters (default: the default template instances of the multi-step
kernels) it prints registers / LDS / spills from the metadata and the instruction classes of (a) the whole kernel
and (b) its loops — the blocks the compiler's comments assign to each loop header — ordered by arithmetic content: the row
loops of the two sweep directions, in their general (start-up) and steady forms.
With --path it prints, instead of (b), the instructions ONE trip round each arithmetic inner loop executes on the path of an
ordinary row (executed_paths: round the accelerate blocks), and the kernel's SGPR spills and scratch beside its registers —
the bookkeeping of profiles/core_loop_isa.txt (8-level steady loop of the free sweeps: 959 = v_pk 536 / v_trans 32 / dpp 32 /
v_mov 66 / v_other 33 / v_cndmask 9 / salu 177 / lds 40 / vmem 18 / s_waitcnt 16 before the CORE loop).
Used for the VALU-diet bookkeeping in DESIGN.md (v_cndmask / v_mov per loop body)."""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["step4ILb1ELi0", "step4pILb1ELi0", "step3ILb1ELi0ELb1ELi1", "step3pILb1ELi0", "step2ILb1ELi2", "stepILi4ELb1ELi2", "multiILi32"]


def classify(op):
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith(("v_mov", "v_pk_mov", "v_accvgpr", "v_readfirstlane", "v_readlane", "v_writelane")):
        return "v_mov" if not op.endswith("_dpp") else "dpp"
    if "_dpp" in op:
        return "dpp"
    if op.startswith("v_pk_"):
        return "v_pk"
    if op.startswith(("v_rcp", "v_sqrt", "v_rsq")):
        return "v_trans"
    if op.startswith("v_"):
        return "v_other"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def kernels(text):
    """yields (name, [instruction lines]) for every function in the assembly"""
    cur, body = None, []
    for ln in text.split("\n"):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", ln)
        if m:
            if cur:
                yield cur, body
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            yield cur, body
            cur, body = None, []
            continue
        body.append(ln)
    if cur:
        yield cur, body


def loops(body):
    """(all instructions, {loop header label: [instructions of the blocks the compiler marks as part of that loop]}) — from the
    block comments of the assembly ('=>This Inner Loop Header', 'in Loop: Header=BBn_m'): blocks of a loop need not be
    contiguous in the layout, so a label-to-backward-branch span would miss or mix them"""
    ins, per, cur, label = [], {}, None, None
    for ln in body:
        m = re.match(r"^\.(LBB\w+):\s*(;.*)?$", ln)
        if m:
            c = m.group(2) or ""
            label = m.group(1) if "Parent Loop" in c else None  # (a nested loop: its header comment is on the next lines)
            if "Loop Header" in c:
                cur = m.group(1)
            else:
                h = re.search(r"in Loop: Header=(BB\w+)", c)
                cur = "L" + h.group(1) if h else None
            continue
        if label and re.match(r"^\s+;", ln):
            if "Loop Header" in ln:
                cur = label
            continue
        label = None
        h = re.match(r"^; %bb\.\d+:\s*;\s*in Loop: Header=(BB\w+)", ln)
        if h:
            cur = "L" + h.group(1)
            continue
        if re.match(r"^; %bb\.\d+:", ln):
            cur = None
            continue
        s = ln.strip()
        if ln.startswith("\t") and s and not s.startswith((".", ";")):
            ins.append(s)
            if cur:
                per.setdefault(cur, []).append(s)
    return ins, per


def blocks(body):
    """[[label, header of the innermost loop the block belongs to (its own label for a loop header) or None, is an inner-loop
    header, [instructions]]] in layout order.  A loop nested in another one has its header comment on the lines AFTER the label
    ('Parent Loop BBn_m' first, then '=>  This Inner Loop Header')."""
    out, pending = [], False
    for ln in body:
        m = re.match(r"^\.(LBB\w+):\s*(;.*)?$", ln)
        h = None if m else re.match(r"^; %bb\.(\d+):\s*(;.*)?$", ln)
        if m or h:
            label = m.group(1) if m else "bb." + h.group(1)
            c = (m or h).group(2) or ""
            mem = re.search(r"in Loop: Header=(BB\w+)", c)
            out.append([label, "L" + mem.group(1) if mem else None, False, []])
            pending = "Parent Loop" in c
            if "Loop Header" in c:
                out[-1][1], out[-1][2] = label, "Inner Loop Header" in c
            continue
        if not out:
            continue
        if pending and re.match(r"^\s+;", ln):
            if "Loop Header" in ln:
                out[-1][1], out[-1][2] = out[-1][0], "Inner Loop Header" in ln
            continue
        pending = False
        s = ln.strip()
        if ln.startswith("\t") and s and not s.startswith((".", ";")):
            out[-1][3].append(s)
    return out


def executed_paths(body):
    """{inner-loop header: the instructions ONE trip round the loop executes}: from the header back to it, every lane-mask skip
    (s_cbranch_execz / execnz: some lane is active) falling through; a wave-uniform forward branch (scc, vcc) round blocks of the
    loop is taken when those blocks hold float compares — the accelerate step of a level, which one row of the grid executes,
    is the only place the window kernels compare floats — and falls through otherwise (a sum over one of the chunk's own
    rows); any other branch goes the way that is back at the header after the fewest instructions."""
    blks = blocks(body)
    index = {b[0]: i for i, b in enumerate(blks)}
    res = {}
    for hi, hb in enumerate(blks):
        if not hb[2]:
            continue
        member = {i for i, b in enumerate(blks) if b[1] == hb[0]}

        def succ(i):
            last = blks[i][3][-1].split() if blks[i][3] else [""]
            if last[0] == "s_branch":
                return [index.get(last[1][1:], -1)], False
            if last[0].startswith("s_cbranch"):
                return [i + 1, index.get(last[1][1:], -1)], "exec" in last[0]
            return [i + 1], False

        inf = float("inf")
        dist = {i: inf for i in member}
        for _ in range(len(member) + 1):  # instructions from the start of a block to the header, by the shortest way
            for i in member:
                ss, lane_skip = succ(i)
                if lane_skip:
                    ss = ss[:1]
                dist[i] = len(blks[i][3]) + min([0 if s == hi else dist.get(s, inf) for s in ss])
        seq, cur = [], hi
        for _ in range(len(member) + 1):
            seq += blks[cur][3]
            ss, lane_skip = succ(cur)
            if lane_skip:
                ss = ss[:1]
            if len(ss) == 2 and cur < ss[1] and all(i in member for i in range(cur + 1, ss[1] + 1)):
                # a wave-uniform forward branch round blocks of this loop: round them if they are an accelerate step
                around = [x for i in range(cur + 1, ss[1]) for x in blks[i][3]]
                cur = ss[1] if any(re.match(r"v_cmp\w*_f32", x) for x in around) else ss[0]
            else:
                cur = min(ss, key=lambda s: 0 if s == hi else dist.get(s, inf))
            if cur == hi or dist.get(cur, inf) == inf:
                break
        res[hb[0]] = seq
    return res


def main():
    args = sys.argv[1:]
    follow = "--path" in args
    args = [a for a in args if a != "--path"]
    path = args[0] if args and args[0].endswith(".s") else None
    filters = [a for a in args if not a.endswith(".s")] or DEFAULT
    if path is None:
        # the library's two translation units with the flags the Makefile gives them (the deep window kernels: max-ILP scheduling)
        text = ""
        for src, extra in (("lbm_hip.cpp", []), ("lbm_deep.cpp", ["-mllvm", "-amdgpu-sched-strategy=max-ilp"])):
            path = os.path.join(tempfile.gettempdir(), src.replace(".cpp", "_gfx950.s"))
            subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-I/opt/rocm/include", "-w"] + extra +
                           ["-S", "--cuda-device-only", "-o", path, os.path.join(ROOT, "opencl-lattice-boltzmann_amd", "csrc", src)], check=True)
            text += open(path).read() + "\n"
    else:
        text = open(path).read()
    meta = {}
    for b in text.split("  - .agpr_count")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", b).group(1)
        meta[nm] = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, b).group(1)) for k in
                         ("vgpr_count", "vgpr_spill_count", "group_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size"))
    for name, body in kernels(text):
        if not any(f in name for f in filters):
            continue
        ins, per = loops(body)
        v, sp, lds, sg, ssp, scratch = meta.get(name, (0, 0, 0, 0, 0, 0))
        print("%s\n  vgpr %d  spilled %d  lds %d B  sgpr %d  sgprs spilled %d  scratch %d B" % (name, v, sp, lds, sg, ssp, scratch))
        if follow:
            # what ONE trip round each arithmetic loop executes on its ordinary path (--path), by arithmetic content
            for h, seq in sorted(executed_paths(body).items(), key=lambda kv: -sum(1 for x in kv[1] if x.startswith("v_pk"))):
                c = Counter(classify(x.split()[0]) for x in seq)
                if c["v_pk"] < 100:
                    continue
                print("  path %-12s %5d executed: " % (h, len(seq)) +
                      "  ".join("%s %d" % (k, c[k]) for k in ("v_pk", "v_trans", "dpp", "v_mov", "v_other", "v_cndmask", "salu", "lds", "vmem", "s_waitcnt", "other") if c[k]))
            continue
        # the kernel, then its loops by arithmetic content (the row loops of the two sweep directions, general and steady form)
        rows = [("kernel", ins)] + [("loop " + h, seq) for h, seq in sorted(per.items(), key=lambda kv: -sum(1 for x in kv[1] if x.startswith("v_pk")))[:int(os.environ.get("ISA_LOOPS","4"))]]
        for label, seq in rows:
            c = Counter(classify(x.split()[0]) for x in seq)
            valu = sum(n for k, n in c.items() if k.startswith("v_") or k == "dpp")
            print("  %-14s %5d instructions, VALU %5d: " % (label, len(seq), valu) +
                  "  ".join("%s %d" % (k, c[k]) for k in ("v_pk", "v_other", "v_trans", "v_cndmask", "v_mov", "dpp", "lds", "vmem", "salu", "s_waitcnt", "other") if c[k]))


if __name__ == "__main__":
    main()

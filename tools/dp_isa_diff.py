#!/usr/bin/env python3
"""tools/dp_isa_diff.py — are the fp64 kernels of two builds the same instructions?  No device needed.

Give it the device assembly of csrc/lbm_dp.cpp and csrc/lbm_dens.cpp of two trees, written with the Makefile's flags, the units
in the same order on both sides:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -I/opt/rocm/include --cuda-device-only -S csrc/lbm_dp.cpp -o new_dp.s
    python tools/dp_isa_diff.py old_dp.s,old_dens.s new_dp.s,new_dens.s

Every fp64 kernel of each unit of the first build — the step families d2q9_dp_step, d2q9_dp_multi, d2q9_dp_ensemble and
d2q9_dp_ensemble_gated, d2q9_dp_buoyant, the scalar's dp_scalar_*, the helpers dp_reduce, dp_accelerate_row, dp_init_cells,
dp_pack_planes, dp_final_fields and dp_force_state, and the two steady kernels — is compared with the instance of the same unit
of the second build that has the same name and whose bool template flags begin with the same values and end in zeros (a build
with one more option, the option off): instructions, directives and the kernel descriptor, line by line, with comments dropped
and symbol names and basic-block label numbers normalised.  Prints the instances that differ, one summary line for the four step families and one for
the other kernels; exits 1 if any differs or is missing."""
import re
import sys

STEP_FAMILIES = ("d2q9_dp_step", "d2q9_dp_multi", "d2q9_dp_ensemble", "d2q9_dp_ensemble_gated")
STEADY = ("dens_steady_check", "ens_steady_begin")


def kernels(path, unit):
    """{(unit, kernel, flags): normalised lines} of every fp64 kernel in one assembly file"""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^_ZN3lbmL?(\d+)(\S*):", line)
        kind = m.group(2)[:int(m.group(1))] if m else ""
        if kind.startswith(("d2q9_dp_", "dp_")) or kind in STEADY:
            if name is not None:
                out[name] = body
            name, body = (unit, kind, "".join(re.findall(r"Lb([01])E", m.group(2)))), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name], name = body, None
            continue
        text = line.split(";")[0].strip()
        if text:
            body.append(re.sub(r"_ZN3lbm[0-9A-Za-z_]+", "NAME", re.sub(r"\.LBB\d+_", ".LBB_", text)))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = {}, {}
    for unit, f in enumerate(sys.argv[1].split(",")):
        old.update(kernels(f, unit))
    for unit, f in enumerate(sys.argv[2].split(",")):
        new.update(kernels(f, unit))
    # [identical, not, in the second] for the step families and for the other kernels
    count = {True: [0, 0, sum(k in STEP_FAMILIES for _, k, _ in new)], False: [0, 0, sum(k not in STEP_FAMILIES for _, k, _ in new)]}
    for (unit, kind, flags), body in sorted(old.items()):
        width = max((len(f) for u, k, f in new if (u, k) == (unit, kind)), default=len(flags))
        other = new.get((unit, kind, flags + "0" * (width - len(flags))))
        count[kind in STEP_FAMILIES][other != body] += 1
        if other != body:
            print("%s unit %d %s<%s>" % ("missing" if other is None else "differs", unit, kind, ",".join(flags)))
    for step, what in ((True, "instances"), (False, "other kernels")):
        same, bad, there = count[step]
        print("%d %s of the first build: %d identical in the second, %d not; the second has %d" % (same + bad, what, same, bad, there))
    return 1 if count[True][1] or count[False][1] else 0


if __name__ == "__main__":
    sys.exit(main())

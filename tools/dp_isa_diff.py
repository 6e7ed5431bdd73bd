#!/usr/bin/env python3
"""tools/dp_isa_diff.py — are the fp64 step kernels of two builds the same instructions?  No device needed.

Give it the device assembly of csrc/lbm_dp.cpp and csrc/lbm_dens.cpp of two trees, written with the Makefile's flags:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -I/opt/rocm/include --cuda-device-only -S csrc/lbm_dp.cpp -o new_dp.s
    python tools/dp_isa_diff.py old_dp.s,old_dens.s new_dp.s,new_dens.s

Every instance of d2q9_dp_step, d2q9_dp_multi, d2q9_dp_ensemble and d2q9_dp_ensemble_gated of the first build is compared with
the instance of the second whose bool template flags begin with the same values and end in zeros (a build with one more option,
the option off): instructions, directives and the kernel descriptor, line by line, with comments dropped and symbol names and
basic-block label numbers normalised.  Prints the instances that differ and one summary line; exits 1 if any differs or is
missing."""
import re
import sys


def kernels(path):
    """{(kernel, flags): normalised lines} of every fp64 step kernel in one assembly file"""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_ZN3lbm\S*d2q9_dp_(?:step|multi|ensemble)\S*):", line)   # not d2q9_dp_buoyant: it has no older twin
        if m:
            if name is not None:
                out[name] = body
            kind = re.search(r"d2q9_dp_(step|multi|ensemble_gated|ensemble)", m.group(1)).group(1)
            name, body = (kind, "".join(re.findall(r"Lb([01])E", m.group(1)))), []
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
    for f in sys.argv[1].split(","):
        old.update(kernels(f))
    for f in sys.argv[2].split(","):
        new.update(kernels(f))
    same = bad = 0
    for (kind, flags), body in sorted(old.items()):
        width = max((len(f) for k, f in new if k == kind), default=len(flags))
        other = new.get((kind, flags + "0" * (width - len(flags))))
        if other == body:
            same += 1
        else:
            bad += 1
            print("%s d2q9_dp_%s<%s>" % ("missing" if other is None else "differs", kind, ",".join(flags)))
    print("%d instances of the first build: %d identical in the second, %d not; the second has %d" % (len(old), same, bad, len(new)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two hipcc ``-S`` listings (gfx950): the evidence behind a
"compiles to the same instructions" claim.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math --cuda-device-only \
        -S -o OLD.s flame_amd/csrc/fedagg.hip -Iinclude          # on the parent, then on the branch
    python tools/isa_diff.py OLD.s NEW.s [--show 20]

A kernel is a symbol with an ``.amdhsa_kernel`` descriptor.  Two kernels are identical when their
instruction lines agree (comments stripped, the function number in ``.LBB<n>_<k>`` labels dropped)
and their descriptors give the same VGPR / SGPR counts, scratch bytes and LDS bytes.  Prints one
summary line, then every kernel that is missing, added or different with its instruction and
resource deltas (``--show N``: the first N differing lines of each).  Exit status 0 only when the
sets of names are equal and every kernel is identical.
"""
import argparse
import difflib
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    """{name: (instruction lines, {resource: value})} of every .amdhsa_kernel in the listing."""
    lines = open(path).read().splitlines()
    res, name = {}, None
    for ln in lines:
        s = ln.strip()
        if s.startswith(".amdhsa_kernel "):
            name = s.split()[1]
            res[name] = {}
        elif s == ".end_amdhsa_kernel":
            name = None
        elif name is not None:
            m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", s)
            if m and m.group(1) in RESOURCES:
                res[name][m.group(1)] = m.group(2)
    out, cur = {}, None
    for ln in lines:
        m = re.match(r"^([_A-Za-z0-9.$]+):", ln)
        if m and m.group(1) in res and cur is None:
            cur = m.group(1)
            out[cur] = ([], res[cur])
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        s = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].split("//")[0]).strip()
        if s and not (s.startswith(".") and not s.startswith(".LBB_")):     # drop directives, keep block labels
            out[cur][0].append(s)
    missing = sorted(set(res) - set(out))
    if missing:
        sys.exit(f"{path}: no body found for {missing[:3]}")
    return out


def count(body):
    return sum(1 for s in body if not s.endswith(":"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", type=int, default=0, help="differing lines to print per kernel")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    common = sorted(set(old) & set(new))
    differ = [k for k in common if old[k] != new[k]]
    same = len(common) - len(differ)
    print(f"kernels: old {len(old)}, new {len(new)}; names only in old {len(gone)}, only in new {len(added)}; "
          f"identical {same} of {len(common)}")
    print(f"instructions compared: {sum(count(old[k][0]) for k in common)} old, "
          f"{sum(count(new[k][0]) for k in common)} new")
    for k in gone:
        print(f"  only in old: {k}")
    for k in added:
        print(f"  only in new: {k}")
    for k in differ:
        (ob, orr), (nb, nr) = old[k], new[k]
        print(f"  differs: {k}: instructions {count(ob)} -> {count(nb)} ({count(nb) - count(ob):+d})" +
              "".join(f", {r} {orr.get(r)} -> {nr.get(r)}" for r in RESOURCES if orr.get(r) != nr.get(r)))
        if a.show:
            d = [ln for ln in difflib.unified_diff(ob, nb, lineterm="", n=0) if not ln.startswith(("---", "+++", "@@"))]
            for ln in d[:a.show]:
                print(f"      {ln}")
    sys.exit(1 if gone or added or differ else 0)


if __name__ == "__main__":
    main()

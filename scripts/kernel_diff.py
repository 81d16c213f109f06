#!/usr/bin/env python3
"""Did a source change alter any kernel? Compares the cross-compiler's assembly
of two builds of the same translation units, kernel by kernel: the instruction
streams with labels renumbered and every .amdhsa_* directive (kernarg_size
included). Kernels are matched by demangled name with the namespace qualifiers
stripped (an argument type that moved to another namespace renames the
symbol); the argument list joins the name only where a file has two kernels of
one name. The parser is scripts/rates_kernel_resources.py's.

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 \
        --cuda-device-only -S FILE.hip -o DIR/FILE.s      (the Makefile's flags)
    ... for every .hip file of csrc/, of the parent commit and of this one ...
    python3 scripts/kernel_diff.py PARENT_DIR NOW_DIR FILE.s ... \
        > profiles/common_core_kernel_diff.txt

Exit status 1 when a kernel differs, is missing or is new.
"""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rates_kernel_resources import demangle, kernels, short  # noqa: E402


def strip_ns(d):
    d = d.replace("(anonymous namespace)::", "")
    return re.sub(r"\b[A-Za-z_]\w*::", "", d)


def by_name(path):
    """{matching name: (directives, body)} of one assembly file."""
    ks = kernels(path)
    dm = demangle(list(ks))
    names = {m: short(strip_ns(dm[m])) for m in ks}
    count = collections.Counter(names.values())
    out = {}
    for m, v in ks.items():
        key = names[m]
        if count[key] > 1:
            key = re.sub(r"^void ", "", strip_ns(dm[m]))
        assert key not in out, key
        out[key] = v
    return out


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    par_dir, now_dir, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    print("Every kernel of csrc/*.hip against the parent commit: hipcc --offload-arch=gfx950 -O3")
    print("-ffp-contract=off -fPIC -std=c++17 --cuda-device-only -S (the Makefile's flags);")
    print("instruction streams with labels renumbered and every .amdhsa_* directive, kernels")
    print("matched by demangled name without namespace qualifiers (scripts/kernel_diff.py).")
    print()
    print("%-18s | %7s %7s %9s %7s" % ("file", "kernels", "parent", "identical", "differ"))
    bad, total, same_total = [], 0, 0
    for f in files:
        par, now = by_name(os.path.join(par_dir, f)), by_name(os.path.join(now_dir, f))
        same = diff = 0
        for k, (h, body) in sorted(now.items()):
            if k not in par:
                bad.append("%s: %s  (not in the parent)" % (f, k))
                continue
            hp, bp = par[k]
            if h == hp and body == bp:
                same += 1
                continue
            diff += 1
            dirs = sorted(d for d in set(h) | set(hp) if h.get(d) != hp.get(d))
            bad.append("%s: %s  (instructions %d -> %d, vgpr %s -> %s, sgpr %s -> %s%s)" % (
                f, k, len(bp), len(body), hp["next_free_vgpr"], h["next_free_vgpr"],
                hp["next_free_sgpr"], h["next_free_sgpr"],
                "".join(", %s %s -> %s" % (d, hp.get(d), h.get(d)) for d in dirs
                        if d not in ("next_free_vgpr", "next_free_sgpr"))))
        for k in sorted(set(par) - set(now)):
            bad.append("%s: %s  (only in the parent)" % (f, k))
        print("%-18s | %7d %7d %9d %7d" % (f, len(now), len(par), same, diff))
        total += len(now)
        same_total += same
    print()
    print("%d kernels, %d identical to the parent's, %d not%s" % (
        total, same_total, len(bad), ":" if bad else ""))
    for b in bad:
        print("  " + b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

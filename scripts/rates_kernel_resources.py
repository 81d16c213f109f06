#!/usr/bin/env python3
"""profiles/rates_kernel_resources.txt: registers, scratch and LDS of every
update kernel instantiation that forms the rate and J.E sums, from the
cross-compiler's assembly, and -- given the parent commit's assembly -- whether
the instantiations without the sums kept their code.

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 \
        --cuda-device-only -S afh_species.hip -o now_species.s     (the Makefile's flags)
    ... the same for afh2d.hip, and for both files of the parent commit ...
    python3 scripts/rates_kernel_resources.py now_species.s now_2d.s \
        [--parent par_species.s par_2d.s] > profiles/rates_kernel_resources.txt
"""
import argparse
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: (dict of .amdhsa_* values, normalised body lines)}."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text,
                         re.S | re.M):
        name, block = m.group(1), m.group(2)
        out[name] = [dict(re.findall(r"\.amdhsa_(\w+) (\S+)", block)), None]
    cur = None
    for line in text.splitlines():
        if cur is None:
            m = re.match(r"(\S+):\s*; @", line)
            if m and m.group(1) in out:
                cur, body = m.group(1), []
        elif line.startswith(".Lfunc_end"):
            out[cur][1], cur = body, None
        else:
            line = line.split(";")[0].strip()
            if line and not line.startswith("."):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                       check=True)
    return dict(zip(names, r.stdout.splitlines()))


def short(d):
    d = re.sub(r"^void ", "", d)
    d = re.sub(r"\(.*$", "", d)
    return d.replace("afh2::", "").replace("afh::", "").replace("(anonymous namespace)::", "")


def with_sums(s):
    """An update instantiation whose last template argument (RS / RATES) is on."""
    return re.match(r"k2?_update<.*, true>$", s) is not None


def parent_name(s):
    """The parent's name of an instantiation without the sums."""
    return re.sub(r", false>$", ">", s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm", nargs="+")
    ap.add_argument("--parent", nargs="*", default=[])
    a = ap.parse_args()
    now, par = {}, {}
    for p in a.asm:
        now.update(kernels(p))
    for p in a.parent:
        par.update(kernels(p))
    dn, dp = demangle(list(now)), demangle(list(par))
    print("The update kernels that form the rate and J.E sums (afh_fluid_set_rate_sums):")
    print("k_update<NS, SLOW, NP, SD, GAS, NET, SF, RS = true> of afh_species.hip and")
    print("k2_update<NS, CYL, PHOTO, MASK, IONS, SRCFAC, RATES = true> of afh2d.hip, and the")
    print("fold kernels. hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17")
    print("--cuda-device-only -S (the Makefile's flags), the .amdhsa_* directives:")
    print("  vgpr  .amdhsa_next_free_vgpr")
    print("  scr   .amdhsa_private_segment_fixed_size (scratch, bytes)")
    print("  lds   .amdhsa_group_segment_fixed_size (bytes)")
    print("  karg  .amdhsa_kernarg_size (bytes, the hidden arguments included)")
    print()
    print("  sib   scr of the sibling instantiation without the sums (the same arguments)")
    print()
    print("%-72s | %4s %5s %5s %5s %5s" % ("kernel", "vgpr", "scr", "lds", "karg", "sib"))
    bys = {short(v): k for k, v in dn.items()}
    rows, bad, more = [], [], []
    for name, (h, _) in now.items():
        s = short(dn[name])
        if with_sums(s) or "rate_fold" in s:
            ns = int(re.match(r"k2?_update<(\d+)", s).group(1)) if "update" in s else 0
            scr = int(h["private_segment_fixed_size"])
            sib = bys.get(re.sub(r", true>$", ", false>", s)) if "update" in s else None
            sib_scr = int(now[sib][0]["private_segment_fixed_size"]) if sib else 0
            rows.append((s.startswith("k2"), ns, s, int(h["next_free_vgpr"]), scr,
                         int(h["group_segment_fixed_size"]), int(h["kernarg_size"]), sib_scr))
            if scr and ns <= 12:
                bad.append("%s  (%d bytes; its sibling %d)" % (s, scr, sib_scr))
            if scr > sib_scr:
                more.append(s)
    for _, _, s, v, scr, lds, ka, sib in sorted(rows):
        print("%-72s | %4d %5d %5d %5d %5d" % (s, v, scr, lds, ka, sib))
    print()
    print("%d instantiations; with more scratch than the sibling without the sums: %d%s" % (
        len(rows), len(more), "".join("\n  " + b for b in more)))
    print("with NS <= 12 and scratch (NS = 1: the one-element species arrays indexed at run")
    print("time; GAS with NS >= 9: the NS + 4 density slots): %d%s" % (
        len(bad), "".join("\n  " + b for b in bad)))
    upd = [r for r in rows if "update" in r[2]]
    print("largest vgpr %d (arch + accumulation registers), largest scratch %d (k2_update<32>:"
          % (max(r[3] for r in upd), max(r[4] for r in upd)))
    print("the species arrays of the generic count)")
    if par:
        byp = {short(v): k for k, v in dp.items()}
        same = diff = 0
        changed = []
        for name, (h, body) in now.items():
            s = short(dn[name])
            if not re.match(r"k2?_update<", s) or with_sums(s):
                continue
            p = byp.get(parent_name(s)) or byp.get(s)
            if p is None:
                changed.append(s + "  (not in the parent)")
                continue
            hp, bp = par[p]
            if body == bp and h == hp:
                same += 1
            else:
                diff += 1
                changed.append("%s  (instructions %d -> %d, vgpr %s -> %s)" % (
                    s, len(bp), len(body), hp["next_free_vgpr"], h["next_free_vgpr"]))
        print()
        print("Instantiations without the sums against the parent commit (instruction streams")
        print("with labels renumbered, and every .amdhsa_* directive): %d identical, %d differ%s"
              % (same, diff, "".join("\n  " + c for c in changed)))
    return 1 if more else 0


if __name__ == "__main__":
    sys.exit(main())

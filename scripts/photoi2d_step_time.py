#!/usr/bin/env python3
"""Time of one photoionization update (photoi_set_src) in the 2-D library.

The case_s2d deck (programs/standard_2d/streamer_2d.cfg) with photoionization
switched on in memory (photoi%enabled, the `photo` and `helmh_n` variables,
photoi%species = O2_plus as the deck names it), its coarse grid refined
uniformly until the finest level holds 256 boxes of 8^2 cells, and again to
1024. Per tree, medians over --rounds rounds of wall-clock times, each from a
drained stream to a drained stream:

  set_src      the driver's photoi_set_src: source + afh_photoi_helmh_compute
  source       afh_photoi_set_src alone (k2_photoi_src, one launch)
  helmh        afh_photoi_helmh_compute alone (sequential modes + the sum)
  mode_n       one fas_fmg(1, 1) + maxabs_cc(i_tmp) of mode n, from the public
               calls (n_fmg of them run inside helmh)
  sum_rest     helmh - sum_n n_fmg_n * mode_n: the copies of the source, max|rhs|
               and k2_photoi_sum

The launches of one call are counted from a kernel trace, not here: run

    rocprofv3 --kernel-trace --output-format csv -d DIR -- \\
        python3 scripts/photoi2d_step_time.py --count-calls N --level 5

which issues two warm-up calls and then N photoi_set_src calls, each starting
with one k2_photoi_src launch; `photoi2d_step_time.py --trace DIR N` then
takes the kernels traced from the first to the last source launch of those N
calls and divides by N - 1.

    python3 scripts/photoi2d_step_time.py [--rounds R] [--json PATH]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "afivo-streamer_amd"))

from afh import capi, decks  # noqa: E402
from afh.driver import Simulation  # noqa: E402
from afh.model import photoi_helmh_compute  # noqa: E402


def photoi_deck():
    d = dict(decks.load("case_s2d"))
    names = [str(x) for x in d["cc_names"]]
    ivars = np.array(d["ivars"]).copy()
    ivars[6] = len(names) + 1
    d["cc_names"] = np.array(names + ["photo", "helmh_1", "helmh_2", "helmh_3"], dtype="U64")
    d["ivars"] = ivars
    d["photoi%enabled"] = np.array([1], d["photoi%enabled"].dtype)
    species = [str(x) for x in d["species_list"]]
    n_gas = int(d["n_species"][1])
    d["photoi_species_index"] = np.array(
        [n_gas + species.index(str(d["photoi%species"][0])) + 1], d["photoi_species_index"].dtype)
    return d


def build(deck, lvl, device):
    sim = Simulation(capi.hip_library_2d(), deck, device=device, coarse_mode=capi.COARSE_PFMG,
                     coarse_cycles=50, coarse_tol=1e-6)
    sim.af.refine_up_to_lvl(lvl)
    sim._bind(sim._create_tree())
    af, ng = sim.af, sim.af.nc + 2
    ne = np.zeros((af.highest_id, ng, ng))
    fld = np.zeros_like(ne)
    L = sim.L
    for b in range(1, af.highest_id + 1):
        if not af.in_use[b]:
            continue
        idx = np.arange(ng) - 0.5
        x = af.r_min[b][0] + idx * af.dr[b][0]
        y = af.r_min[b][1] + idx * af.dr[b][1]
        yy, xx = np.meshgrid(y, x, indexing="ij")
        g = np.exp(-((xx - 0.5 * L[0]) ** 2 + (yy - 0.5 * L[1]) ** 2) / (0.05 * L[0]) ** 2)
        ne[b - 1] = 1e14 + 1e19 * g
        fld[b - 1] = 2e6 + 8e6 * g
    sim.tree.put_cc(sim.i_electron, ne)
    sim.tree.put_cc(sim.i_efld, fld)
    return sim


def wall(sim, fn):
    sim.tree.sync()
    t0 = time.perf_counter()
    r = fn()
    sim.tree.sync()
    return 1e3 * (time.perf_counter() - t0), r


def measure(sim, rounds):
    rel = sim.c.r("photoi_helmh%max_rel_residual")
    src = lambda: sim.fluid.photoi_set_src(sim.i_rhs, sim.photoi_coeff, alpha_col=3)  # noqa: E731
    helmh = lambda: list(photoi_helmh_compute(sim.helm, sim.helm_coeffs, sim.i_photo,  # noqa: E731
                                              rel, 10))
    for _ in range(2):  # warm-up: code objects, the PFMG tables
        sim.photoi_set_src()
    t = {"set_src": [], "source": [], "helmh": [], "sum_rest": []}
    for k in range(len(sim.helm)):
        t["mode_%d" % (k + 1)] = []
    n_fmg = None
    for _ in range(rounds):
        t["set_src"].append(wall(sim, sim.photoi_set_src)[0])
        t["source"].append(wall(sim, src)[0])
        ms, n_fmg = wall(sim, helmh)
        t["helmh"].append(ms)
        modes = 0.0
        for k, m in enumerate(sim.helm):
            def one(m=m):
                m.fas_fmg(True, True)
                return sim.tree.maxabs_cc(m.i_tmp)
            mk = wall(sim, one)[0]
            t["mode_%d" % (k + 1)].append(mk)
            modes += n_fmg[k] * mk
        t["sum_rest"].append(ms - modes)
    af = sim.af
    return {"boxes_per_level": [len(af.lvls[l]["ids"]) for l in range(1, af.highest_lvl + 1)],
            "n_fmg": [int(n) for n in n_fmg],
            "ms": {k: float(np.median(v)) for k, v in t.items()}, "ms_all": t}


def count_from_trace(path, calls):
    """Kernels per photoi_set_src call from a rocprofv3 kernel trace: those
    from the first k2_photoi_src of the counted calls up to (not including)
    the last one's, over calls - 1."""
    rows = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    marks = [i for i, n in enumerate(names) if "k2_photoi_src" in n]
    if len(marks) < calls:
        sys.exit("trace holds %d source launches, fewer than %d" % (len(marks), calls))
    first, last = marks[-calls], marks[-1]
    per = (last - first) / (calls - 1)
    seg = names[first:last]
    by = {}
    for n in seg:
        key = n.split("(")[0].split("<")[0].split("::")[-1]
        by[key] = by.get(key, 0) + 1
    return {"launches_per_call": per,
            "by_kernel_per_call": {k: v / (calls - 1) for k, v in sorted(by.items())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--levels", type=int, nargs="+", default=[5, 6])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json")
    ap.add_argument("--count-calls", type=int, default=0)
    ap.add_argument("--level", type=int, default=5)
    ap.add_argument("--trace", nargs=2, metavar=("DIR", "CALLS"))
    a = ap.parse_args()
    if a.trace:
        out = count_from_trace(a.trace[0], int(a.trace[1]))
        print(json.dumps(out))
        if a.json:
            prev = json.load(open(a.json)) if os.path.exists(a.json) else {}
            prev["launches"] = out
            json.dump(prev, open(a.json, "w"), indent=1)
        return
    deck = photoi_deck()
    if a.count_calls:
        sim = build(deck, a.level, a.device)
        for _ in range(2 + a.count_calls):
            sim.photoi_set_src()
        sim.tree.sync()
        sim.tree.close()
        return
    out = {"rounds": a.rounds, "trees": {}}
    for lvl in a.levels:
        sim = build(deck, lvl, a.device)
        out["trees"]["finest_%d_boxes" % len(sim.af.lvls[lvl]["ids"])] = measure(sim, a.rounds)
        sim.tree.close()
    print(json.dumps(out))
    if a.json:
        prev = json.load(open(a.json)) if os.path.exists(a.json) else {}
        prev.update(out)
        with open(a.json, "w") as f:
            json.dump(prev, f, indent=1)


if __name__ == "__main__":
    main()

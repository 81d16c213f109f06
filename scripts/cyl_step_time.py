#!/usr/bin/env python3
"""Time per launch of the cylindrical smoother pair against the Cartesian one.

The case_s2d deck (programs/standard_2d/streamer_2d.cfg) with `cylindrical`
switched on in memory; the same host tree for both -- the deck's coarse grid
refined uniformly until the two finest levels hold 256 and 1024 boxes of 8^2
cells, the levels afh_profile_enable(AFH_PROF_GSRB) times -- and the same
right-hand side. V-cycles run eagerly while kernels are timed, so the figure
is the kernel's (k2_pair_box / k2_pair_box<CYL = true>), alternating the two trees.

    python3 scripts/cyl_step_time.py [--cycles N] [--rounds R] [--json PATH]

Prints microseconds per launch of each and their ratio.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "afivo-streamer_amd"))

from afh import capi, decks  # noqa: E402
from afh.driver import Simulation  # noqa: E402


def build(deck, cyl, lvl, device):
    d = dict(deck)
    d["cylindrical"] = np.array([1 if cyl else 0], d["cylindrical"].dtype)
    sim = Simulation(capi.hip_library_2d(), d, device=device, coarse_mode=capi.COARSE_PFMG,
                     coarse_cycles=50, coarse_tol=1e-6)
    sim.af.refine_up_to_lvl(lvl)
    sim._bind(sim._create_tree())
    af, ng = sim.af, sim.af.nc + 2
    rhs = np.zeros((af.highest_id, ng, ng))
    L = sim.L
    for b in range(1, af.highest_id + 1):
        if not af.in_use[b]:
            continue
        idx = np.arange(ng) - 0.5
        x = af.r_min[b][0] + idx * af.dr[b][0]
        y = af.r_min[b][1] + idx * af.dr[b][1]
        yy, xx = np.meshgrid(y, x, indexing="ij")
        rhs[b - 1] = 1e9 * np.exp(-((xx - 0.3 * L[0]) ** 2 + (yy - 0.5 * L[1]) ** 2) /
                                  (0.1 * L[0]) ** 2)
    sim.tree.put_cc(sim.i_rhs, rhs)
    sim.tree.put_cc(sim.i_phi, np.zeros_like(rhs))
    sim.tree.gc_tree(sim.i_phi)
    return sim


def timed(sim, cycles):
    lib = sim.lib
    lib.call("profile_enable", sim.tree.h, capi.PROF_GSRB)
    for _ in range(cycles):
        sim.mg.fas_vcycle(False)
    sim.tree.sync()
    ms, nl, by = C.c_double(), C.c_int64(), C.c_double()
    lib.call("profile_read", sim.tree.h, C.byref(ms), C.byref(nl), C.byref(by))
    lib.call("profile_enable", sim.tree.h, 0)
    return ms.value, nl.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json")
    a = ap.parse_args()
    deck = decks.load("case_s2d")
    sims = {name: build(deck, name == "cyl", a.level, a.device) for name in ("xyz", "cyl")}
    for s in sims.values():  # warm-up: code objects, the PFMG tables
        timed(s, 2)
    us = {"xyz": [], "cyl": []}
    for _ in range(a.rounds):
        for name in ("xyz", "cyl"):
            ms, nl = timed(sims[name], a.cycles)
            if not nl:
                sys.exit("no level of >= 256 boxes was timed")
            us[name].append(1e3 * ms / nl)
    out = {"boxes_per_level": [len(sims["xyz"].af.lvls[l]["ids"])
                               for l in range(1, a.level + 1)],
           "cycles": a.cycles, "rounds": a.rounds,
           "us_per_launch": {k: float(np.median(v)) for k, v in us.items()},
           "us_per_launch_all": us}
    out["ratio_cyl_over_xyz"] = out["us_per_launch"]["cyl"] / out["us_per_launch"]["xyz"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    for s in sims.values():
        s.tree.close()


if __name__ == "__main__":
    main()

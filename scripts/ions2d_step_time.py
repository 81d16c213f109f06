#!/usr/bin/env python3
"""Cost of mobile ions in the 2-D library.

1. The flux kernel. The test_cyl_ion_motion set-up (6 mobile ions) on a
   uniformly refined cylindrical tree whose finest level holds 256 boxes of 8^2
   cells, and again 1024: the time per launch of k2_flux_ions with 6 ions and
   with 1, and of k2_flux on the same tree and state with no ions, from
   afh_profile_enable(AFH_PROF_FLUX) (HIP events around every flux launch).
   Next to the time ratio the ratio of bytes per cell: k2_flux moves 48 B (ne,
   |E|, two face fields read, two fluxes written), every ion adds one density
   read and two face writes, 24 B.

2. The step. test_cyl_ion_motion against test_cyl_chem (the same chemistry,
   no mobile ions), each run from its start: wall-clock per step of the main
   loop after a warm-up, and the leaf cells at the end.

    python3 scripts/ions2d_step_time.py [--rounds R] [--steps S] [--json PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "afivo-streamer_amd"))

from afh import capi  # noqa: E402
from afh.driver import Simulation  # noqa: E402

PFMG = dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)


def fixture(name):
    with np.load(os.path.join(REPO, "tests", "golden", name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def build(deck, lvl, n_ions, device):
    sim = Simulation(capi.hip_library_2d(), deck, device=device, **PFMG)
    sim.ions = sim.ions[:n_ions]
    sim.af.refine_up_to_lvl(lvl)
    sim._bind(sim._create_tree())
    af, ng, nf = sim.af, sim.af.nc + 2, sim.af.nc + 1
    rng = np.random.default_rng(1)
    for iv in sim.densities:
        sim.tree.put_cc(iv, 1e15 * (0.2 + rng.random((af.highest_id, ng, ng))))
    sim.tree.put_cc(sim.i_efld, 3e6 * (0.1 + 2 * rng.random((af.highest_id, ng, ng))))
    sim.tree.put_fc(sim.f_field, 3e6 * rng.standard_normal((af.highest_id, 2, nf, nf)))
    return sim


def flux_launch_us(sim, calls):
    lib = sim.lib
    for _ in range(3):
        sim.fluid.flux_upwind_tree(0)
    lib.call("profile_enable", sim.tree.h, capi.PROF_FLUX)
    for _ in range(calls):
        sim.fluid.flux_upwind_tree(0)
    ms, nl, by = C.c_double(), C.c_int64(), C.c_double()
    lib.call("profile_read", sim.tree.h, C.byref(ms), C.byref(nl), C.byref(by))
    lib.call("profile_enable", sim.tree.h, 0)
    return {"us_per_launch": 1e3 * ms.value / nl.value, "launches": nl.value,
            "bytes_per_launch": by.value / nl.value,
            "GBps": by.value / (1e-3 * ms.value) / 1e9}


def wall_flux_us(sim, calls):
    """The whole afh_flux_upwind_tree (restriction, gc2 fills, flux, consistent
    fluxes, the limits read back), wall clock."""
    sim.tree.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        sim.fluid.flux_upwind_tree(0)
    sim.tree.sync()
    return 1e6 * (time.perf_counter() - t0) / calls


def measure_kernel(deck, lvl, rounds, calls, device):
    out = {}
    for n_ions in (0, 1, 6):
        sim = build(deck, lvl, n_ions, device)
        r = [flux_launch_us(sim, calls) for _ in range(rounds)]
        w = [wall_flux_us(sim, calls) for _ in range(rounds)]
        best = sorted(r, key=lambda x: x["us_per_launch"])[len(r) // 2]
        best["us_per_launch_all"] = [x["us_per_launch"] for x in r]
        best["flux_tree_wall_us"] = float(np.median(w))
        best["leaf_boxes"] = len(sim.af.leaves())
        best["bytes_per_cell"] = 48 + 24 * n_ions
        out["ions_%d" % n_ions] = best
        sim.tree.close()
    for n in (1, 6):
        a, b = out["ions_%d" % n], out["ions_0"]
        a["time_ratio_to_k2_flux"] = a["us_per_launch"] / b["us_per_launch"]
        a["byte_ratio_to_k2_flux"] = a["bytes_per_cell"] / b["bytes_per_cell"]
    return out


def measure_steps(name, warm, steps, device):
    sim = Simulation(capi.hip_library_2d(), fixture(name), device=device, **PFMG)
    sim.start()
    for _ in range(warm):
        sim.step()
    sim.tree.sync()
    t0 = time.perf_counter()
    done = 0
    while done < steps and sim.step():
        done += 1
    sim.tree.sync()
    steps = max(done, 1)
    ms = 1e3 * (time.perf_counter() - t0) / steps
    out = {"ms_per_step": ms, "n_ions": len(sim.ions), "leaf_cells": int(sim.af.n_leaf_cells()),
           "levels": int(sim.af.highest_lvl), "steps": steps, "time": sim.time}
    sim.tree.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--levels", type=int, nargs="+", default=[5, 6])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json")
    a = ap.parse_args()
    deck = fixture("rtest_test_cyl_ion_motion")
    out = {"rounds": a.rounds, "calls": a.calls, "kernel": {}, "step": {}}
    for lvl in a.levels:
        r = measure_kernel(deck, lvl, a.rounds, a.calls, a.device)
        out["kernel"]["finest_%d_boxes" % (r["ions_0"]["leaf_boxes"])] = r
    for name in ("rtest_test_cyl_chem", "rtest_test_cyl_ion_motion"):
        out["step"][name] = measure_steps(name, a.warm, a.steps, a.device)
    s = out["step"]
    s["ms_ratio"] = (s["rtest_test_cyl_ion_motion"]["ms_per_step"] /
                     s["rtest_test_cyl_chem"]["ms_per_step"])
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the rate and J.E sums (afh_fluid_set_rate_sums) on a last step.

Sums off and on alternate in one process, medians of --rounds samples, on two
trees:

* bench.py's s1 tree (libafivo_hip.so): microseconds per update launch from
  afh_profile_read(AFH_PROF_UPDATE) over flux_update_densities with last_step
  (off: the compiled network's k_update; on: the generic reaction loop with
  the sums, and k_rate_fold after it, which the profile class does not time --
  the wall time per call is printed next to it);
* the case_s2d deck refined uniformly to --level (libafivo_hip_2d.so): wall
  time of forward_euler with last_step, the stream synchronised.

    python3 scripts/rates_step_time.py [--calls N] [--rounds R] [--json PATH]
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
sys.path.insert(0, REPO)

import bench  # noqa: E402
from afh import capi, decks  # noqa: E402
from afh.driver import Simulation  # noqa: E402
from afh.streamer import IV  # noqa: E402


def s1_sample(case, on, calls):
    """(us per update launch, wall us per flux_update_densities call)."""
    lib, f = case.lib, case.fluid
    f.set_rate_sums(on)
    f.flux_update_densities(1e-12, 0, [0], [1.0], 1, True)  # (the rows' first use)
    lib.call("profile_enable", case.tree.h, capi.PROF_UPDATE)
    case.tree.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        f.flux_update_densities(1e-12, 0, [0], [1.0], 1, True)
    case.tree.sync()
    wall = time.perf_counter() - t0
    ms, nl, by = C.c_double(), C.c_int64(), C.c_double()
    lib.call("profile_read", case.tree.h, C.byref(ms), C.byref(nl), C.byref(by))
    lib.call("profile_enable", case.tree.h, 0)
    return 1e3 * ms.value / nl.value, 1e6 * wall / calls


def build_2d(level, device):
    sim = Simulation(capi.hip_library_2d(), decks.load("case_s2d"), device=device,
                     coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
    sim.af.refine_up_to_lvl(level)
    sim._bind(sim._create_tree())
    af, ng, nf = sim.af, sim.af.nc + 2, sim.af.nc + 1
    dens = np.zeros((af.highest_id, ng, ng))
    L = sim.L
    for b in range(1, af.highest_id + 1):
        if not af.in_use[b]:
            continue
        idx = np.arange(ng) - 0.5
        x = af.r_min[b][0] + idx * af.dr[b][0]
        y = af.r_min[b][1] + idx * af.dr[b][1]
        yy, xx = np.meshgrid(y, x, indexing="ij")
        dens[b - 1] = 1e15 + 5e18 * np.exp(-((xx - 0.5 * L[0]) ** 2 + (yy - 0.5 * L[1]) ** 2) /
                                           (0.05 * L[0]) ** 2)
    for iv in sim.densities:
        sim.tree.put_cc(iv, dens)
    sim.tree.put_cc(sim.i_efld, np.full(dens.shape, 2.5e6))
    field = np.zeros((af.highest_id, 2, nf, nf))
    field[:, 1] = -2.5e6
    sim.tree.put_fc(sim.f_field, field)
    return sim


def wall_2d(sim, on, calls):
    f = sim.fluid
    f.set_rate_sums(on)
    f.forward_euler(1e-12, 0, [0], [1.0], 1, True)
    sim.tree.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        f.forward_euler(1e-12, 0, [0], [1.0], 1, True)
    sim.tree.sync()
    return 1e6 * (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json")
    a = ap.parse_args()
    med = lambda v: float(np.median(v))  # noqa: E731

    case = bench.build_case(capi.hip_library(), "s1", a.device, bench.coarse_choice("auto", "s1"))
    case.fluid.field_set_rhs(IV["rhs"], 0)
    case.field_compute(0, check_residual=False)
    case.fluid.flux_upwind_tree(0)
    s1 = {"off": [], "on": []}
    for _ in range(a.rounds):
        for name in ("off", "on"):
            s1[name].append(s1_sample(case, name == "on", a.calls))
    rates, jde = case.fluid.fetch_rate_sums()
    out = {"calls": a.calls, "rounds": a.rounds,
           "s1": {"leaves": int(sum(len(case.topo["lvl_leaves_%d" % l]) for l in
                                    range(1, int(case.topo["highest_lvl"]) + 1))),
                  "n_cell": int(case.topo["nc"]),
                  "update_us_per_launch": {k: med([x[0] for x in v]) for k, v in s1.items()},
                  "wall_us_per_call": {k: med([x[1] for x in v]) for k, v in s1.items()},
                  "samples": s1, "rates": list(rates), "jdote": jde}}
    case.tree.close()

    sim = build_2d(a.level, a.device)
    w = {"off": [], "on": []}
    for _ in range(a.rounds):
        for name in ("off", "on"):
            w[name].append(wall_2d(sim, name == "on", a.calls))
    out["2d"] = {"leaves": len(sim.af.leaves()), "n_cell": sim.af.nc,
                 "forward_euler_wall_us": {k: med(v) for k, v in w.items()}, "samples": w}
    sim.tree.close()
    for k in ("s1", "2d"):
        d = out[k].get("update_us_per_launch") or out[k]["forward_euler_wall_us"]
        out[k]["ratio_on_over_off"] = d["on"] / d["off"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

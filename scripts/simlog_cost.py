#!/usr/bin/env python3
"""Cost of one Simulation.log_row() against one time step of the same case.

The S3 case (BASELINE config 3: the 10-level AMR tree of 8^3 boxes that
set_initial_conditions builds) with log=True: wall time of step() -- Heun's
two sub-steps with their field solves, the stream synchronised -- and of
log_row(), each the median of --rounds samples on the same state and build.

    python3 scripts/simlog_cost.py [--steps N] [--rounds R] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "afivo-streamer_amd"))

from afh import capi, decks  # noqa: E402
from afh.driver import Simulation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="case_s3")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json")
    a = ap.parse_args()
    sim = Simulation(capi.hip_library(), decks.load(a.case), device=a.device, log=True)
    sim.start()
    sim.step()  # (the first step: first launches, graph captures)
    steps = []
    for _ in range(a.steps):
        sim.tree.sync()
        t0 = time.perf_counter()
        sim.step()
        sim.tree.sync()
        steps.append(time.perf_counter() - t0)
    sim.log_row()
    rows = []
    for _ in range(a.rounds):
        sim.tree.sync()
        t0 = time.perf_counter()
        sim.log_row()
        rows.append(time.perf_counter() - t0)
    out = {"case": a.case, "leaves": len(sim.af.leaves()), "n_cell": sim.af.nc,
           "highest_lvl": sim.af.highest_lvl,
           "step_ms": 1e3 * float(np.median(steps)), "log_row_ms": 1e3 * float(np.median(rows)),
           "step_samples_ms": [1e3 * x for x in steps],
           "log_row_samples_ms": [1e3 * x for x in rows]}
    out["log_row_over_step"] = out["log_row_ms"] / out["step_ms"]
    sim.tree.close()
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

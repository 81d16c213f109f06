#!/usr/bin/env python3
"""Time of one step on an electrode tree in the 2-D library, fused variable
pair against split half-sweeps.

tests/golden/rtest_test_2d_pos_electrode.npz (programs/standard_2d/tests/
test_2d_pos_electrode.cfg) is run to 1 ns; on the tree it then has, one step
is timed: copy_current_state, the two Heun stages (advance), field_compute
with its V-cycles through the electrode stencils, and the state put back, so
that every repetition does the same work. Medians over --rounds rounds of
--reps repetitions each, wall clock from a drained stream to a drained stream,
once with AFH_PAIR2D=1 (k2_pair_box<VAR = true> on the levels with variable boxes) and
once with AFH_PAIR2D=0 (k2_gsrb + k2_gsrb_v + k2_gc), plus the time of one
V-cycle alone.

    python3 scripts/electrode2d_step_time.py [--rounds R] [--reps N] [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "afivo-streamer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import golden  # noqa: E402
from afh import capi  # noqa: E402
from afh.driver import Simulation  # noqa: E402

CASE = "rtest_test_2d_pos_electrode"


def measure(pair, t_end, rounds, reps):
    os.environ["AFH_PAIR2D"] = "1" if pair else "0"
    sim = Simulation(capi.hip_library_2d(), golden.load(CASE), device=0, coarse_cycles=50,
                     coarse_tol=1e-6, coarse_mode=capi.COARSE_PFMG)
    sim.start()
    while sim.time < t_end and sim.step():
        pass
    del os.environ["AFH_PAIR2D"]
    sync = lambda: sim.lib.call("tree_sync", sim.tree.h)  # noqa: E731
    af = sim.af
    lv = {l: len(af.lvls[l]["ids"]) for l in range(1, af.highest_lvl + 1)}
    var = {l: sum(1 for b in sim.electrode_ids if af.lvl[b] == l) for l in lv}

    def one_step():
        sim.copy_current_state()
        sim.advance(sim.dt)
        sim.field_compute(0, True)
        sim.restore_previous_state()

    def one_vcycle():
        sim.mg.fas_vcycle(True)

    out = {}
    for name, fn in (("step", one_step), ("vcycle", one_vcycle)):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(rounds):
            sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            sync()
            ts.append((time.perf_counter() - t0) / reps * 1e3)
        out[name + "_ms"] = float(np.median(ts))
        out[name + "_ms_rounds"] = [float(x) for x in ts]
    out.update(time=sim.time, it=sim.it, boxes_per_level=lv, variable_boxes_per_level=var)
    sim.tree.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--t-end", type=float, default=1e-9)
    ap.add_argument("--json", default=os.path.join(REPO, "profiles", "electrode2d_step_time.json"))
    a = ap.parse_args()
    res = {"case": CASE, "t_end": a.t_end, "rounds": a.rounds, "reps": a.reps}
    # alternate the two settings so that drift shows in both
    res["pair"] = measure(True, a.t_end, a.rounds, a.reps)
    res["split"] = measure(False, a.t_end, a.rounds, a.reps)
    res["pair_again"] = measure(True, a.t_end, a.rounds, a.reps)
    print(json.dumps(res))
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tests/golden/replay_periodic2d.npz: the reference's own forward_euler on
the periodic 2-D tree P (build container only; run after
`make -C oracle ref2dfull`).

The deterministic state of tests/state_periodic2d.py is handed to
oracle/_ref/2d/replay_step with the reference's test_2d.cfg and
`-periodic=T F` (plus P's grid and domain), once per Heun stage. What is
kept is data the reference wrote: the new densities on the leaves'
interiors and dt_lim of both stages. tests/test_periodic2d_gpu.py holds the
device step to them bit for bit.
"""
import os
import resource
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "afivo-streamer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import state_periodic2d as sp  # noqa: E402

REF_TESTS = "/root/reference/programs/standard_2d/tests"
REPLAY_STEP = os.path.join(REPO, "oracle", "_ref", "2d", "replay_step")
OUT = os.path.join(REPO, "tests", "golden", "replay_periodic2d.npz")


def main():
    c, af, cc, fc = sp.build_state()
    dens = c.ia("all_densities")
    leaves = af.leaves()
    ng = af.nc + 2
    out = {"leaves": np.array(leaves, np.int32)}

    def unlimited_stack():
        resource.setrlimit(resource.RLIMIT_STACK,
                           (resource.RLIM_INFINITY, resource.RLIM_INFINITY))

    with tempfile.TemporaryDirectory() as tmp:
        for k, stage in enumerate(sp.STAGES):
            rec, res = os.path.join(tmp, "step.bin"), os.path.join(tmp, "out.bin")
            dt = sp.DT * (1.0 if k == 0 else 0.5)
            used = sp.write_record(rec, af, cc, fc, dt, 0.0, stage)
            env = dict(os.environ, OMP_STACKSIZE="512M", OMP_NUM_THREADS="4")
            subprocess.run([REPLAY_STEP, rec, res, "test_2d.cfg"] + sp.cfg_args(),
                           cwd=REF_TESTS, check=True, stdout=subprocess.DEVNULL,
                           preexec_fn=unlimited_stack, env=env)
            raw = open(res, "rb").read()
            out["dt_lim_%d" % (k + 1)] = np.frombuffer(raw, np.float64, 1)
            ref = np.frombuffer(raw, np.float64, offset=8).reshape(len(cc), len(used), ng, ng)
            pos = {b: q for q, b in enumerate(used)}
            li = [pos[b] for b in leaves]
            s_out = stage[3]
            out["dens_%d" % (k + 1)] = np.stack(
                [ref[iv + s_out - 1][li][:, 1:-1, 1:-1] for iv in dens])
            changed = np.max(np.abs(out["dens_%d" % (k + 1)][0] /
                                    cc[dens[0] + s_out][np.array(leaves) - 1][:, 1:-1, 1:-1] - 1))
            print("stage", k + 1, "dt_lim", out["dt_lim_%d" % (k + 1)][0],
                  "max relative change of the electrons", changed)
    np.savez(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

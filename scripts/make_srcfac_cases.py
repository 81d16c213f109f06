#!/usr/bin/env python3
"""tests/golden/srcfac_<model>_<variant>.npz: the reference's own forward_euler
with fixes%source_factor = flux (build container only; run after
`make -C oracle ref ref2dfull`).

The deterministic states of tests/state_srcfac.py (tree P of
tests/state_periodic.py with test_3d.cfg and test_3d_chem.cfg; the states of
tests/state2d.py with test_2d.cfg and streamer_2d.cfg) are handed to
oracle/_ref/replay_step and oracle/_ref/2d/replay_step, once per Heun stage,
with

    -fixes%source_factor=flux -fixes%write_source_factor=t

and, for the variant `min`, -fixes%source_min_electrons_per_cell=5e4.
write_source_factor adds the cc variable srcfac to the reference's registry,
so the record is laid out by name from the registry oracle/_ref/export_case
prints with the same arguments. What is kept is data the reference wrote, on
the interiors of the leaves tests/state_srcfac.kept_leaves names: dt_lim, the
new densities and the stored factor of both stages, and the electrons of the
same step without the factor (for the tests' not-vacuous conditions, which
this script checks too before it writes).
"""
import os
import resource
import struct
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "afivo-streamer_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import state_periodic as sp  # noqa: E402
import state_srcfac as ss  # noqa: E402
from make_cases import parse_dump  # noqa: E402

REF = "/root/reference/programs"
# model -> (directory of the cfg, cfg, further settings)
RUN = {
    "test_3d": (REF + "/standard_3d/tests", "test_3d.cfg", sp.cfg_args()),
    "test_3d_chem": (REF + "/standard_3d/tests", "test_3d_chem.cfg", sp.cfg_args()),
    "test_2d": (REF + "/standard_2d/tests", "test_2d.cfg", []),
    "s2d": (REF + "/standard_2d", "streamer_2d.cfg", []),
}
FACTOR = ["-fixes%source_factor=flux", "-fixes%write_source_factor=t"]


def tool(ndim, name):
    return os.path.join(REPO, "oracle", "_ref", *(["2d"] if ndim == 2 else []), name)


def unlimited_stack():
    resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))


def registry(model, extra, tmp):
    """cc_names of the reference with the settings `extra`."""
    ndim = ss.MODELS[model][0]
    cwd, cfg, args = RUN[model]
    dump = os.path.join(tmp, "export.txt")
    subprocess.run([tool(ndim, "export_case"), dump, cfg] + args + extra, cwd=cwd, check=True,
                   stdout=subprocess.DEVNULL)
    return [str(x) for x in parse_dump(dump)["cc_names"]]


def write_record(path, af, arrays, fc, dt, stage, ndim):
    """oracle/harness/replay_step.f90's record with the cc variables `arrays`
    (in the reference's order)."""
    s_deriv, s_prev, w_prev, s_out = stage
    hid = af.highest_id
    used = [b for b in range(1, hid + 1) if af.in_use[b]]
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", hid, len(arrays), len(fc), af.nc))
        for b in range(1, hid + 1):
            ix = (tuple(af.ix[b]) + (0,) * (3 - ndim)) if af.in_use[b] else (0, 0, 0)
            f.write(struct.pack("<6i", af.parent[b], af.lvl[b], *ix, int(af.in_use[b])))
        f.write(struct.pack("<ddii", dt, 0.0, s_deriv, len(s_prev)))
        f.write(struct.pack("<%di" % len(s_prev), *s_prev))
        f.write(struct.pack("<%dd" % len(w_prev), *w_prev))
        f.write(struct.pack("<i", s_out))
        for a in arrays:
            for b in used:
                f.write(np.ascontiguousarray(a[b - 1]).tobytes())
        for iv in range(1, len(fc) + 1):
            for b in used:
                f.write(np.ascontiguousarray(fc[iv][b - 1]).tobytes())
    return used


def replay(model, extra, names, state, stage, dt, tmp):
    """The reference's step with the settings `extra`; names: its registry.
    Returns dt_lim and {name: tree-wide cc array of the kept leaves}."""
    c, af, cc, fc, keep = state
    ndim = ss.MODELS[model][0]
    own = [str(x) for x in c.sa("cc_names")]
    ng = af.nc + 2
    zeros = np.zeros((af.highest_id,) + (ng,) * ndim)
    arrays = [cc[own.index(n) + 1] if n in own else zeros for n in names]
    assert [n for n in names if n not in own] in ([], ["srcfac"])
    rec, res = os.path.join(tmp, "step.bin"), os.path.join(tmp, "out.bin")
    used = write_record(rec, af, arrays, fc, dt, stage, ndim)
    cwd, cfg, args = RUN[model]
    env = dict(os.environ, OMP_STACKSIZE="512M", OMP_NUM_THREADS="4")
    subprocess.run([tool(ndim, "replay_step"), rec, res, cfg] + args + extra, cwd=cwd,
                   check=True, stdout=subprocess.DEVNULL, preexec_fn=unlimited_stack, env=env)
    raw = open(res, "rb").read()
    ref = np.frombuffer(raw, np.float64, offset=8).reshape((len(names), len(used)) + (ng,) * ndim)
    pos = {b: q for q, b in enumerate(used)}
    li = [pos[b] for b in keep]
    return float(np.frombuffer(raw, np.float64, 1)[0]), \
        {n: ss.interior(ref[q][li], ndim) for q, n in enumerate(names)}


def main():
    models = sys.argv[1:] or list(ss.MODELS)
    for model in models:
        ndim = ss.MODELS[model][0]
        c, af, cc, fc, dt0, _ = ss.build_state(model)
        own = [str(x) for x in c.sa("cc_names")]
        dens = c.ia("all_densities")
        keep = ss.kept_leaves(model, af, len(dens))
        state = (c, af, cc, fc, keep)
        with tempfile.TemporaryDirectory() as tmp:
            reg_off = registry(model, [], tmp)
            assert reg_off == own, "the exported case's registry is not the reference's"
            off = []
            for k, stage in enumerate(ss.stages(model)):
                _, o = replay(model, [], reg_off, state, stage, ss.stage_dt(model, k, dt0), tmp)
                off.append(o[own[dens[0] + stage[3] - 1]])
            changed = {}
            for variant, min_e in ss.VARIANTS.items():
                extra = FACTOR + (["-fixes%%source_min_electrons_per_cell=%r" % min_e]
                                  if min_e > 0 else [])
                reg = registry(model, extra, tmp)
                out = {"leaves": np.array(keep, np.int32)}
                for k, stage in enumerate(ss.stages(model)):
                    lim, o = replay(model, extra, reg, state, stage,
                                    ss.stage_dt(model, k, dt0), tmp)
                    out["dt_lim_%d" % (k + 1)] = np.array([lim])
                    out["dens_%d" % (k + 1)] = np.stack([o[own[iv + stage[3] - 1]] for iv in dens])
                    out["srcfac_%d" % (k + 1)] = o["srcfac"]
                    out["off_e_%d" % (k + 1)] = off[k]
                    e = out["dens_%d" % (k + 1)][0]
                    ch = np.abs(e / off[k] - 1) > 1e-10
                    s = o["srcfac"]
                    changed[variant, k] = ch
                    print("%s %s stage %d: dt_lim %.6g, electrons changed %.1f %% (max %.2g), "
                          "factor = 1: %.1f %%, = 0: %.1f %%, between: %.1f %%"
                          % (model, variant, k + 1, lim, 100 * ch.mean(),
                             np.abs(e / off[k] - 1).max(), 100 * (s == 1).mean(),
                             100 * (s == 0).mean(), 100 * ((s > 0) & (s < 1)).mean()))
                path = os.path.join(REPO, "tests", "golden", "srcfac_%s_%s.npz" % (model, variant))
                np.savez_compressed(path, **out)
                print("wrote", path, os.path.getsize(path), "bytes,", len(keep), "of",
                      len(af.leaves()), "leaves")
            for k in range(len(ss.stages(model))):
                f, m = changed["flux", k], changed["min", k]
                print("%s stage %d: threshold changes %.1f %% more cells"
                      % (model, k + 1, 100 * (m & ~f).mean()))


if __name__ == "__main__":
    main()

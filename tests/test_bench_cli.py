"""bench.py's command line: a plain run prints the result line only, --full
adds the roofline lines and the CPU baseline, --dump-outputs writes the last
timed step's outputs.

dump_outputs itself on the C oracle (CPU), on a two-level tree of 8^3 boxes:
every leaf's interior cells when they fit the byte budget, else the same
seeded cells in every variable and every call.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from afh import capi  # noqa: E402
from afh.streamer import IV  # noqa: E402

NAMES = {"e": "e", "pos": "pos", "neg": "neg", "phi": "phi", "electric_fld": "efld"}


@pytest.fixture
def tiny(monkeypatch):
    monkeypatch.setitem(bench.CONFIGS, "tiny", (8, (8, 8, 8), 2, (16e-3, 16e-3, 16e-3)))
    case = bench.build_case(capi.oracle_library(), "tiny", -1, "direct")
    case.fuse_rhs(True, ghosts=False)
    case.faces_from_phi(True)
    case.field_compute(0, n_vcycles=2)
    last = None
    for k in range(3):
        last = bench.unit_step(case, 1e-13, k)
    case.tree.sync()
    return case, last  # (k = 2: a Heun stage 1, state 1 written)


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_whole_tree(tiny, tmp_path):
    case, last = tiny
    bench.dump_outputs(case, 1, last, str(tmp_path))
    got = _load(str(tmp_path))
    assert sorted(got) == sorted(NAMES)  # (stage 1 returns no scalars)
    leaves = np.asarray(case.topo["lvl_leaves_2"]) - 1
    assert len(leaves) == 8
    for name, key in NAMES.items():
        iv = IV[key] + (1 if key in ("e", "pos", "neg") else 0)
        want = case.tree.get_cc(iv)[leaves][:, 1:-1, 1:-1, 1:-1]
        assert got[name].dtype == np.float64 and got[name].shape == (8, 8, 8, 8)
        assert np.array_equal(got[name], want), name
    assert np.all(got["e"] > 0) and np.any(got["electric_fld"] > 0)


def test_dump_outputs_sampled(tiny, tmp_path, monkeypatch):
    case, last = tiny
    monkeypatch.setattr(bench, "DUMP_BYTES", 5 * 8 * 300)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(case, 1, last, a)
    bench.dump_outputs(case, 1, last, b)
    ga, gb = _load(a), _load(b)
    assert sorted(ga) == sorted(NAMES)
    assert sum(v.nbytes for v in ga.values()) <= bench.DUMP_BYTES
    leaves = np.asarray(case.topo["lvl_leaves_2"]) - 1
    for name, key in NAMES.items():
        assert ga[name].shape == (300,) and ga[name].dtype == np.float64
        assert np.array_equal(ga[name], gb[name]), name
        # the sample lies in the leaves' interiors
        iv = IV[key] + (1 if key in ("e", "pos", "neg") else 0)
        inner = case.tree.get_cc(iv)[leaves][:, 1:-1, 1:-1, 1:-1]
        assert np.isin(ga[name], inner).all(), name
    assert len(np.unique(ga["electric_fld"])) > 50  # (not one cell over and over)


def test_dump_outputs_scalars(tiny, tmp_path):
    case, _ = tiny
    last = bench.unit_step(case, 1e-13, 3)  # a Heun stage 2: residual and dt limits
    case.tree.sync()
    bench.dump_outputs(case, 0, last, str(tmp_path))
    s = np.load(str(tmp_path / "step_scalars.npy"))
    assert s.dtype == np.float64
    assert np.array_equal(s, np.concatenate([np.ravel(last[0]), np.ravel(last[1])]))


def _run(*extra):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
                        "--config", "s1", "--steps", "3", "--warmup", "1"] + list(extra),
                       stdout=subprocess.PIPE, check=True, text=True)
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    d = _run("--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "cell-updates/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["ms_per_step"] > 0
    cells = d["config"]["leaf_cells"]
    assert cells == 512 * 16 ** 3
    assert d["value"] == pytest.approx(cells / (d["ms_per_step"] * 1e-3), rel=1e-12)
    for key in ("roofline", "roofline_smoother", "roofline_species", "cpu_baseline"):
        assert key not in d
    got = _load(str(tmp_path))
    # 3 + 1 steps: the last one a Heun stage 2, with its residual and limits
    assert sorted(got) == sorted(list(NAMES) + ["step_scalars"])
    assert sum(v.nbytes for v in got.values()) <= 64e6
    for name in NAMES:
        assert got[name].dtype == np.float64 and np.all(np.isfinite(got[name])), name
    assert got["step_scalars"][0] == d["last_residual"]


@pytest.mark.gpu
def test_full_run_line():
    d = _run("--full")
    assert d["ms_per_step"] > 0 and d["steps"] == 3
    assert d["roofline"]["launches"] > 0 and 0 < d["roofline"]["frac"] < 1
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "port"

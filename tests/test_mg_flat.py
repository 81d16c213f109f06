"""The flat forms of the multigrid's residual and correction,
k_residual_flat and k_prolong_flat (AFH_MG_FLAT, default on): constant-stencil
boxes of even nc >= 32 are swept flat over their ghosted planes in 16-byte
aligned pairs of cells, the x neighbours of a pair coming from the adjacent
lanes. AFH_MG_FLAT=0 restores k_residual and k_prolong.

Every GPU case writes a finite sentinel pattern into every cell of tmp and
of |E| (ghost layers included: the flat kernels store interior cells only),
runs field_compute with two V-cycles that read max|res| and two
bench.unit_steps, and compares
  (i)  the switch on against the switch off: every cell variable as a whole
       array, ghost layers included, the residual lists and the dt limits,
       all array_equal;
  (ii) on uni32 and amr32, the switch on against the C oracle, bitwise (phi
       with its ghost layers; of the other variables the interiors, as in
       tests/test_pair_xfetch.py: their ghost cells are left to the next fill
       by other launches on the two sides).

Trees, the smallest that reach each path:
  uni32  1 + 8 boxes of 32^3: rows of 17 pairs, 9 workgroups per box;
  uni64  1 + 8 boxes of 64^3: the flagship's box size;
  uni48  1 + 8 boxes of 48^3: rows of 25 pairs (an odd count), not a power
         of two;
  amr32  2 level-1 boxes of 32^3, one refined: leaves on two levels, so the
         leaves / parents lists differ and the one-launch all-levels residual
         takes its coefficients from the level table.
Variants: the gradient output (|E| from the residual pass) off, one residual
launch per level (AFH_ALL_LVL=0), columns of 4 and 8 for both kernels.
"""
import numpy as np
import pytest

from afh import capi
from afh.streamer import IV, N_VAR_CELL, StreamerCase, seed_state, tables_from
from afh.tree import build_tree, uniform_tree

SWITCHES = ("AFH_MG_FLAT", "AFH_ALL_LVL", "AFH_RES_K", "AFH_PROLONG_K")

TOPOS = {
    "uni32": lambda: uniform_tree(32, (32, 32, 32), (2e-3, 2e-3, 2e-3), 2),
    "uni64": lambda: uniform_tree(64, (64, 64, 64), (4e-3, 4e-3, 4e-3), 2),
    "uni48": lambda: uniform_tree(48, (48, 48, 48), (3e-3, 3e-3, 3e-3), 2),
    "amr32": lambda: build_tree(32, (64, 32, 32), (4e-3, 2e-3, 2e-3), 1,
                                refine=lambda lvl, r0, r1: lvl < 2 and r0[0] < 1e-3),
}
VARIANTS = {
    "default": ({}, True),
    "nograd": ({}, False),
    "per_level": ({"AFH_ALL_LVL": "0"}, True),
    "res_k4": ({"AFH_RES_K": "4"}, True),
    "res_k8": ({"AFH_RES_K": "8"}, True),
    "prolong_k4": ({"AFH_PROLONG_K": "4"}, True),
    "prolong_k8": ({"AFH_PROLONG_K": "8"}, True),
}
_topo_cache, _ref_cache = {}, {}


def _topo(name):
    if name not in _topo_cache:
        _topo_cache[name] = TOPOS[name]()
    return _topo_cache[name]


def _sentinel(shape, base):
    """Finite, different in every cell, nowhere near a computed value."""
    n = int(np.prod(shape))
    return (base + np.arange(n, dtype=np.float64) / n).reshape(shape)


def _run(lib, dev, name, monkeypatch, env, grad):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    import bench
    from afh import decks
    topo = _topo(name)
    td, chem = tables_from(decks.load("tables_air_siglo"))
    dom = np.asarray(topo["domain"], float)
    voltage = 2.5e6 * dom[2]
    c = StreamerCase(lib, topo, td, chem, voltage, device=dev, coarse_cycles=0)
    if grad:
        c.faces_from_phi(True)  # |E| from the final residual pass
    # off centre in every direction: no symmetry hides a swapped neighbour
    seed_state(c, r0=dom * np.array([0.37, 0.45, 0.55]), width=0.08 * dom[2])
    c.fuse_rhs(True, ghosts=False)
    c.tree.put_cc(IV["tmp"], _sentinel(c.tree.cc_shape, 7.0e33))
    c.tree.put_cc(IV["efld"], _sentinel(c.tree.cc_shape, -3.0e35))
    # (max_rel_residual=0: the second V-cycle runs whatever the first left)
    out = {"res0": c.field_compute(0, n_vcycles=2, max_rel_residual=0.0)}
    for k in range(2):
        out["step%d" % k] = bench.unit_step(c, 1e-13, k)
    for iv in range(1, N_VAR_CELL + 1):
        out[iv] = c.tree.get_cc(iv)
    c.tree.close()
    return out


def _same(a, b, what, interior_only=()):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            x, y = a[k], b[k]
            if k in interior_only:
                x, y = x[:, 1:-1, 1:-1, 1:-1], y[:, 1:-1, 1:-1, 1:-1]
            assert np.array_equal(x, y), (what, k, np.nanmax(np.abs(x - y)))
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


NOT_PHI = tuple(iv for iv in range(1, N_VAR_CELL + 1) if iv not in (IV["phi"], IV["phi_2"]))


def _oracle(name, monkeypatch, grad):
    """The C oracle's run, once per tree."""
    key = (name, grad)
    if key not in _ref_cache:
        _ref_cache[key] = _run(capi.oracle_library(), -1, name, monkeypatch, {}, grad)
    return _ref_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(TOPOS))
def test_flat_bitwise(name, variant, monkeypatch):
    env, grad = VARIANTS[variant]
    on = _run(capi.hip_library(), 0, name, monkeypatch, dict(env, AFH_MG_FLAT="1"), grad)
    off = _run(capi.hip_library(), 0, name, monkeypatch, dict(env, AFH_MG_FLAT="0"), grad)
    _same(on, off, "on / off")
    # two V-cycles read max|res|; the steps' residuals are deferred (stage 1
    # returns none, stage 2 one)
    assert len(on["res0"]) == 2 and len(on["step1"][0]) == 1
    # the solve did run: tmp's interior no longer holds the sentinel
    assert np.all(np.abs(on[IV["tmp"]][:, 1:-1, 1:-1, 1:-1]) < 1e30)
    if grad:
        assert np.all(on[IV["efld"]][:, 1:-1, 1:-1, 1:-1] >= 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("name", ["uni32", "amr32"])
def test_flat_equals_oracle(name, grad, monkeypatch):
    on = _run(capi.hip_library(), 0, name, monkeypatch, {"AFH_MG_FLAT": "1"}, grad)
    _same(on, _oracle(name, monkeypatch, grad), "on / oracle", NOT_PHI)

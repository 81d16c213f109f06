"""The fused pair k_gsrb_pair2 fetches the x ghost cells of the box it smooths
(a same-level neighbour's boundary cell from its old values, a physical face
by gc_face_nocopy), so the level fills that nothing but such a pair reads
leave out the x faces (all but their rim, which the pair reads through its y
and z neighbours): the fill between the pairs of a leg and the fill after the
correction. AFH_PAIR_XFETCH=0 restores the full fills.

Every GPU case runs a field solve and four bench.unit_steps and compares
every cell variable bitwise (phi with its ghost layers):
  (i)  the switch on against the switch off;
  (ii) the switch on against the C oracle (the reference's sequence: split
       half-sweeps, a full fill after each).
The oracle takes no periodic flag (afh.model.Tree clears it there, and its
level-1 solve then does not wrap), so on the periodic tree (ii) is held
against the library's own split half-sweeps with full fills instead, the form
tests/test_periodic_gpu.py and test_hip_parity.py hold to the oracle.

Trees, the smallest that reach each path (AFH_GSRB_FUSED_MIN_BOXES=1 fuses
their levels):
  uni32_l3  1 + 8 + 64 boxes of 32^3: the whole-box pair <32, 32, 2>
            (AFH_GSRB_TILES_MIN=0) and the quarter-box tiles <32, 8, 2>
            (AFH_GSRB_TILES=1), whose halo rows read the adjacent tile's x
            ghost cells;
  uni64_l2  1 + 8 boxes of 64^3: 16 chunks of 4 planes <64, 64, 1, 16> and
            the whole-box march <64, 64, 1, 1> (AFH_GSRB_TILES_MIN=0);
  amr32     2 level-1 boxes of 32^3, the low-x one refined: level 2 has a
            refinement boundary on its high x faces (the x-face list is not
            empty there) and a physical low x face;
  per32     periodic in x and one box wide in x on level 1: on level 2 both
            x neighbours of a box are the same box;
  uni32_l2  Dirichlet and inhomogeneous Neumann x walls; 1 and 3 pairs per
            leg (an odd count starts a leg with split half-sweeps, which need
            the full fill).
"""
import ctypes as C

import numpy as np
import pytest

from afh import capi
from afh.amr import AfTree
from afh.model import Multigrid, tree_desc
from afh.streamer import IV, N_VAR_CELL, StreamerCase, seed_state, tables_from
from afh.tree import build_tree, uniform_tree

SWITCHES = ("AFH_PAIR_XFETCH", "AFH_GSRB_FUSED_MIN_BOXES", "AFH_GSRB_TILES",
            "AFH_GSRB_TILES_MIN")
WHOLE = {"AFH_GSRB_TILES_MIN": "0"}
TILES = {"AFH_GSRB_TILES": "1"}


def _per32():
    dr = 2.0 ** -14
    af = AfTree(32, [32 * dr, 64 * dr, 64 * dr], [32, 64, 64], periodic=(True, False, False))
    af.refine_up_to_lvl(2)
    return af.topology()


TOPOS = {
    "uni32_l3": lambda: uniform_tree(32, (32, 32, 32), (4e-3, 4e-3, 4e-3), 3),
    "uni32_l2": lambda: uniform_tree(32, (32, 32, 32), (2e-3, 2e-3, 2e-3), 2),
    "uni64_l2": lambda: uniform_tree(64, (64, 64, 64), (4e-3, 4e-3, 4e-3), 2),
    "amr32": lambda: build_tree(32, (64, 32, 32), (4e-3, 2e-3, 2e-3), 1,
                                refine=lambda lvl, r0, r1: lvl < 2 and r0[0] < 1e-3),
    "per32": _per32,
}
_topo_cache, _ref_cache = {}, {}


def _topo(name):
    if name not in _topo_cache:
        _topo_cache[name] = TOPOS[name]()
    return _topo_cache[name]


# ------------------------------------------------------------- the x-face list
def _xrb_lib(topo, lvl):
    lib = C.CDLL(capi.HIP_LIB)
    fn = lib.afh_xface_rb_boxes
    fn.restype = C.c_int32
    fn.argtypes = [C.POINTER(capi.TreeDesc), C.c_int32, capi.P_i32, C.c_int32, capi.P_i32]
    d, _keep = tree_desc(topo, 1, 0)
    n = C.c_int32()
    assert fn(C.byref(d), lvl, None, 0, C.byref(n)) == 0
    out = np.zeros(max(n.value, 1), np.int32)
    assert fn(C.byref(d), lvl, out.ctypes.data_as(capi.P_i32), n.value, C.byref(n)) == 0
    return out[:n.value].tolist()


@pytest.mark.parametrize("name", sorted(TOPOS))
def test_xface_list_equals_the_topology(name):
    """The per-level list of boxes with a refinement boundary on an x face
    (their x faces stay in the fills without x faces) is what the topology
    says: neighbour 0 on face 1 or 2, in the level list's order. No GPU."""
    topo = _topo(name)
    nbs = np.asarray(topo["meta_neighbors"])
    total = 0
    for lvl in range(1, int(topo["highest_lvl"]) + 1):
        ids = np.asarray(topo["lvl_ids_%d" % lvl])
        want = [int(b) for b in ids if nbs[b - 1][0] == 0 or nbs[b - 1][1] == 0]
        assert _xrb_lib(topo, lvl) == want, (name, lvl)
        total += len(want)
    # amr32: the four level-2 boxes on the high x side of the refined box
    assert total == (4 if name == "amr32" else 0)


# -------------------------------------------------------------------- GPU runs
def _run(lib, dev, name, monkeypatch, env, xbc=None, n_cycle=2):
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
    if xbc is not None:
        bc = c.phi_bc(voltage)
        bc[0], bc[1] = xbc
        for s in (0, 1):
            c.tree.set_cc_methods(IV["phi"] + s, bc, capi.RB_MG_SIDES)
    if n_cycle != 2:
        c.mg.close()
        c.mg = Multigrid(c.tree, IV["phi"], IV["rhs"], IV["tmp"], n_cycle_down=n_cycle,
                         n_cycle_up=n_cycle, coarse_cycles=0)
    # off centre in every direction: no symmetry hides a swapped face
    seed_state(c, r0=dom * np.array([0.37, 0.45, 0.55]), width=0.08 * dom[2])
    c.fuse_rhs(True, ghosts=False)
    out = {"res0": c.field_compute(0, n_vcycles=2, check_residual=False)}
    for k in range(4):
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


# (ii) compares the ghost layers of phi; of the other variables the interiors
# (the species step with the rhs folded in leaves their ghost cells to the
# next fill, on both sides but not by the same launches)
NOT_PHI = tuple(iv for iv in range(1, N_VAR_CELL + 1) if iv not in (IV["phi"], IV["phi_2"]))


def _reference(name, monkeypatch, xbc, n_cycle):
    """The C oracle's run, once per tree and set-up; on the periodic tree
    the library's split half-sweeps with full fills (module docstring)."""
    key = (name, xbc, n_cycle)
    if key not in _ref_cache:
        if name == "per32":
            _ref_cache[key] = _run(capi.hip_library(), 0, name, monkeypatch,
                                   {"AFH_GSRB_FUSED_MIN_BOXES": "0"}, xbc, n_cycle)
        else:
            _ref_cache[key] = _run(capi.oracle_library(), -1, name, monkeypatch, {}, xbc, n_cycle)
    return _ref_cache[key]


def _check(name, form, monkeypatch, xbc=None, n_cycle=2):
    env = dict(form, AFH_GSRB_FUSED_MIN_BOXES="1")
    on = _run(capi.hip_library(), 0, name, monkeypatch, dict(env, AFH_PAIR_XFETCH="1"),
              xbc, n_cycle)
    off = _run(capi.hip_library(), 0, name, monkeypatch, dict(env, AFH_PAIR_XFETCH="0"),
               xbc, n_cycle)
    _same(on, off, "on / off")
    _same(on, _reference(name, monkeypatch, xbc, n_cycle), "on / reference", NOT_PHI)
    assert len(on["res0"]) == 0 and len(on["step3"][0]) == 1  # (deferred residuals)


@pytest.mark.gpu
@pytest.mark.parametrize("name,form", [
    ("uni32_l3", WHOLE), ("uni32_l3", TILES), ("uni64_l2", {}), ("uni64_l2", WHOLE),
    ("amr32", WHOLE), ("amr32", TILES), ("per32", WHOLE), ("per32", TILES)],
    ids=lambda v: v if isinstance(v, str) else "-".join(sorted(v)) or "default")
def test_xfetch_bitwise(name, form, monkeypatch):
    _check(name, form, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["uni32_l2", "amr32"])
def test_fills_without_x_faces_run(name, monkeypatch):
    """The switch does change the fills: over one V(2,2)-cycle the fills of
    the tree are as many and fill fewer cells (the library's own count of
    algorithmic bytes: 16 B per ghost cell filled). Level 2 of uni32_l2: five fills
    of 8 boxes, three of them with 4 nc + 8 rows of nc cells instead of 6 nc;
    on amr32 the four boxes of the x-face list add their 2 nc rows back."""
    from afh import decks
    got = {}
    for on in ("1", "0"):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("AFH_GSRB_FUSED_MIN_BOXES", "1")
        monkeypatch.setenv("AFH_PAIR_XFETCH", on)
        monkeypatch.setenv("AFH_GRAPHS", "0")
        topo = _topo(name)
        td, chem = tables_from(decks.load("tables_air_siglo"))
        c = StreamerCase(capi.hip_library(), topo, td, chem, 5e3, device=0, coarse_cycles=0)
        seed_state(c)
        c.fluid.field_set_rhs(IV["rhs"], 0)
        c.mg.fas_vcycle(False)  # (ghost cells current from here on)
        c.lib.call("profile_enable", c.tree.h, capi.PROF_GHOST)
        c.mg.fas_vcycle(False)
        ms, nl, by = C.c_double(), C.c_int64(), C.c_double()
        c.lib.call("profile_read", c.tree.h, C.byref(ms), C.byref(nl), C.byref(by))
        got[on] = (nl.value, by.value)
        c.tree.close()
    nc, n = 32, 8
    full = 16.0 * nc * 6 * nc * n
    free = 16.0 * nc * ((4 * nc + 8) * n + (2 * nc * 4 if name == "amr32" else 0))
    print(name, got)
    assert got["1"][0] == got["0"][0]
    assert got["0"][1] - got["1"][1] == 3 * (full - free)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dirichlet", "neumann"])
def test_xfetch_physical_x_walls(kind, monkeypatch):
    """Physical x faces with values that are not zero: the pair's own
    gc_face_nocopy against k_gc_faces'."""
    xbc = {"dirichlet": ((capi.BC_DIRICHLET, 350.0), (capi.BC_DIRICHLET, -120.0)),
           "neumann": ((capi.BC_NEUMANN, 4e5), (capi.BC_NEUMANN, -7e5))}[kind]
    _check("uni32_l2", WHOLE, monkeypatch, xbc=xbc)
    _check("uni32_l2", TILES, monkeypatch, xbc=xbc)


@pytest.mark.gpu
@pytest.mark.parametrize("n_cycle", [1, 3])
def test_xfetch_odd_pair_counts(n_cycle, monkeypatch):
    """n_cycle_up = n_cycle_down = 1 and 3: a leg starts with split
    half-sweeps, which read the x ghost cells of the fill before them."""
    _check("uni32_l2", WHOLE, monkeypatch, n_cycle=n_cycle)

"""The reductions of include/afivo_hip_analysis.h and the simulation log on
the GPU, in both libraries.

There is no reference program for output_log, so the reductions are held to
tests/analysis_numpy.py, a numpy restatement of the Fortran (float64, in the
order written) on the arrays get_cc / get_fc return. Every reduction is a
selection of a stored value or a cell-centre coordinate formed by one
expression, so every comparison is bitwise, locations included.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import analysis_numpy as an
import golden
import state2d
from afh import capi, simlog
from afh.amr import AF_CYL, AF_XYZ, DO_REF, KEEP_REF, AfTree
from afh.driver import Case, Simulation
from afh.model import Tree

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -2
PFMG = dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
LEN = 2e-3
MAX, MIN = capi.RED_MAX, capi.RED_MIN

# (kind, ndim, box size): "two" one level-1 box refined once; "amr" leaves on
# three levels (2-D at 8: the tree of tests/state2d.py); "cyl" cylindrical;
# "per" periodic in the first (3-D: and last) dimension
TREES = [("two", 2, 4), ("two", 2, 8), ("two", 2, 6), ("amr", 2, 8), ("amr", 2, 6),
         ("two", 3, 4), ("two", 3, 8), ("two", 3, 6), ("amr", 3, 4), ("amr", 3, 8),
         ("amr", 3, 6), ("cyl", 2, 8), ("per", 2, 8), ("per", 3, 8)]
PREPARED = [("amr", 2, 8), ("two", 2, 4), ("amr", 3, 6), ("per", 3, 8)]


def _lib(nd):
    return capi.hip_library_2d() if nd == 2 else capi.hip_library()


def _code(exc):
    return int(re.search(r"failed \((-?\d+)\)", str(exc.value)).group(1))


@functools.lru_cache(maxsize=None)
def _af(kind, nd, nc):
    if kind == "amr" and nd == 2 and nc == 8:
        return state2d.build_tree(Case(golden.load("rtest_test_2d")), 4, 7, (0.5, 0.3), 0.08)
    if kind in ("two", "cyl"):
        af = AfTree(nc, [LEN] * nd, [nc] * nd, coord=AF_CYL if kind == "cyl" else AF_XYZ)
        af.refine_up_to_lvl(2)
        return af
    per = (True, False, True)[:nd] if kind == "per" else None
    af = AfTree(nc, [LEN] * nd, [2 * nc] * nd, periodic=per)
    for lvl in (1, 2):  # the box at the origin, then its child there
        def fn(ids, lvl=lvl):
            f = [DO_REF if (af.lvl[b] == lvl and np.all(af.r_min[b] < 0.2 * LEN)) else KEEP_REF
                 for b in ids]
            return np.array(f), np.zeros(len(ids), np.uint32)
        af.adjust_refinement(fn)
    return af


def _make(kind, nd, nc, seed=3):
    """(AfTree, device tree with 2 cell and 1 face variable, random normal cc
    and fc arrays as uploaded)."""
    af = _af(kind, nd, nc)
    t = Tree(_lib(nd), af.topology(), 2, 1, device=0)
    if kind == "cyl":
        t.set_coord(capi.COORD_CYL)
    t.set_cc_methods(1, [(capi.BC_NEUMANN, 0.0)] * 6)
    rng = np.random.default_rng(seed)
    cc, fc = rng.standard_normal(t.cc_shape), rng.standard_normal(t.fc_shape)
    t.put_cc(1, cc)
    t.put_fc(1, fc)
    return af, t, cc, fc


def _cell(nd, b, i, j, k=1):
    """Index of cell / face (i, j[, k]) (1-based) of box b in a get_cc array
    (for a get_fc array: shift by -1 and insert the direction)."""
    return (b - 1,) + ((k,) if nd == 3 else ()) + (j, i)


def _face(nd, b, dim, i, j, k=1):
    return (b - 1, dim - 1) + ((k - 1,) if nd == 3 else ()) + (j - 1, i - 1)


def test_trees():
    for kind, nd, nc in TREES:
        af = _af(kind, nd, nc)
        lv = {af.lvl[b] for b in af.leaves()}
        assert af.nc == nc and af.ndim == nd
        assert len(lv) >= 3 if kind in ("amr", "per") else lv == {2}
    # (several workgroups of leaves: four 8^2 boxes to a workgroup)
    assert len(_af("amr", 2, 8).leaves()) > 16


# ------------------------------------------------------------- reduce_fc
@pytest.mark.parametrize("kind,nd,nc", TREES)
def test_reduce_fc(kind, nd, nc):
    af, t, _, fc = _make(kind, nd, nc)
    got_fc = t.get_fc(1)
    assert np.array_equal(got_fc, fc)
    for dim in range(1, nd + 1):
        for op in (MAX, MIN):
            ref = an.reduce_fc(af.leaves(), got_fc, nc, nd, dim, op == MIN)
            got = t.reduce_fc(1, dim, op)
            assert got == ref, (dim, op)
            assert t.reduce_fc(1, dim, op) == got  # repeatable
            assert t.reduce_fc(1, dim, op, with_loc=False) == (ref[0], None)
    t.close()


@pytest.mark.parametrize("kind,nd,nc", PREPARED)
def test_reduce_fc_prepared(kind, nd, nc):
    af, t, _, fc = _make(kind, nd, nc)
    leaves = af.leaves()
    parent = next(b for b in range(1, af.highest_id + 1) if af.in_use[b] and af.has_children(b))
    for dim in range(1, nd + 1):
        for op, big in ((MAX, 100.0), (MIN, -100.0)):
            # on an upper-boundary face (index nc + 1 along dim) of a leaf
            a = fc.copy()
            b = leaves[len(leaves) // 2]
            ijk = [2, 3, 1][:nd]
            ijk[dim - 1] = nc + 1
            a[_face(nd, b, dim, *ijk)] = big
            # a larger one on a box that is no leaf: ignored
            a[_face(nd, parent, dim, *ijk)] = 10 * big
            t.put_fc(1, a)
            got = t.reduce_fc(1, dim, op)
            assert got == (big, (b,) + tuple(ijk) + (0,) * (3 - nd))
            assert got == an.reduce_fc(leaves, a, nc, nd, dim, op == MIN)
            # the same value in two cells of one leaf and in a later leaf:
            # the first cell (i fastest) of the first leaf
            a = fc.copy()
            b1, b2 = leaves[1], leaves[-1]
            for bb, (i, j) in ((b1, (3, 2)), (b1, (4, 1)), (b2, (1, 1))):
                a[_face(nd, bb, dim, i, j)] = big
            t.put_fc(1, a)
            got = t.reduce_fc(1, dim, op)
            assert got == (big, (b1, 4, 1) + ((1,) if nd == 3 else (0,)))
            assert got == an.reduce_fc(leaves, a, nc, nd, dim, op == MIN)
    t.close()


# ----------------------------------------------------- zminmax_threshold
@pytest.mark.parametrize("kind,nd,nc", TREES)
def test_zminmax_threshold(kind, nd, nc):
    af, t, cc, _ = _make(kind, nd, nc)
    leaves = af.leaves()
    lo, hi = float(af.r_base[nd - 1]), float(af.domain[nd - 1])
    lim = [hi, lo]
    # (the ghost cells hold larger values than any interior: never read)
    inner = (slice(None),) + (slice(1, -1),) * nd
    a = cc + 50.0
    a[inner] = cc[inner]
    t.put_cc(1, a)
    for thr in (0.5, 2.0, 3.0, -10.0):
        ref = an.zminmax(leaves, a, af.r_min, af.dr, nc, nd, thr, lim)
        assert t.zminmax_threshold(1, thr, lim) == ref, thr
        assert t.zminmax_threshold(1, thr, lim) == ref
    top = max(a[b - 1][inner[1:]].max() for b in leaves)
    assert t.zminmax_threshold(1, top, lim) == (hi, lo)  # > : equal does not count
    assert t.zminmax_threshold(1, 40.0, [0.25, 0.75]) == (0.25, 0.75)
    below = np.nextafter(top, -np.inf)
    ref = an.zminmax(leaves, a, af.r_min, af.dr, nc, nd, below, lim)
    assert ref[0] == ref[1] and lo < ref[0] < hi
    assert t.zminmax_threshold(1, below, lim) == ref
    # the kept quirk: planes 2 and nc - 1 of one leaf above, nothing else on
    # the tree: both entries are plane 2's centre
    a = np.zeros_like(cc)
    b = leaves[len(leaves) // 3]
    for n in (2, nc - 1):
        a[_cell(nd, b, 1, n) if nd == 2 else _cell(nd, b, 2, 1, n)] = 1.0
    t.put_cc(1, a)
    z2 = af.r_min[b][nd - 1] + 1.5 * af.dr[b][nd - 1]
    assert t.zminmax_threshold(1, 0.5, [1e100, -1e100]) == (z2, z2)
    assert an.zminmax(leaves, a, af.r_min, af.dr, nc, nd, 0.5, [1e100, -1e100]) == (z2, z2)
    t.close()


# ------------------------------------------------------------ max_region
@pytest.mark.parametrize("kind,nd,nc", TREES)
def test_max_region(kind, nd, nc):
    af, t, cc, _ = _make(kind, nd, nc)
    leaves = af.leaves()
    args = (leaves, cc, af.r_min, af.dr, nc, nd)
    whole = (af.r_base.copy(), af.domain.copy())
    top, loc = t.reduce_loc(1, MAX)
    assert t.max_region(1, *whole) == (top, loc) == an.max_region(*args, *whole)
    # a window inside the leaf farthest from the one holding the maximum
    mid = {b: af.r_min[b] + 0.5 * nc * af.dr[b] for b in leaves}
    far = max(leaves, key=lambda b: np.linalg.norm(mid[b] - mid[loc[0]]))
    w = (mid[far] - 0.25 * nc * af.dr[far], mid[far] + 0.25 * nc * af.dr[far])
    ref = an.max_region(*args, *w)
    assert ref[0] < top and ref[1][0] != loc[0]
    assert t.max_region(1, *w) == ref
    assert t.max_region(1, *w) == ref
    assert t.max_region(1, *w, with_loc=False) == (ref[0], None)
    # a window whose edge is a box edge: the boxes on both sides take part
    b = next(b for b in leaves if af.r_min[b][0] > af.r_base[0])
    for side, a in ((0, cc.copy()), (1, cc.copy())):
        # (the prepared maximum lies in b, which the window only touches)
        a[_cell(nd, b, 2, 2, 2)] = 100.0
        t.put_cc(1, a)
        w = (af.r_base.copy(), af.domain.copy())
        if side == 0:
            w[1][0] = af.r_min[b][0]
        else:
            w[0][0] = af.r_min[b][0] + nc * af.dr[b][0]
        ref = an.max_region(leaves, a, af.r_min, af.dr, nc, nd, *w)
        assert ref == (100.0, (b, 2, 2) + ((2,) if nd == 3 else (0,)))
        assert t.max_region(1, *w) == ref
    # outside the domain
    out = (af.domain + 1.0, af.domain + 2.0)
    assert t.max_region(1, *out) == (-1e100, an.no_loc(nd)) == an.max_region(*args, *out)
    t.close()


# ---------------------------------------------------------- local_maxima
@pytest.mark.parametrize("kind,nd,nc", TREES)
def test_local_maxima(kind, nd, nc):
    af, t, _, _ = _make(kind, nd, nc)
    leaves = af.leaves()
    t.gc_tree(1)
    a = t.get_cc(1)
    for thr in (0.0, 1.0):
        ref = an.local_maxima(leaves, a, af.r_min, af.dr, nc, nd, thr)
        assert len(ref) > len(leaves) // 8
        none, n = t.local_maxima(1, thr, 0)
        assert n == len(ref) and none.shape == (0, nd + 1)
        got, n = t.local_maxima(1, thr, len(ref) + 3)
        assert n == len(ref) and np.array_equal(got, ref)
        got2, n2 = t.local_maxima(1, thr, len(ref) + 3)
        assert n2 == n and np.array_equal(got2, got)
        few = max(1, len(ref) // 2)
        got, n = t.local_maxima(1, thr, few)
        assert n == len(ref) and np.array_equal(got, ref[:few])
    # a plateau: two equal neighbouring cells above all others are both maxima
    a = np.zeros(t.cc_shape)
    b = leaves[-1]
    a[_cell(nd, b, 2, 2, 2)] = a[_cell(nd, b, 3, 2, 2)] = 5.0
    t.put_cc(1, a)
    t.gc_tree(1)
    got, n = t.local_maxima(1, 1.0)
    ref = an.local_maxima(leaves, t.get_cc(1), af.r_min, af.dr, nc, nd, 1.0)
    assert n == 2 and np.array_equal(got, ref) and got[:, nd].tolist() == [5.0, 5.0]
    assert got[1, 0] - got[0, 0] == pytest.approx(af.dr[b][0]) and got[0, 1] == got[1, 1]
    # a flat field has none
    t.put_cc(1, np.full(t.cc_shape, 2.0))
    assert t.local_maxima(1, 1.0)[1] == 0
    t.close()


# ------------------------------------------------------------ error codes
@pytest.mark.parametrize("nd", [2, 3])
def test_error_codes(nd):
    af, t, _, _ = _make("two", nd, 4)
    z3 = np.zeros(3)
    bad = [lambda: t.reduce_fc(0, 1, MAX), lambda: t.reduce_fc(2, 1, MAX),
           lambda: t.reduce_fc(1, 0, MAX), lambda: t.reduce_fc(1, nd + 1, MAX),
           lambda: t.reduce_fc(1, 1, 0), lambda: t.reduce_fc(1, 1, capi.RED_MAXABS),
           lambda: t.zminmax_threshold(0, 0.0, [1.0, 0.0]),
           lambda: t.zminmax_threshold(3, 0.0, [1.0, 0.0]),
           lambda: t.max_region(0, z3[:nd], z3[:nd]), lambda: t.max_region(3, z3[:nd], z3[:nd]),
           lambda: t.local_maxima(0, 0.0), lambda: t.local_maxima(3, 0.0),
           lambda: t.local_maxima(1, 0.0, -1)]
    for k, call in enumerate(bad):
        with pytest.raises(capi.AfhError) as e:
            call()
        assert _code(e) == ERR_ARG, k
    # a NULL loc is accepted
    assert t.reduce_fc(1, 1, MAX, with_loc=False)[1] is None
    assert t.max_region(1, z3[:nd], z3[:nd] + LEN, with_loc=False)[1] is None
    t.close()


def test_sharded_tree_is_refused():
    af, t, _, _ = _make("two", 3, 4)
    hook = capi.HOOK_FN(lambda *a: 0)
    t.lib.call("tree_set_hook", t.h, C.cast(hook, C.c_void_p), None)
    z3 = np.zeros(3)
    for call in (lambda: t.reduce_fc(1, 1, MAX), lambda: t.zminmax_threshold(1, 0.0, [1.0, 0.0]),
                 lambda: t.max_region(1, z3, z3 + LEN), lambda: t.local_maxima(1, 0.0)):
        with pytest.raises(capi.AfhError, match="sharded") as e:
            call()
        assert _code(e) == ERR_UNSUPPORTED
    t.lib.call("tree_set_hook", t.h, None, None)
    assert t.reduce_fc(1, 1, MAX)[1][0] > 0
    t.close()


# ------------------------------------------------------------- the driver
def _run(name, log, extra=None):
    """The driver until its second output (the initial one and one more)."""
    d = dict(golden.load(name))
    d.update(extra or {})
    nd = len(d["coarse_grid_size_value"])
    sim = Simulation(_lib(nd), d, device=0, log=log, **(PFMG if nd == 2 else {}))
    sim.start()
    while len(sim.log) < 2 and sim.step():
        pass
    return sim


def _restated(sim):
    """analysis_numpy.log_columns on the arrays fetched from the run."""
    af, nd = sim.af, sim.ndim
    thr = sim.density_threshold * (sim.N / 2.414e25) ** 2
    return an.log_columns(af.leaves(), sim.tree.get_cc(sim.i_electron),
                          sim.tree.get_cc(sim.i_efld), sim.tree.get_fc(sim.f_field),
                          af.r_min, af.dr, af.nc, nd, sim.origin, sim.L, thr)


@pytest.mark.parametrize("name", ["rtest_test_2d", "rtest_test_cyl", "rtest_test_3d"])
def test_driver_log(name, tmp_path):
    plain = _run(name, False)
    # output%density_threshold such that the scaled threshold is a tenth of
    # the largest electron density (the default, 1e18, lies above every
    # density of some of these cases: the extent then stays at its limits)
    thr = 0.1 * plain.tree.max_cc(plain.i_electron) / (plain.N / 2.414e25) ** 2
    sim = _run(name, True, {"output%density_threshold": np.array([thr])})
    nd = sim.ndim
    # the regression rows are bitwise those of a run without the log
    assert len(sim.log) == 2 and np.array_equal(np.array(sim.log), np.array(plain.log))
    plain.tree.close()
    assert len(sim.sim_log) == 2
    names = simlog.header_line(nd).split()
    assert all(len(r) == len(names) for r in sim.sim_log)
    col = {n: k for k, n in reversed(list(enumerate(names)))}  # a name's first column
    first, second = sim.sim_log
    assert first[col["v"]] == 0.0 and first[col["it"]] == 0 and second[col["it"]] == 1
    # the row of the final state against the restatement, bitwise
    before = [sim.tree.get_cc(iv) for iv in range(1, sim.n_var_cell + 1)]
    d, row = sim.log_row()
    d2, row2 = sim.log_row()
    d.pop("wc_time"), d2.pop("wc_time")
    assert d == d2  # repeatable; and no cell changed
    for iv, a in enumerate(before, 1):
        assert np.array_equal(sim.tree.get_cc(iv), a, equal_nan=True), iv
    ref = _restated(sim)
    assert set(ref) <= set(d)
    for k, v in ref.items():
        assert d[k] == v, (k, d[k], v)
    assert d["max(E)"] == sim.tree.max_cc(sim.i_efld) > 0
    lo, hi = sim.origin[nd - 1], sim.origin[nd - 1] + sim.L[nd - 1]
    assert lo < d["ne_zmin"] <= d["ne_zmax"] < hi
    assert 0 < d["max(Etip)"] <= d["max(E)"] and any(x != 0 for x in d["r(Etip)"])
    sim.density_threshold = 1e18
    d18 = sim.log_row()[0]
    ref18 = _restated(sim)
    assert all(d18[k] == v for k, v in ref18.items())
    assert d18["ne_zmin"] >= d["ne_zmin"] and d18["ne_zmax"] <= d["ne_zmax"]
    sim.density_threshold = thr
    if nd == 2:
        assert d["min(E_r)"] <= d["max(E_r)"]
    assert len(row) == len(names) and row[col["max(E)"]] == d["max(E)"]
    assert second[col["v"]] >= 0.0
    # the sums and the currents are the diagnostics'
    dg = sim.diagnostics()
    assert d["sum(J.E)"] == dg["global_JdotE"] and d["sum(J.E)"] != 0
    assert d["current_J.E"] == dg["JdotE_current"]
    assert d["current_displ"] == dg["displ_current"]
    assert d["sum(n_e)"] == sim.tree.sum_cc(sim.i_electron)
    assert d["sum(n_i)"] == sim.tree.sum_cc(sim.i_1pos_ion)
    charge = 0.0
    for n in range(sim.n_gas, len(sim.species_list)):
        if sim.species_charge[n] != 0:
            charge = charge + sim.tree.sum_cc(sim.species_itree[n]) * sim.species_charge[n]
    assert d["sum(charge)"] == charge
    # the mesh columns are the host tree's
    assert d["n_cells"] == len(sim.af.leaves()) * sim.af.nc ** nd
    assert d["min(dx)"] == sim.af.min_dr() and d["highest(lvl)"] == sim.af.highest_lvl
    assert d["dt_limits"] == sim.dt_limits and min(d["dt_limits"]) > 0
    assert (d["it"], d["time"], d["dt"]) == (sim.output_cnt, sim.global_time, sim.global_dt)
    # prev_pos is not in the .dat record: the first row after a restart has
    # v = 0 (afh.datfile writes 3-D trees only)
    if nd == 3:
        sim.write_dat(str(tmp_path / "run"))
        e = dict(golden.load(name))
        e["output%density_threshold"] = np.array([thr])
        other = Simulation(_lib(3), e, device=0, log=True)
        other.restart(str(tmp_path / "run.dat"))
        d3 = other.log_row(advance=True)[0]
        assert d3["v"] == 0.0 and other.log_prev_pos == d["r(E)"]
        assert all(d3[k] == v for k, v in ref.items())
        other.tree.close()
    # the file reads back to the eight printed digits
    sim.write_log(str(tmp_path / "run_log.txt"))
    assert open(tmp_path / "run_log.txt").readline().split() == names
    back = np.loadtxt(tmp_path / "run_log.txt", skiprows=1)
    want = np.array(sim.sim_log, float)
    assert back.shape == want.shape
    assert np.all(np.abs(back - want) <= 0.5000001e-7 * np.abs(want))
    sim.tree.close()


def test_driver_field_maxima(tmp_path):
    extra = {"field_maxima%write": np.array([1]), "field_maxima%threshold": np.array([1e5]),
             "field_maxima%distance": np.array([2e-4])}
    sim = _run("rtest_test_2d", False, extra)
    got = sim.field_maxima()
    a = sim.tree.get_cc(sim.i_efld)
    af = sim.af
    rows = an.local_maxima(af.leaves(), a, af.r_min, af.dr, af.nc, 2, 1e5)
    ref = an.merge_maxima(rows[:1000], len(rows), 2e-4, 1e5)
    assert len(rows) >= 1 and len(ref) >= 1 and np.array_equal(got, ref)
    sim.write_field_maxima(str(tmp_path / "run_Emax_000001.txt"))
    assert np.array_equal(np.loadtxt(tmp_path / "run_Emax_000001.txt", ndmin=2), ref)
    sim.tree.close()

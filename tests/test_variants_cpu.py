"""Every limiter and every boundary-condition type, on the CPU.

The reference's compiled afivo numerics (oracle/harness/variants_gen.f90,
packed by oracle/make_variants.py into tests/golden/variants3d.npz and
variants2d.npz) ran, on a small three-level tree with a lattice-valued input:
flux_upwind_tree with each of the seven flux limiters and with each of the
seven prolongation limiters of the species' second ghost layer, af_gc_tree
under four rotations of the four boundary types over the faces (af_gc_interp
and af_gc_interp_lim), and the flux with Dirichlet, Neumann and
dirichlet_copy faces of non-zero value (bc_to_gc2 and its high-y quirk).

Here: the C oracle against those fixtures (ghost cells bitwise; fluxes and
limits within test_oracle_golden.TOL_EXACT -- they are in fact bitwise, which
is asserted too); a numpy statement of the limiters and of
af_prolong_limit (tests/variants_numpy.py) against the oracle's regrid of a
uniform level into refined boxes, bitwise; the 2-D fixture against the numpy
statement of the 2-D flux; the two refusals (a potential boundary that is
neither Dirichlet nor Neumann; AFH_BC_CONTINUOUS on a flux species); and the
branch census: every input a limiter test uses reaches every branch of the
Koren and generalised minmod limiters, equalities included, at least three
times along every dimension.

test_variants_gpu.py holds the HIP side and imports the builders below.
"""
import re

import numpy as np
import pytest

import golden
import variants_numpy as vn
from afh import capi
from afh.amr import AfTree, DO_REF, KEEP_REF
from afh.model import Fluid, Multigrid, Tree
from afh.streamer import FV, IV, N_VAR_CELL, standard_reactions, tables_from
from test_oracle_golden import TOL_EXACT

ERR_UNSUPPORTED = -2
RB = {"interp": capi.RB_GC_INTERP, "interp_lim": capi.RB_GC_INTERP_LIM,
      "mg_sides": capi.RB_MG_SIDES}
FOUR_TYPES = (capi.BC_DIRICHLET, capi.BC_NEUMANN, capi.BC_CONTINUOUS, capi.BC_DIRICHLET_COPY)
BFLUX_TYPES = (capi.BC_DIRICHLET, capi.BC_NEUMANN, capi.BC_DIRICHLET_COPY)
# mobile ions of the 3-D ion tests: (species, face variable, mobility x N)
IONS = [(2, 3, 5.0e21), (3, 4, 7.5e21)]


def code_of(exc):
    return int(re.search(r"failed \((-?\d+)\)", str(exc.value)).group(1))


def fixture(ndim):
    return golden.load("variants%dd" % ndim)


# ---------------------------------------------------------------------- trees
def variants_tree(nc, ndim):
    """The harness' tree at box size nc: level 1 (one box in 3-D, 4 x 4 in
    2-D) refined, then its children at the two opposite corners of the
    domain refined: three levels, refinement boundaries with the fine side
    on level 3 in every face direction."""
    n1 = 1 if ndim == 3 else 4
    af = AfTree(nc, [2.0 ** -10] * ndim, [n1 * nc] * ndim)

    def fn(ids):
        f = []
        for b in ids:
            ix = tuple(af.ix[b][:ndim])
            corner = ix == (1,) * ndim or ix == (2 * n1,) * ndim
            f.append(DO_REF if af.lvl[b] == 1 or (af.lvl[b] == 2 and corner) else KEEP_REF)
        return np.array(f), np.zeros(len(ids), np.uint32)

    af.adjust_refinement(fn)
    af.adjust_refinement(fn)
    assert af.highest_lvl == 3
    return af.topology()


def two_box_tree(nc, ndim=3):
    """One level, two boxes side by side in x: an interior face and every
    physical boundary."""
    af = AfTree(nc, [2.0 ** -9] + [2.0 ** -10] * (ndim - 1), [2 * nc] + [nc] * (ndim - 1))
    return af.topology()


def bc_values(types, ndim):
    """The harness' face_value: non-zero, another on every face, a small
    integer times a power of two."""
    return [(int(t), (nb + 1) * 2.0 ** 60 if t == capi.BC_NEUMANN else (nb + 2) * 2.0 ** 50)
            for nb, t in enumerate(types[:2 * ndim])]


def rotation(r, ndim):
    """Rotation r of the four types over the faces: every face sees every
    type over r = 0..3."""
    return bc_values([FOUR_TYPES[(nb + r) % 4] for nb in range(2 * ndim)], ndim)


def assignment(a, ndim):
    """Dirichlet (0), Neumann (1) or dirichlet_copy (2) on every face."""
    return bc_values([BFLUX_TYPES[a]] * (2 * ndim), ndim)


# --------------------------------------------------------------------- inputs
def lattice_inputs(topo, seed, n_face=2):
    """Densities of the three species k 2^50, |E| (1 + k) 2^20, a face field
    (k - 4) 2^18 and a potential 16 k whose gradient has both signs along
    every dimension."""
    nb, nc, nd = int(topo["n_boxes"]), int(topo["nc"]), int(topo.get("ndim", 3))
    rng = np.random.default_rng(seed)
    cs, fs = (nb,) + (nc + 2,) * nd, (nb, nd) + (nc + 1,) * nd
    x = {"e": vn.lattice(rng, cs), "pos": vn.lattice(rng, cs), "neg": vn.lattice(rng, cs)}
    x["efld"] = (1.0 + rng.integers(0, 9, cs)) * 2.0 ** 20
    x["fc_field"] = (rng.integers(0, 9, fs) - 4.0) * 2.0 ** 18
    x["phi"] = 16.0 * rng.integers(0, 9, cs)
    # the slope pairs on which the two sides of a Koren threshold differ:
    # electrons and negative ions take them against the field, positive ions
    # along it
    sites = edge_sites(topo)
    for s in ("e", "pos", "neg"):
        vn.plant_koren_edges(x[s], nd, sites, reverse=(s == "pos"))
    vn.plant_edge_fields(x["fc_field"], x["phi"], nd, sites)
    return x


def edge_sites(topo):
    """(box, offset) of the planted slope pairs: the first three leaves of
    level 2, as the harness; on a one-level tree two places in each of its
    first two boxes."""
    if int(topo["highest_lvl"]) >= 2:
        return [(int(b) - 1, 0) for b in topo["lvl_leaves_2"][:3]]
    if int(topo["nc"]) < 8:  # (the refusal tests' tree: no limiter test uses it)
        return []
    return [(b, o) for b in (0, 1) for o in (0, 4)]


def fixture_inputs(g):
    nd = int(g.get("ndim", 3))
    x = lattice_inputs(g, 5)
    x.update(e=g["in_e"], efld=g["in_efld"], fc_field=g["in_fc_field"])
    assert x["e"].shape == (int(g["n_boxes"]),) + (int(g["nc"]) + 2,) * nd
    return x


# ---------------------------------------------------------------------- cases
class FluxCase:
    """A tree with the streamer's variables and a fluid on it, the species'
    boundary, refinement-boundary method and limiters open."""

    def __init__(self, lib, dev, topo, tabs, limiter=capi.LIM_KOREN, bc=None, prolong=None,
                 rb=capi.RB_GC_INTERP_LIM, ions=(), phi=False, cyl=False):
        td, chem = tables_from(tabs)
        self.lib, self.topo = lib, topo
        self.nd = int(topo.get("ndim", 3))
        n0 = [(capi.BC_NEUMANN, 0.0)] * (2 * self.nd)
        self.tree = t = Tree(lib, topo, N_VAR_CELL, 2 + len(ions), device=dev)
        if cyl:
            t.set_coord(capi.COORD_CYL)
        for sp in ("e", "pos", "neg"):
            for s in range(3):
                t.set_cc_methods(IV[sp] + s, bc or n0, rb, prolong)
        t.set_cc_methods(IV["efld"], n0, capi.RB_GC_INTERP)
        t.set_cc_methods(IV["phi"], n0, capi.RB_GC_INTERP)
        self.ions = list(ions)
        self.fluid = Fluid(t, [IV["e"], IV["pos"], IV["neg"]], [-1, 1, -1], IV["e"],
                           IV["efld"], FV["flux"], FV["field"],
                           float(tabs["gas_number_density"]), td, chem, standard_reactions(),
                           limiter=limiter, ions=self.ions)
        if phi:
            self.fluid.set_field_source(IV["phi"], -1.0)

    def put(self, x):
        for k, v in x.items():
            if k.startswith("fc_"):
                self.tree.put_fc(FV[k[3:]], v)
            else:
                self.tree.put_cc(IV[k], v)

    def flux(self):
        """afh_flux_upwind_tree: ([face fluxes of every flux species], the
        densities with the ghost layer written back, (dt_cfl, dt_drt))."""
        lim = self.fluid.flux_upwind_tree(0)
        F = [self.tree.get_fc(fv) for fv in [FV["flux"]] + [q[1] for q in self.ions]]
        sp = ["e"] + [("e", "pos", "neg")[q[0] - 1] for q in self.ions]
        return F, [self.tree.get_cc(IV[s]) for s in sp], lim

    def close(self):
        self.tree.close()


def run_flux(lib, dev, topo, tabs, x, **kw):
    c = FluxCase(lib, dev, topo, tabs, **kw)
    c.put(x)
    out = c.flux()
    c.close()
    return out


def leaf_faces(F, topo):
    """The face entries the leaves own, per dimension."""
    return golden.faces(F[vn.leaves(topo)])


def census_after_flux(cc_after, topo, what):
    """The census on what the flux read: the leaves' cells with the ghost
    layer the flux wrote back."""
    nd = int(topo.get("ndim", 3))
    for c in cc_after:
        vn.assert_census(c[vn.leaves(topo)], nd, what)


# -------------------------------------------------- numpy limiters, by hand
def test_limiter_equalities_by_hand():
    """The branch a pair on an equality takes, m_af_limiters.f90:81-94 and
    139-149: (1, 4) is on aa = ab / 4 and takes 2 a; (5, 2) is on aa = 2.5 ab
    and takes (b + 2 a) / 3; (3, 5) is on the tie of theta = 4 / 3."""
    assert vn.koren(1.0, 4.0) == 2.0
    assert vn.koren(1.0, 4.0 + 2 ** -40) == 2.0 and vn.koren(1.0, 4.0 - 2 ** -40) != 2.0
    assert vn.koren(5.0, 2.0) == (1 / 3.0) * (2.0 + 10.0)
    assert vn.koren(5.0 + 2 ** -40, 2.0) == 4.0
    assert vn.koren(0.0, 3.0) == 0.0 and vn.koren(-1.0, 3.0) == 0.0
    assert vn.vanleer(0.0, 2.0) == 0.0 and vn.vanleer(1.0, 3.0) == 1.5
    assert vn.limiter(vn.LIM_MINMOD, 2.0, 3.0) == 2.0
    assert vn.limiter(vn.LIM_MINMOD, -3.0, -2.0) == -2.0
    assert vn.limiter(vn.LIM_MC, 1.0, 5.0) == 2.0 and vn.limiter(vn.LIM_MC, 2.0, 3.0) == 2.5
    assert vn.limiter(vn.LIM_GMINMOD43, 3.0, 5.0) == 4.0
    assert vn.limiter(vn.LIM_GMINMOD43, 3.0, 9.0) == (4 / 3.0) * 3.0
    assert vn.limiter(vn.LIM_GMINMOD43, 1.0, -1.0) == 0.0
    assert vn.limiter(vn.LIM_NONE, 1.0, -4.0) == -1.5 and vn.limiter(vn.LIM_ZERO, 1.0, 4.0) == 0.0
    c = vn.classes(*np.array([(1, 4), (5, 2), (3, 5), (2, 2), (0, 1), (-1, 1), (1, 8), (8, 1)],
                             float).T)
    assert c["koren aa==ab/4"] == 1 and c["koren aa==2.5ab"] == 1 and c["koren ab==0"] == 1
    assert c["koren ab<0"] == 1 and c["koren aa<ab/4"] == 1 and c["koren aa>2.5ab"] == 1
    assert c["theta 4/3: tie"] == 1 and c["theta 1: tie"] == 1 and c["theta 2: tie"] == 0
    assert c["theta 4/3: (a+b)/2"] == 1 and c["theta 2: (a+b)/2"] == 3


# ------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("ndim", [3, 2])
def test_fixture_tree(ndim):
    """The fixture's tree is variants_tree(4), id for id, and has what the
    tests need of it (oracle/make_variants.py check_tree)."""
    g = fixture(ndim)
    t = variants_tree(4, ndim)
    keys = [k for k in t if k in g and k != "periodic"]
    assert len(keys) >= 20
    for k in keys:
        assert np.array_equal(t[k], g[k]), k
    nbs = g["meta_neighbors"][vn.leaves(g)]
    assert all((nbs[:, f] < 0).any() and (nbs[:, f] == 0).any() for f in range(2 * ndim))
    assert (nbs > 0).any() and int(g["n_boxes"]) == (25 if ndim == 3 else 88)


@pytest.mark.parametrize("ndim", [3, 2])
def test_fixture_values(ndim):
    """Lattice input; every face sees every type; the values the harness
    used are bc_values()."""
    g = fixture(ndim)
    k = g["in_e"][vn.leaves(g)][(slice(None),) + (slice(1, -1),) * ndim] / vn.LATTICE
    off = k[k != np.round(k)] * vn.LATTICE
    planted = {a for a, _ in vn.KOREN_EDGES} | {a + b for a, b in vn.KOREN_EDGES}
    assert set(off.tolist()) == planted and off.size == 3 * 2 * 2 * ndim
    assert k.min() == 0 and np.sort(k[k == np.round(k)])[-1] == 8
    f = g["in_fc_field"]
    assert (f > 0).any() and (f < 0).any() and (f == 0).any()
    for r in range(4):
        want = rotation(r, ndim)
        assert [int(t) for t in g["gc_bc_types"][r]] == [t for t, _ in want]
        assert list(g["gc_bc_vals"][r]) == [v for _, v in want]
    for a in range(3):
        want = assignment(a, ndim)
        assert [int(t) for t in g["bflux_bc_types"][a]] == [t for t, _ in want]
        assert list(g["bflux_bc_vals"][a]) == [v for _, v in want]
    # the Neumann assignment has a non-zero value on high-y (m_af_ghostcell.f90:361)
    assert g["bflux_bc_vals"][1][3] != 0


def _against_fixture(g, key, F, lim):
    """Fluxes and limits within TOL_EXACT of the reference's; they are in
    fact its bits."""
    for d, (a, b) in enumerate(zip(leaf_faces(F[0], g), leaf_faces(g[key], g))):
        e = golden.rel_err(a, b)
        print(key, "dim", d, "rel err", e, "bitwise", np.array_equal(a, b))
        assert e <= TOL_EXACT, (key, d, e)
        assert np.array_equal(a, b), (key, d, e)
        assert np.count_nonzero(b) > b.size // 2
    np.testing.assert_allclose(lim, g[key + "_dt"], rtol=TOL_EXACT)
    assert list(lim) == list(g[key + "_dt"])


@pytest.mark.parametrize("lim", vn.LIMITERS)
def test_oracle_flux_limiter_matches_reference(lim):
    g = fixture(3)
    F, cc, dt = run_flux(capi.oracle_library(), -1, g, g, fixture_inputs(g), limiter=lim)
    _against_fixture(g, "flux_%d" % lim, F, dt)
    census_after_flux(cc, g, "fixture 3-D")


def test_flux_limiters_differ():
    """No two of the seven give the same fluxes on this input."""
    g = fixture(3)
    for nd in (3, 2):
        g = fixture(nd)
        for kind in ("flux", "pflux"):
            for a in vn.LIMITERS:
                for b in range(a + 1, 8):
                    assert not np.array_equal(g["%s_%d" % (kind, a)], g["%s_%d" % (kind, b)])


@pytest.mark.parametrize("lim", vn.LIMITERS)
def test_oracle_prolong_limiter_matches_reference(lim):
    """The species' prolongation limiter, through gc2_prolong_rb."""
    g = fixture(3)
    F, _, dt = run_flux(capi.oracle_library(), -1, g, g, fixture_inputs(g), prolong=lim)
    _against_fixture(g, "pflux_%d" % lim, F, dt)


def gc_filled(lib, dev, topo, bc, rb, corners, v, bc2=None):
    """afh_gc_tree of variable 1 holding v under bc; bc2: then afh_set_bc to
    that boundary, face by face, and a second fill."""
    t = Tree(lib, topo, 1, 0, device=dev)
    t.set_cc_methods(1, bc, rb)
    t.put_cc(1, v)
    t.gc_tree(1, corners)
    if bc2 is not None:
        for nb, (ty, val) in enumerate(bc2):
            t.set_bc(1, nb + 1, ty, val)
        t.gc_tree(1, corners)
    out = t.get_cc(1)
    t.close()
    return out


@pytest.mark.parametrize("meth", [1, 2])
@pytest.mark.parametrize("rot", range(4))
def test_oracle_gc_tree_matches_reference(rot, meth):
    """af_gc_tree with corners under each rotation of the four types: the
    arithmetic is exact by construction, every ghost cell of every box."""
    g = fixture(3)
    a = gc_filled(capi.oracle_library(), -1, g, rotation(rot, 3), meth, True, g["in_e"])
    b = g["gc_%d_%d" % (rot, meth)]
    assert np.array_equal(a, b), np.argwhere(a != b)[:4]
    assert not np.array_equal(a, g["in_e"])


def test_gc_rotations_differ():
    for nd in (3, 2):
        g = fixture(nd)
        keys = ["gc_%d_%d" % (r, m) for r in range(4) for m in (1, 2)]
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                assert not np.array_equal(g[a], g[b]), (a, b)


@pytest.mark.parametrize("asg", range(3))
def test_oracle_two_layer_boundary_matches_reference(asg):
    """bc_to_gc2 with non-zero values, seen through the flux; the Neumann
    assignment carries the c0 of m_af_ghostcell.f90:361 on high-y."""
    g = fixture(3)
    F, cc, dt = run_flux(capi.oracle_library(), -1, g, g, fixture_inputs(g),
                         bc=assignment(asg, 3))
    _against_fixture(g, "bflux_%d" % (asg + 1), F, dt)
    assert not np.array_equal(F[0], g["flux_3"])


# --------------------------------------------- the 2-D fixture and the model
def test_numpy_2d_flux_matches_reference():
    """tests/variants_numpy.py flux_2d (the statement the 2-D library is held
    to on the GPU) against the reference's 2-D build: every flux limiter,
    every prolongation limiter, the three boundary assignments; bitwise."""
    g = fixture(2)
    x = fixture_inputs(g)
    n0 = [(capi.BC_NEUMANN, 0.0)] * 4
    runs = [("flux_%d" % l, dict(lim=l, prolong=vn.LIM_MC, bc=n0)) for l in vn.LIMITERS]
    runs += [("pflux_%d" % l, dict(lim=vn.LIM_KOREN, prolong=l, bc=n0)) for l in vn.LIMITERS]
    runs += [("bflux_%d" % (a + 1), dict(lim=vn.LIM_KOREN, prolong=vn.LIM_MC,
                                         bc=assignment(a, 2))) for a in range(3)]
    for key, kw in runs:
        F, cc, dt = vn.flux_2d(g, x["e"], x["efld"], x["fc_field"], tables_from(g)[0],
                               1 / float(g["gas_number_density"]), **kw)
        for a, b in zip(leaf_faces(F, g), leaf_faces(g[key], g)):
            assert np.array_equal(a, b), key
        assert list(dt) == list(g[key + "_dt"]), key
        if key == "flux_3":
            vn.assert_census(cc[vn.leaves(g)], 2, "fixture 2-D")


@pytest.mark.parametrize("meth", [1, 2])
@pytest.mark.parametrize("rot", range(4))
def test_numpy_2d_boundary_fill_matches_reference(rot, meth):
    """The physical-boundary ghost cells of the 2-D fixture are bc_to_gc's
    (m_af_ghostcell.f90:173-279) of the fixture's own interiors."""
    g = fixture(2)
    a, nc = g["gc_%d_%d" % (rot, meth)], 4
    nbs, bc = g["meta_neighbors"], rotation(rot, 2)
    n = 0
    for b in vn.in_use(g):
        for nb in range(4):
            if nbs[b, nb] >= 0:
                continue
            want = vn.bc_ghost_2d(a[b], nb, bc[nb], g["meta_dr"][b], nc)
            got = (a[b][1:-1, 0 if nb == 0 else nc + 1] if nb < 2 else
                   a[b][0 if nb == 2 else nc + 1, 1:-1])
            assert np.array_equal(got, want), (b, nb)
            n += 1
    assert n > 30


# ------------------------------------------------- af_prolong_limit, regrid
# level-1 boxes per dimension of the regrid tests: some 4000 parent cells, so
# that the rarest class of slope pairs (one in 400) occurs along every dimension
REGRID_N1 = {(3, 4): 4, (3, 6): 3, (2, 4): 16, (2, 6): 11}


def regrid_topos(nc, ndim):
    """A uniform level 1, then every box of it refined."""
    n1 = REGRID_N1[ndim, nc]
    af = AfTree(nc, [2.0 ** -10] * ndim, [n1 * nc] * ndim)
    t0 = af.topology()

    def fn(ids):
        return np.full(len(ids), DO_REF), np.zeros(len(ids), np.uint32)

    assert af.adjust_refinement(fn).n_add == (2 * n1) ** ndim
    return t0, af.topology()


def regrid_prolong(lib, dev, nc, ndim, lim):
    """afh_tree_regrid with AFH_PROLONG_LIMIT and limiter lim of a lattice
    field on a uniform level: (the parent level as it was prolonged from,
    ghost cells filled; the new tree's array; the new topology)."""
    t0, t1 = regrid_topos(nc, ndim)
    t = Tree(lib, t0, 1, 0, device=dev)
    t.set_cc_methods(1, [(capi.BC_NEUMANN, 0.0)] * (2 * ndim), capi.RB_GC_INTERP_LIM, lim)
    t.set_cc_prolong(1, capi.PROLONG_LIMIT, lim)
    rng = np.random.default_rng(100 * nc + ndim)
    v = vn.lattice(rng, t.cc_shape)
    vn.plant_koren_edges(v, ndim, [(0, 0), (1, 0), (2, 0)])
    t.put_cc(1, v)
    t.gc_tree(1)
    before = t.get_cc(1)
    t2 = t.regrid(t1)
    after = t2.get_cc(1)
    t2.close()
    return before, after, t1


def check_prolong_against_numpy(before, after, t1, ndim, lim):
    nc, n_old = int(t1["nc"]), len(before)
    vn.assert_census(before, ndim, "regrid input %d-D nc %d" % (ndim, nc), both=False)
    inner = (slice(1, -1),) * ndim
    for p in range(n_old):
        for c in t1["meta_children"][p]:
            off = [((int(t1["meta_ix"][c - 1][d]) - 1) & 1) * (nc // 2) for d in range(ndim)]
            want = vn.prolong_limit(before[p], off, lim)
            assert np.array_equal(after[c - 1][inner], want), (c, lim)
    assert len(after) == n_old * (1 + 2 ** ndim) and np.array_equal(after[:n_old], before)


@pytest.mark.parametrize("nc", [4, 6])
@pytest.mark.parametrize("lim", vn.LIMITERS)
def test_oracle_regrid_prolong_limit_is_the_numpy_model(lim, nc):
    """af_prolong_limit into new boxes (m_af_prolong.f90:311-420): child =
    f0 -+ f1 -+ f2 -+ f3 with f_d a quarter of the limited slope."""
    before, after, t1 = regrid_prolong(capi.oracle_library(), -1, nc, 3, lim)
    check_prolong_against_numpy(before, after, t1, 3, lim)


def test_numpy_prolong_limit_2d_by_hand():
    """One parent cell by hand, minmod: slopes (1, 3) in x give 1, (2, 2) in
    y give 2 (times 2^50), a quarter of each added and subtracted."""
    cp = np.zeros((4, 4))
    cp[1, 1] = 10
    cp[1, 0], cp[1, 2] = 9, 13
    cp[0, 1], cp[2, 1] = 8, 12
    out = vn.prolong_limit(cp, (0, 0), vn.LIM_MINMOD)
    assert out[0, 0] == 10 - 0.25 - 0.5 and out[0, 1] == 10 + 0.25 - 0.5
    assert out[1, 0] == 10 - 0.25 + 0.5 and out[1, 1] == 10 + 0.25 + 0.5


# ------------------------------------------------------------------ refusals
def phi_solves(lib, dev, bad_type):
    """A Dirichlet / Neumann solve, a refused solve with bad_type on one face
    of the potential (set by afh_set_bc after the multigrid exists), the
    boundary restored, the first solve again: (phi of the two good solves,
    phi after the refused call, the exceptions)."""
    topo = two_box_tree(4)
    t = Tree(lib, topo, N_VAR_CELL, 2, device=dev)
    bc = [(capi.BC_NEUMANN, 0.0)] * 4 + [(capi.BC_DIRICHLET, 0.0), (capi.BC_DIRICHLET, 100.0)]
    for iv in (IV["phi"], IV["rhs"], IV["tmp"]):
        t.set_cc_methods(iv, bc, capi.RB_MG_SIDES)
    mg = Multigrid(t, IV["phi"], IV["rhs"], IV["tmp"], coarse_cycles=0)
    rng = np.random.default_rng(3)
    phi0, rhs = rng.random(t.cc_shape), 1e6 * rng.random(t.cc_shape)

    def solve(fmg):
        t.put_cc(IV["phi"], phi0)
        t.put_cc(IV["rhs"], rhs)
        if fmg:
            mg.fas_fmg(True, have_guess=True)
        else:
            mg.fas_vcycle(True)
        return t.get_cc(IV["phi"])

    good, errs, kept = [solve(False), solve(True)], [], []
    t.set_bc(IV["phi"], 2, bad_type, 5.0)
    for fmg in (False, True):
        with pytest.raises(capi.AfhError) as e:
            solve(fmg)
        errs.append(e)
        kept.append(t.get_cc(IV["phi"]))
    t.set_bc(IV["phi"], 2, capi.BC_NEUMANN, 0.0)
    good += [solve(False), solve(True)]
    t.close()
    return good, kept, errs, phi0


def check_phi_refusal(lib, dev, bad_type):
    good, kept, errs, phi0 = phi_solves(lib, dev, bad_type)
    for e in errs:
        assert code_of(e) == ERR_UNSUPPORTED
        assert "coarse solve: bc type %d" % bad_type in str(e.value)
    # the refused calls changed nothing; the solves around them agree
    assert all(np.array_equal(k, phi0) for k in kept)
    assert np.array_equal(good[0], good[2]) and np.array_equal(good[1], good[3])
    assert not np.array_equal(good[0], phi0)


@pytest.mark.parametrize("bad", [capi.BC_CONTINUOUS, capi.BC_DIRICHLET_COPY])
def test_oracle_refuses_potential_boundary(bad):
    """m_coarse_solver.f90:485-486: the level-1 solve takes Dirichlet and
    Neumann only."""
    check_phi_refusal(capi.oracle_library(), -1, bad)


def flux_refusal(lib, dev, topo, tabs, ions=(), species="e"):
    """AFH_BC_CONTINUOUS on one face of a flux species: every entry point of
    the flux refuses before it changes anything; afterwards the flux is the
    one from before."""
    c = FluxCase(lib, dev, topo, tabs, ions=ions)
    x = lattice_inputs(topo, 11)
    c.put(x)
    F0, _, lim0 = c.flux()
    c.put(x)
    c.tree.set_bc(IV[species], 3, capi.BC_CONTINUOUS, 0.0)
    calls = [lambda: c.fluid.flux_upwind_tree(0),
             lambda: c.fluid.forward_euler(1e-12, 0, [0], [1.0], 1, False)]
    if lib.has("fluid_forward_euler_fold"):
        calls.append(lambda: c.fluid.forward_euler_fold(1e-12, 0, [0], [1.0], 1, False))
    for call in calls:
        with pytest.raises(capi.AfhError) as e:
            call()
        assert code_of(e) == ERR_UNSUPPORTED and "bc type -12" in str(e.value)
        for s in ("e", "pos", "neg"):
            assert np.array_equal(c.tree.get_cc(IV[s]), x[s])
            assert np.array_equal(c.tree.get_cc(IV[s] + 1), np.zeros_like(x[s]))
    # dirichlet_copy is bc_to_gc2's third case: accepted
    c.tree.set_bc(IV[species], 3, capi.BC_DIRICHLET_COPY, 2.0 ** 51)
    F1, _, _ = c.flux()
    q = 0 if species == "e" else 1
    assert not np.array_equal(F1[q], F0[q])
    c.put(x)
    c.tree.set_bc(IV[species], 3, capi.BC_NEUMANN, 0.0)
    F2, _, lim2 = c.flux()
    assert lim2 == lim0 and all(np.array_equal(a, b) for a, b in zip(F0, F2))
    c.close()


@pytest.mark.parametrize("species", ["e", "pos"])
def test_oracle_refuses_continuous_flux_species(species):
    """m_af_ghostcell.f90:317-318: bc_to_gc2 stops on af_bc_continuous."""
    g = fixture(3)
    flux_refusal(capi.oracle_library(), -1, two_box_tree(4), g,
                 ions=IONS if species != "e" else (), species=species)


# ---------------------------------------------------------------- the census
# the inputs of the limiter tests of test_variants_gpu.py: (tree, box size,
# seed); the fixtures' own census is taken by the tests above
FLUX_INPUTS_3D = [("amr", 4, 1), ("amr", 6, 2), ("amr", 16, 3), ("two", 32, 4), ("two", 64, 5)]
FLUX_INPUTS_2D = [("amr", 4, 1), ("amr", 6, 2), ("amr", 16, 3)]


def flux_input(kind, nc, seed, ndim=3):
    topo = variants_tree(nc, ndim) if kind == "amr" else two_box_tree(nc, ndim)
    return topo, lattice_inputs(topo, seed)


@pytest.mark.parametrize("kind,nc,seed", FLUX_INPUTS_3D)
def test_census_of_the_3d_flux_inputs(kind, nc, seed):
    """Every class of pairs at least three times along every dimension, in
    the electrons and in both ions, on what the flux reads (the oracle's
    ghost layer included)."""
    topo, x = flux_input(kind, nc, seed)
    _, cc, _ = run_flux(capi.oracle_library(), -1, topo, fixture(3), x,
                        ions=IONS if nc == 4 else ())
    census_after_flux(cc, topo, "%s %d" % (kind, nc))


@pytest.mark.parametrize("kind,nc,seed", FLUX_INPUTS_2D)
def test_census_of_the_2d_flux_inputs(kind, nc, seed):
    """The same on what the 2-D flux reads, from the numpy statement."""
    topo, x = flux_input(kind, nc, seed, 2)
    g = fixture(2)
    for s in ("e", "pos", "neg"):
        _, cc, _ = vn.flux_2d(topo, x[s], x["efld"], x["fc_field"], tables_from(g)[0],
                              1 / float(g["gas_number_density"]), lim=vn.LIM_KOREN,
                              prolong=vn.LIM_MC, bc=[(capi.BC_NEUMANN, 0.0)] * 4)
        vn.assert_census(cc[vn.leaves(topo)], 2, "2-D %s %d %s" % (kind, nc, s))

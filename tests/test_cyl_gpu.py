"""Cylindrical (af_cyl) coordinates in libafivo_hip_2d.so, on the device.

The reference's replay harnesses are Cartesian only, so the operators are held
to tests/cyl_numpy.py (the reference's formulas in numpy, float64 in the
stated order) -- bitwise wherever the kernel evaluates the same expression --
and the whole time loop to the regression logs the reference committed for
programs/standard_2d/tests/test_cyl.cfg and test_cyl_chem.cfg.

Trees: tests/state2d.py's AMR tree (8^2 boxes, levels 4..7 around a point,
starting on the axis, coarse-fine faces normal to r and to z) and, where a
global-array statement is needed, a 16 x 16 level 1 with one uniform
refinement.
"""
import functools
import re

import numpy as np
import pytest

import cyl_numpy as cn
import golden
import state2d
from afh import capi
from afh.amr import AfTree
from afh.driver import Simulation
from afh.model import Multigrid, Tree, tree_desc

pytestmark = pytest.mark.gpu

PFMG = dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
EPS = np.finfo(np.float64).eps
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -4


@functools.lru_cache(maxsize=None)
def _state():
    return state2d.build_state("test_2d")


def _used(af):
    return [b for b in range(1, af.highest_id + 1) if af.in_use[b]]


def _sim(cyl, af=None, case=None):
    """A Simulation bound to the state2d tree (or `af`), cylindrical or not,
    with the reference's PFMG level-1 solve."""
    c, af0, _, _, _ = _state()
    sim = Simulation(capi.hip_library_2d(), case if case is not None else c, device=0, **PFMG)
    sim.af = af if af is not None else af0
    sim.cylindrical = cyl
    sim._bind(sim._create_tree())
    assert sim.tree.coord == (capi.COORD_CYL if cyl else capi.COORD_XYZ)
    return sim


def _code(exc):
    return int(re.search(r"failed \((-?\d+)\)", str(exc.value)).group(1))


def _rand_fields(af, seed, scale=1.0):
    """Random box images (ghost cells included) on the boxes in use."""
    rng = np.random.default_rng(seed)
    ng = af.nc + 2
    a = np.zeros((af.highest_id, ng, ng))
    for b in _used(af):
        a[b - 1] = rng.standard_normal((ng, ng)) * scale
    return a


# ------------------------------------------------------------------ 1. ABI
def test_set_coord_rules():
    lib = capi.hip_library_2d()
    af = AfTree(8, [1e-3, 1e-3], [8, 8])
    bc = [(capi.BC_NEUMANN, 0.0)] * 2 + [(capi.BC_DIRICHLET, 0.0)] * 2
    t = Tree(lib, af.topology(), 4, 1, device=0)
    assert t.coord == capi.COORD_XYZ
    with pytest.raises(capi.AfhError) as e:
        t.set_coord(7)
    assert _code(e) == ERR_ARG
    t.set_coord(capi.COORD_CYL)
    t.set_coord(capi.COORD_XYZ)
    t.set_coord(capi.COORD_CYL)
    assert t.coord == capi.COORD_CYL
    t.set_cc_methods(1, bc, capi.RB_MG_SIDES)
    t.set_cc_prolong(1, capi.PROLONG_LINEAR)
    # the direct level-1 solve does not apply
    with pytest.raises(capi.AfhError) as e:
        Multigrid(t, 1, 2, 3, coarse_cycles=0, coarse_mode=capi.COARSE_DIRECT)
    assert _code(e) == ERR_UNSUPPORTED and "cylindrical" in str(e.value)
    t.set_coord(capi.COORD_CYL)  # a failed create fixes nothing
    # a regridded tree inherits the type
    af.refine_up_to_lvl(2)
    t2 = t.regrid(af.topology())
    assert t2.coord == capi.COORD_CYL
    mg = Multigrid(t2, 1, 2, 3, **PFMG)
    with pytest.raises(capi.AfhError) as e:
        t2.set_coord(capi.COORD_XYZ)
    assert _code(e) == ERR_STATE
    assert t2.coord == capi.COORD_CYL
    mg.close()
    t2.close()
    t.close()
    # r_base[0] < 0
    afn = AfTree(8, [1e-3, 1e-3], [8, 8], r_min=[-1e-3, 0.0])
    tn = Tree(lib, afn.topology(), 4, 1, device=0)
    with pytest.raises(capi.AfhError) as e:
        tn.set_coord(capi.COORD_CYL)
    assert _code(e) == ERR_ARG
    tn.set_coord(capi.COORD_XYZ)
    tn.close()
    # periodic in r
    import ctypes as C
    d, keep = tree_desc(af.topology(), 4, 1)
    d.periodic[0] = 1
    h = C.c_void_p()
    lib.call("tree_create", C.byref(d), 0, C.byref(h))
    with pytest.raises(capi.AfhError) as e:
        lib.call("tree_set_coord", h, capi.COORD_CYL)
    assert _code(e) == ERR_ARG
    lib.call("tree_destroy", h)


# ------------------------------------------------------------ 2. operators
def test_restrict_tree_and_weighted_sum_bitwise():
    c, af, _, _, _ = _state()
    sim = _sim(True)
    iv = sim.i_rhs
    a = np.abs(_rand_fields(af, 11)) + 0.5
    sim.tree.put_cc(iv, a)
    # af_tree_sum_cc, powers 1 and 2, in the reference's loop order
    for power in (1, 2):
        boxes = [(a[b - 1], af.r_min[b][0], af.dr[b]) for l in range(1, af.highest_lvl + 1)
                 for b in af.lvls[l]["leaves"]]
        assert sim.tree.sum_cc(iv, power) == cn.tree_sum(boxes, power)
    sim.tree.restrict_tree(iv)
    ref = a.copy()
    for l in range(af.highest_lvl - 1, 0, -1):
        for p in af.lvls[l]["parents"]:
            for ch in af.children[p]:
                cn.restrict(ref[ch - 1], ref[p - 1], af.ix[ch], af.r_min[p][0], af.dr[p][0])
    got = sim.tree.get_cc(iv)
    n_par = sum(len(af.lvls[l]["parents"]) for l in range(1, af.highest_lvl))
    assert n_par > 20
    assert np.array_equal(got, ref)
    # ... and it is not the Cartesian mean
    plain = a.copy()
    p = af.lvls[af.highest_lvl - 1]["parents"][0]
    for ch in af.children[p]:
        cn.restrict(plain[ch - 1], plain[p - 1], af.ix[ch], 0.0, 1.0, geometry=False)
    assert not np.array_equal(plain[p - 1], got[p - 1])
    sim.tree.close()


def _vcycle_fields(cyl, pair, monkeypatch, n=1, seed=5):
    """phi, rhs, tmp after n V-cycles from the same random phi and rhs."""
    c, af, _, _, _ = _state()
    monkeypatch.setenv("AFH_PAIR2D", "1" if pair else "0")
    sim = _sim(cyl)
    monkeypatch.delenv("AFH_PAIR2D")
    inv_h2 = 1 / af.dr[af.lvls[af.highest_lvl]["ids"][0]][0] ** 2
    sim.tree.put_cc(sim.i_phi, _rand_fields(af, seed))
    sim.tree.put_cc(sim.i_rhs, _rand_fields(af, seed + 1, inv_h2))
    sim.tree.gc_tree(sim.i_phi)
    for _ in range(n):
        sim.mg.fas_vcycle(True)
    out = [sim.tree.get_cc(iv) for iv in (sim.i_phi, sim.i_rhs, sim.i_tmp)]
    sim.tree.close()
    return out


def test_fused_pair_equals_split_sweeps(monkeypatch):
    """k2_pair_box<CYL = true> against k2_gsrb<StCyl> + the level fills, through whole
    V-cycles on the AMR tree (same-level neighbours across r- and z-faces,
    physical and refinement boundaries): bitwise."""
    _, af, _, _, _ = _state()
    split = _vcycle_fields(True, False, monkeypatch, n=2)
    fused = _vcycle_fields(True, True, monkeypatch, n=2)
    ix = np.asarray(_used(af)) - 1
    for a, b in zip(split, fused):
        assert np.array_equal(a[ix][:, 1:-1, 1:-1], b[ix][:, 1:-1, 1:-1])
    # and the cylindrical operator is in use
    cart = _vcycle_fields(False, True, monkeypatch, n=2)
    assert not np.array_equal(cart[0][ix], fused[0][ix])


def test_residual_bitwise(monkeypatch):
    """tmp after a V-cycle with set_residual is rhs - L phi of the phi and rhs
    the device holds, on every box of every level: bitwise."""
    _, af, _, _, _ = _state()
    phi, rhs, tmp = _vcycle_fields(True, True, monkeypatch)
    n = 0
    for b in _used(af):
        cf = cn.lpl_coef(af.dr[b])
        ref = cn.residual(phi[b - 1], rhs[b - 1], cf, af.r_min[b][0], af.dr[b][0])
        assert np.array_equal(tmp[b - 1][1:-1, 1:-1], ref), b
        n += 1
    assert n > 100


def _uniform2(nc=8):
    """2 x 2 level-1 boxes of nc^2 with one uniform refinement."""
    c, _, _, _, _ = _state()
    L = c.ra("domain_len")
    af = AfTree(nc, c.ra("domain_origin") + L, [2 * nc, 2 * nc], r_min=c.ra("domain_origin"))
    af.refine_up_to_lvl(2)
    return af


def _to_global(af, lvl, a, ghosts=False):
    """Level lvl of box array a as one (ny, nx) image (interiors)."""
    nc = af.nc
    n = 2 * nc * 2 ** (lvl - 1)
    g = np.zeros((n, n))
    for b in af.lvls[lvl]["ids"]:
        i0, j0 = (af.ix[b][0] - 1) * nc, (af.ix[b][1] - 1) * nc
        g[j0:j0 + nc, i0:i0 + nc] = a[b - 1][1:-1, 1:-1]
    return g


def _row_r_mins(af, lvl):
    row = sorted((af.ix[b][0], af.r_min[b][0]) for b in af.lvls[lvl]["ids"] if af.ix[b][1] == 1)
    return [r for _, r in row]


def _pad(g):
    p = np.zeros((g.shape[0] + 2, g.shape[1] + 2))
    p[1:-1, 1:-1] = g
    return p


def test_down_leg_coarse_rhs(monkeypatch):
    """One V-cycle's down leg on the uniformly refined tree, split sweeps:
    four half sweeps with fills, the residual, its restriction with geometry,
    phi's without, and rhs = L phi + tmp on level 1 -- against numpy on global
    arrays with the boxes' own radii."""
    _down_leg_coarse_rhs(monkeypatch, 8)


@pytest.mark.parametrize("nc", [6, 12])
def test_down_leg_coarse_rhs_box_size(nc, monkeypatch):
    """The same at box sizes without kernels of their own (k2_gsrb<StCyl>,
    k2_residual<StCyl>, k2_restrict<StCyl> and k2_parent_rhs<StCyl> decode by division;
    the coefficient table of 4 nc doubles)."""
    _down_leg_coarse_rhs(monkeypatch, nc)


def _down_leg_coarse_rhs(monkeypatch, nc):
    af = _uniform2(nc)
    monkeypatch.setenv("AFH_PAIR2D", "0")
    sim = _sim(True, af=af)
    monkeypatch.delenv("AFH_PAIR2D")
    V = sim.voltage
    bc = [("n", 0.0), ("n", 0.0), ("d", 0.0), ("d", V)]
    dr2, dr1 = af.dr[af.lvls[2]["ids"][0]], af.dr[af.lvls[1]["ids"][0]]
    phi0 = _rand_fields(af, 21, abs(V) if V else 1.0)
    rhs0 = _rand_fields(af, 22, (abs(V) if V else 1.0) / dr2[0] ** 2)
    sim.tree.put_cc(sim.i_phi, phi0)
    sim.tree.put_cc(sim.i_rhs, rhs0)
    sim.tree.gc_tree(sim.i_phi)
    sim.mg.fas_vcycle(False)
    got = _to_global(af, 1, sim.tree.get_cc(sim.i_rhs))
    sim.tree.close()
    # numpy
    c2, c1 = cn.lpl_coef(dr2), cn.lpl_coef(dr1)
    t2 = cn.level_radius_tables(c2, _row_r_mins(af, 2), dr2[0], nc)
    t1 = cn.level_radius_tables(c1, _row_r_mins(af, 1), dr1[0], nc)
    g = cn.fill_bc(_pad(_to_global(af, 2, phi0)), bc, dr2)
    r = _pad(_to_global(af, 2, rhs0))
    for s in range(1, 5):
        cn.level_gsrb_half(g, r, c2, t2, s)
        cn.fill_bc(g, bc, dr2)
    res = r[1:-1, 1:-1] - cn.level_apply(g, c2, t2)
    w = [cn.child_weights(r0, dr1[0], np.arange(1, nc + 1)) for r0 in _row_r_mins(af, 1)]
    w1, w2 = np.concatenate([x[0] for x in w]), np.concatenate([x[1] for x in w])
    tmp_c = 0.25 * (w1 * (res[0::2, 0::2] + res[1::2, 0::2]) + w2 * (res[0::2, 1::2] + res[1::2, 1::2]))
    f = g[1:-1, 1:-1]
    phi_c = 0.25 * (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2])
    pc = cn.fill_bc(_pad(phi_c), bc, dr1)
    ref = cn.level_apply(pc, c1, t1) + tmp_c
    rel = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("down leg coarse rhs: max rel %.3g, %d of %d not bitwise"
          % (rel, np.count_nonzero(got != ref), ref.size))
    assert np.array_equal(got, ref)


# ------------------------------------------------------- 3. consistent fluxes
def test_consistent_fluxes_bitwise():
    c, af, cc, fc, _ = _state()
    sim = _sim(True)
    for iv, a in cc.items():
        sim.tree.put_cc(iv, a)
    for iv, a in fc.items():
        sim.tree.put_fc(iv, a)
    sim.fluid.flux_upwind_tree(0)
    F = sim.tree.get_fc(sim.f_flux)
    nc, h = af.nc, af.nc // 2
    adj = {1: (1, 3), 2: (2, 4), 3: (1, 2), 4: (3, 4)}   # af_child_adj_nb
    cdix = {1: (0, 0), 2: (1, 0), 3: (0, 1), 4: (1, 1)}  # af_child_dix
    n_r = n_z = n_weighted = 0
    for l in range(1, af.highest_lvl):
        for p in af.lvls[l]["parents"]:
            for nb in (1, 2, 3, 4):
                q = af.neighbors[p][nb - 1]
                if q <= 0 or af.children[q][0] > 0:
                    continue
                d, low = (nb - 1) // 2, (nb - 1) % 2 == 0
                i, i_nb = (1, nc + 1) if low else (nc + 1, 1)
                for ich in adj[nb]:
                    ch = af.children[p][ich - 1]
                    n = np.arange(1, h + 1)
                    if d == 0:
                        fine = F[ch - 1, 0, :, i - 1]
                        ref = 0.5 * (fine[2 * n - 2] + fine[2 * n - 1])
                        got = F[q - 1, 0, h * cdix[ich][1] + n - 1, i_nb - 1]
                        n_r += 1
                    else:
                        fine = F[ch - 1, 1, i - 1, :]
                        ic = h * cdix[ich][0] + n
                        ref = cn.consistent_zface(fine[2 * n - 2], fine[2 * n - 1],
                                                  af.r_min[q][0], af.dr[q][0], ic)
                        got = F[q - 1, 1, i_nb - 1, ic - 1]
                        n_weighted += int(np.count_nonzero(
                            ref != 0.5 * (fine[2 * n - 2] + fine[2 * n - 1])))
                        n_z += 1
                    assert np.array_equal(got, ref), (p, nb, ich)
    assert n_r > 0 and n_z > 0 and n_weighted > 0
    sim.tree.close()


# ------------------------------------------------------------------ 4. update
def test_update_is_cartesian_plus_the_radial_factors():
    c, af, cc, fc, dt = _state()
    rng = np.random.default_rng(31)
    out, F = {}, None
    for cyl in (False, True):
        sim = _sim(cyl)
        for iv, a in cc.items():
            sim.tree.put_cc(iv, a)
        for iv, a in fc.items():
            sim.tree.put_fc(iv, a)
        if F is None:
            sim.fluid.flux_upwind_tree(0)
            F = sim.tree.get_fc(sim.f_flux)
            F = F * (1 + 0.1 * rng.standard_normal(F.shape))
        sim.tree.put_fc(sim.f_flux, F)
        sim.fluid.flux_update_densities(dt, 0, [0], [1.0], 1, False)
        out[cyl] = {iv: sim.tree.get_cc(iv + 1) for iv in sim.densities}
        i_e = sim.i_electron
        sim.tree.close()
    nc = af.nc
    n = 0
    for b in af.leaves():
        f1, f2 = cn.flux_factors(af.r_min[b][0], af.dr[b][0], nc)
        dtx = dt / af.dr[b][0]
        Fr = F[b - 1, 0, :nc, :]
        a, bq = Fr[:, :nc], Fr[:, 1:]
        want = out[False][i_e][b - 1][1:-1, 1:-1] + dtx * ((f1 - 1) * a - (f2 - 1) * bq)
        got = out[True][i_e][b - 1][1:-1, 1:-1]
        bound = 8 * EPS * (np.abs(got) + dtx * (np.abs(a) + np.abs(bq)))
        assert np.all(np.abs(got - want) <= bound), (b, np.max(np.abs(got - want) / bound))
        n += int(np.count_nonzero(got != out[False][i_e][b - 1][1:-1, 1:-1]))
        # the other species have no flux: identical
        for iv in out[True]:
            if iv != i_e:
                assert np.array_equal(out[True][iv][b - 1][1:-1, 1:-1],
                                      out[False][iv][b - 1][1:-1, 1:-1])
    assert n > 0


# ------------------------------------------------------------- 5. conservation
def test_forward_euler_conserves_the_weighted_charge():
    c, af, cc, fc, dt = _state()
    L, o = c.ra("domain_len"), c.ra("domain_origin")
    # four cells of the coarsest leaves: more than the flux stencil reaches
    m = 4 * max(af.dr[b].max() for b in af.leaves())
    cc = {iv: a.copy() for iv, a in cc.items()}
    for b in _used(af):
        xx, yy = state2d._cells(af, b)
        inside = (xx < o[0] + L[0] - m) & (yy > o[1] + m) & (yy < o[1] + L[1] - m)
        for iv in c.ia("all_densities"):
            for s in (0, 1):
                cc[iv + s][b - 1] = np.where(inside, cc[iv + s][b - 1], 0.0)
    viol = {}
    for cyl in (True, False):
        sim = _sim(cyl)
        for iv, a in cc.items():
            sim.tree.put_cc(iv, a)
        for iv, a in fc.items():
            sim.tree.put_fc(iv, a)
        sim.fluid.forward_euler(dt, 0, [0], [1.0], 1, False)
        after = {iv: sim.tree.get_cc(iv + 1) for iv in sim.densities}
        charge = {sim.species_itree[n]: sim.species_charge[n] for n in sim.plasma}
        leaves = [b for l in range(1, af.highest_lvl + 1) for b in af.lvls[l]["leaves"]]

        def wsum(a):
            return cn.tree_sum([(a[b - 1], af.r_min[b][0], af.dr[b]) for b in leaves])

        q0 = sum(charge[iv] * wsum(cc[iv]) for iv in charge if charge[iv])
        q1 = sum(charge[iv] * wsum(after[iv]) for iv in charge if charge[iv])
        scale = sum(abs(charge[iv]) * wsum(cc[iv]) for iv in charge)
        if cyl:  # the library's own sums are the same numbers
            for iv in charge:
                assert sim.tree.sum_cc(iv + 1, 1) == wsum(after[iv])
        viol[cyl] = abs(q1 - q0) / scale
        moved = max(np.max(np.abs(after[iv] - cc[iv])) for iv in after)
        assert moved > 0
        sim.tree.close()
    print("charge drift / scale: cylindrical %.3g, Cartesian step %.3g" % (viol[True], viol[False]))
    assert viol[True] <= 1e-13
    assert viol[False] > 1e-13


# --------------------------------------------------------------- 6. multigrid
def test_multigrid_converges_to_the_discrete_solution():
    af = _uniform2()
    sim = _sim(True, af=af)
    V = sim.voltage if sim.voltage else 1.0
    sim.tree.set_bc(sim.i_phi, 4, capi.BC_DIRICHLET, V)
    bc = [("n", 0.0), ("n", 0.0), ("d", 0.0), ("d", V)]
    dr2 = af.dr[af.lvls[2]["ids"][0]]
    ng = af.nc + 2
    rhs = np.zeros((af.highest_id, ng, ng))
    for b in _used(af):
        xx, yy = state2d._cells(af, b)
        Lx = af.domain[0] - af.r_base[0]
        rhs[b - 1] = (V / Lx ** 2) * (3 * np.cos(2 * xx / Lx) + np.sin(5 * yy / Lx) + 40 * xx * yy / Lx ** 2)
    sim.tree.put_cc(sim.i_rhs, rhs)
    sim.tree.put_cc(sim.i_phi, np.zeros_like(rhs))
    sim.mg.fas_fmg(True, False)
    for _ in range(14):
        sim.mg.fas_vcycle(True)
    got = _to_global(af, 2, sim.tree.get_cc(sim.i_phi))
    sim.tree.close()
    c2 = cn.lpl_coef(dr2)
    t2 = cn.level_radius_tables(c2, _row_r_mins(af, 2), dr2[0], af.nc)
    n = got.shape[0]
    A, G = cn.level_matrix(c2, t2, n, n, bc)
    b = _to_global(af, 2, rhs).reshape(-1) - G[:, 3] * 2 * V
    ref = np.linalg.solve(A, b).reshape(n, n)
    rel = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("FMG + 14 V-cycles vs dense solve: max rel %.3g" % rel)
    assert rel <= 1e-10


def _reduction_factor(cyl):
    c, af, _, _, _ = _state()
    sim = _sim(cyl)
    ng = af.nc + 2
    rhs = np.zeros((af.highest_id, ng, ng))
    L = c.ra("domain_len")
    for b in _used(af):
        xx, yy = state2d._cells(af, b)
        rhs[b - 1] = 1e6 * np.exp(-((xx - 0.5 * L[0]) ** 2 + (yy - 0.3 * L[1]) ** 2) / (0.05 * L[0]) ** 2)
    sim.tree.put_cc(sim.i_rhs, rhs)
    sim.tree.put_cc(sim.i_phi, np.zeros_like(rhs))
    sim.tree.gc_tree(sim.i_phi)
    res = [sim.mg.fas_vcycle_maxres() for _ in range(6)]
    sim.tree.close()
    return (res[5] / res[1]) ** 0.25, res


def test_vcycle_reduction_close_to_cartesian():
    """The residual reduction per V-cycle (cycles 2 to 6, geometric mean) on
    the AMR tree: the same smoother with mildly variable coefficients, at most
    2 x the Cartesian operator's on the same tree."""
    f_cyl, r_cyl = _reduction_factor(True)
    f_xyz, r_xyz = _reduction_factor(False)
    print("residual factor per V-cycle: cylindrical %.4f, Cartesian %.4f" % (f_cyl, f_xyz))
    print("  cyl", ["%.3g" % r for r in r_cyl], "xyz", ["%.3g" % r for r in r_xyz])
    assert f_cyl < 1.0 and f_cyl <= 2 * f_xyz


# --------------------------------------------------------------- 7. time loop
# measured max relative deviation from the reference's log: 4.67e-8 and
# 4.39e-8; the bound is 10 x that, not below the log's print precision 1e-7, never above
# compare_logs' own 1e-5
RTOL_CYL = {"rtest_test_cyl": 4.7e-7, "rtest_test_cyl_chem": 4.4e-7}


@pytest.mark.parametrize("name", sorted(RTOL_CYL))
def test_cyl_rtest_hip(name):
    """test_cyl.cfg / test_cyl_chem.cfg: every row of the reference's
    committed regression log within compare_logs' criterion (rtol 1e-5, atol
    1e-8) and within RTOL_CYL; a second run is bitwise the first."""
    d = golden.load(name)
    ref = d["rtest_log"]
    logs = []
    for _ in range(2):
        sim = Simulation(capi.hip_library_2d(), d, device=0, **PFMG)
        assert sim.ndim == 2 and sim.cylindrical
        logs.append(sim.run())
        assert sim.tree.coord == capi.COORD_CYL
        sim.tree.close()
    log = logs[0]
    assert log.shape == ref.shape
    rel = np.abs(log - ref) / np.maximum(np.abs(ref), 1e-300)
    print("%s: max rel per row" % name, rel[:, 2:].max(axis=1), "max", rel[:, 2:].max())
    assert np.array_equal(log[:, 0], ref[:, 0])
    assert np.allclose(log[:, 1], ref[:, 1], rtol=1e-12, atol=0)
    assert np.allclose(log, ref, rtol=1e-5, atol=1e-8)
    bad = ~np.isclose(log, ref, rtol=RTOL_CYL[name], atol=1e-8)
    assert not bad.any(), (np.argwhere(bad)[:5], rel.max())
    assert np.array_equal(logs[1], logs[0])

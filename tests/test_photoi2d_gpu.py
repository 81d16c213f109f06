"""Photoionization in libafivo_hip_2d.so, on the device: the Zheleznyak source
(k2_photoi_src) against tests/photoi_numpy.py, photoi_helmh_compute's mode
loop against the same loop composed from the public calls, its sum
(k2_photoi_sum) against the host statement, three multigrids interleaved on
one tree, the cylindrical Helmholtz operator against a dense solve, the
photoionization term of the species step, and the three regression cases of
programs/standard_2d against the logs the reference committed.

Trees: tests/state2d.py's AMR tree (8^2 boxes, levels 4..7, coarse-fine faces
normal to both axes, starting on the axis) and, for the dense check, a 16 x 16
level 1 with one uniform refinement.
"""
import functools
import re

import numpy as np
import pytest

import cyl_numpy as cn
import golden
import photoi_numpy as pn
import state2d
from afh import capi
from afh.amr import AfTree
from afh.driver import Simulation
from afh.model import photoi_helmh_compute

pytestmark = pytest.mark.gpu

PFMG = dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
CASE = "rtest_test_2d_photoi"
MAX_FMG = 10
# the stopping rule's second value: small enough that a mode needs more than
# one FMG cycle on this tree and source (n_fmg is asserted on the run)
TIGHT_REL_RES = 1e-6


@functools.lru_cache(maxsize=None)
def _af():
    return state2d.build_state("test_2d")[1]


def _used(af):
    return [b for b in range(1, af.highest_id + 1) if af.in_use[b]]


def _sim(cyl, af=None, photoi=True):
    """A Simulation of the test_2d_photoi deck bound to the state2d tree (or
    `af`), cylindrical or not, with the reference's PFMG level-1 solve."""
    sim = Simulation(capi.hip_library_2d(), golden.load(CASE), device=0, **PFMG)
    sim.af = af if af is not None else _af()
    sim.cylindrical = cyl
    sim.photoi = photoi
    sim._bind(sim._create_tree())
    assert sim.tree.coord == (capi.COORD_CYL if cyl else capi.COORD_XYZ)
    return sim


def _leaf_mask(af):
    """(boxes, ng, ng) booleans: whole leaf images, and leaf interiors."""
    ng = af.nc + 2
    whole = np.zeros((af.highest_id, ng, ng), bool)
    for b in af.leaves():
        whole[b - 1] = True
    inner = np.zeros_like(whole)
    inner[:, 1:-1, 1:-1] = whole[:, 1:-1, 1:-1]
    return whole, inner


def _source_field(af, seed=3):
    """A non-negative source: a blob around the refined region with noise."""
    rng = np.random.default_rng(seed)
    ng = af.nc + 2
    a = np.zeros((af.highest_id, ng, ng))
    L = af.domain[0] - af.r_base[0]
    for b in _used(af):
        xx, yy = state2d._cells(af, b)
        g = np.exp(-((xx - 0.5 * L) ** 2 + (yy - 0.3 * L) ** 2) / (0.05 * L) ** 2)
        a[b - 1] = 1e25 * g * (1 + 0.3 * rng.random((ng, ng))) + 1e18 * rng.random((ng, ng))
    return a


# ------------------------------------------------------------------ 1. source
@pytest.mark.parametrize("cyl", [False, True])
def test_source_bitwise(cyl):
    _source_bitwise(cyl, _af())


@pytest.mark.parametrize("nc", [6, 12])
@pytest.mark.parametrize("cyl", [False, True])
def test_source_bitwise_box_size(cyl, nc):
    """Box sizes without kernels of their own: 2 x 2 level-1 boxes of nc^2,
    one of them refined."""
    from afh.amr import DO_REF, KEEP_REF
    from afh.driver import Case
    c = Case(golden.load(CASE))
    L, o = c.ra("domain_len"), c.ra("domain_origin")
    af = AfTree(nc, o + L, [2 * nc, 2 * nc], r_min=o)

    def fn(ids):
        f = [DO_REF if af.lvl[b] == 1 and tuple(af.ix[b][:2]) == (1, 1) else KEEP_REF
             for b in ids]
        return np.array(f), np.zeros(len(ids), np.uint32)
    af.adjust_refinement(fn)
    assert af.highest_lvl == 2 and len(af.leaves()) == 7
    _source_bitwise(cyl, af)


def _source_bitwise(cyl, af):
    sim = _sim(cyl, af)
    rng = np.random.default_rng(17)
    ng = af.nc + 2
    shape = (af.highest_id, ng, ng)
    td = sim.td
    table = np.ascontiguousarray(td["rows_cols"].T)
    n_pts = table.shape[1]
    x_max = td["x_min"] + (n_pts - 1) / td["inv_fac"]
    # Td from 0 (below x_min where x_min > 0) to 1.3 x the last point
    Td = 1.3 * x_max * rng.random(shape) ** 3
    Td[rng.random(shape) < 0.05] = 0.0
    fld = Td * sim.N / 1e21
    ne = 1e19 * rng.random(shape)
    ne[rng.random(shape) < 0.1] = 0.0
    got_Td = fld * 1e21 / sim.N
    frac = (got_Td - td["x_min"]) * td["inv_fac"]
    assert (frac <= 0).any() and (frac >= n_pts - 1).any()
    assert ((frac > 0) & (frac < n_pts - 1)).sum() > frac.size // 2
    sentinel = rng.standard_normal(shape)
    sim.tree.put_cc(sim.i_efld, fld)
    sim.tree.put_cc(sim.i_electron, ne)
    _, inner = _leaf_mask(af)
    for coeff in (sim.photoi_coeff, -sim.photoi_coeff):
        sim.tree.put_cc(sim.i_rhs, sentinel)
        sim.fluid.photoi_set_src(sim.i_rhs, coeff, alpha_col=3)
        got = sim.tree.get_cc(sim.i_rhs)
        ref = pn.source(fld, ne, sim.N, td["x_min"], td["inv_fac"], table, 3, coeff)
        assert np.array_equal(got[inner], ref[inner])
        # ghost cells and non-leaf boxes keep what they held
        assert np.array_equal(got[~inner], sentinel[~inner])
        if coeff > 0:
            assert np.count_nonzero(ref[inner]) > inner.sum() // 2
        else:
            assert not got[inner].any()
    sim.tree.close()


# ------------------------------------------------- 2. the mode loop, the sum
def _host_sum(af, phis, coeffs):
    """af_tree_clear_cc, then per mode v = v - c * phi over whole leaf images."""
    whole, _ = _leaf_mask(af)
    out = np.zeros_like(phis[0])
    for c, p in zip(coeffs, phis):
        out[whole] = out[whole] - c * p[whole]
    return out


def _mode_vars(sim):
    return [(m.i_phi, m.i_rhs, m.i_tmp) for m in sim.helm]


def _helm_library(sim, src, rel):
    sim.tree.put_cc(sim.i_rhs, src)
    n = photoi_helmh_compute(sim.helm, sim.helm_coeffs, sim.i_photo, rel, MAX_FMG)
    return (list(n), [sim.tree.get_cc(iv) for iv in sim.helm_iv],
            sim.tree.get_cc(sim.i_photo))


def _helm_python(sim, src, rel):
    """photoi_helmh_compute composed from the public calls."""
    t = sim.tree
    t.put_cc(sim.i_rhs, src)
    last = sim.helm[-1].i_rhs
    assert last == sim.i_rhs
    for m in sim.helm[:-1]:
        if m.i_rhs != last:
            t.copy_cc(last, m.i_rhs)
    max_rhs = max(t.maxabs_cc(last), np.sqrt(np.finfo(np.float64).eps))
    n_fmg = []
    for m in sim.helm:
        for i in range(1, MAX_FMG + 1):
            m.fas_fmg(True, True)
            if t.maxabs_cc(m.i_tmp) / max_rhs < rel:
                break
        n_fmg.append(min(i, MAX_FMG))
    phis = [t.get_cc(iv) for iv in sim.helm_iv]
    return n_fmg, phis, _host_sum(sim.af, phis, sim.helm_coeffs)


@pytest.mark.parametrize("rel", [1e-2, TIGHT_REL_RES])
@pytest.mark.parametrize("own", [True, False])
@pytest.mark.parametrize("cyl", [False, True])
def test_mode_loop_and_sum_bitwise(cyl, own, rel, monkeypatch):
    """afh_photoi_helmh_compute == the loop of fas_fmg(1, 1), maxabs_cc(i_tmp)
    and the stopping rule, bitwise in every phi_n and in i_photo, equal in
    n_fmg; i_photo is the host statement applied to the phi_n read back,
    non-leaf boxes exactly zero. own: modes 1..n-1 with an rhs and tmp of
    their own (the driver's default) or all on the shared pair."""
    af = _af()
    monkeypatch.setenv("AFH_HELMH_CONC", "1" if own else "0")
    src = _source_field(af)
    runs = []
    for fn in (_helm_library, _helm_python):
        sim = _sim(cyl)
        v = _mode_vars(sim)
        assert (len({x[1] for x in v}) == 3) == own and (len({x[2] for x in v}) == 3) == own
        # 1 bar air: the Bourdon-3 lambdas scaled by the O2 partial pressure
        assert np.allclose(sorted(sim.helm_lambdas), sorted(l * 0.2 for l in
                                                            (4.147e3, 1.095e4, 6.675e4)), rtol=0.05)
        sim.tree.put_cc(sim.i_photo, np.full_like(src, 7.0))  # the clear is the call's
        runs.append(fn(sim, src, rel))
        sim.tree.close()
    (n_a, phi_a, photo_a), (n_b, phi_b, photo_b) = runs
    print("cyl %s own %s rel %g: n_fmg" % (cyl, own, rel), n_a)
    assert n_a == n_b
    for a, b in zip(phi_a, phi_b):
        assert np.array_equal(a, b)
    # the sum: signed zeros included
    host = _host_sum(af, phi_a, sim.helm_coeffs)
    assert np.array_equal(photo_a, host)
    assert np.array_equal(np.signbit(photo_a), np.signbit(host))
    assert np.array_equal(photo_a, photo_b)
    whole, _ = _leaf_mask(af)
    assert not photo_a[~whole].any() and not np.signbit(photo_a[~whole]).any()
    assert np.count_nonzero(photo_a[whole]) > whole.sum() // 2
    if rel == TIGHT_REL_RES:
        assert max(n_a) > 1, n_a
    else:
        assert all(1 <= n <= MAX_FMG for n in n_a)


@pytest.mark.parametrize("cyl", [False, True])
def test_zero_source(cyl):
    af = _af()
    sim = _sim(cyl)
    zero = np.zeros((af.highest_id, af.nc + 2, af.nc + 2))
    sim.tree.put_cc(sim.i_photo, zero + 3.0)
    n, phis, photo = _helm_library(sim, zero, 1e-2)
    sim.tree.close()
    assert n == [1, 1, 1]
    assert not photo.any()
    for p in phis:
        assert not p.any()


def _code(exc):
    return int(re.search(r"failed \((-?\d+)\)", str(exc.value)).group(1))


def test_argument_checks():
    """The checks of the 3-D entry points; variable gas density stays
    unsupported in 2-D."""
    ERR_ARG, ERR_UNSUPPORTED = -1, -2
    sim = _sim(False)
    n_cols = sim.td["rows_cols"].shape[1]
    for i_rhs, col in ((0, 3), (sim.n_var_tree + 1, 3), (sim.i_rhs, 0), (sim.i_rhs, n_cols + 1)):
        with pytest.raises(capi.AfhError) as e:
            sim.fluid.photoi_set_src(i_rhs, 1.0, alpha_col=col)
        assert _code(e) == ERR_ARG
    for i_photo, max_fmg in ((0, 10), (sim.n_var_tree + 1, 10), (sim.i_photo, 0)):
        with pytest.raises(capi.AfhError) as e:
            photoi_helmh_compute(sim.helm, sim.helm_coeffs, i_photo, 1e-2, max_fmg)
        assert _code(e) == ERR_ARG
    other = _sim(False)
    with pytest.raises(capi.AfhError) as e:  # modes of two trees
        photoi_helmh_compute([sim.helm[0], other.helm[1]], sim.helm_coeffs[:2], sim.i_photo)
    assert _code(e) == ERR_ARG
    other.tree.close()
    # afh_fluid_create
    good = sim.photo_species
    for bad in (0, len(sim.plasma) + 1):
        sim.photo_species = bad
        with pytest.raises(capi.AfhError) as e:
            sim._bind(sim.tree)
        assert _code(e) == ERR_ARG
    sim.photo_species = good
    sim.i_gas_dens, sim.gas_fractions = sim.i_rhs, [0.8, 0.2]
    with pytest.raises(capi.AfhError) as e:
        sim._bind(sim.tree)
    assert _code(e) == ERR_UNSUPPORTED
    sim.i_gas_dens = 0
    sim._bind(sim.tree)
    sim.tree.close()


# ------------------------------------------- 3. three multigrids on one tree
def _interleaved(cyl, src, only=None):
    """FMG of each mode, then a V-cycle of each, twice -- all three modes in
    turn, or mode `only` alone with the same calls."""
    sim = _sim(cyl)
    for m in sim.helm:
        sim.tree.put_cc(m.i_rhs, src)
    modes = sim.helm if only is None else [sim.helm[only]]
    for _ in range(2):
        for m in modes:
            m.fas_fmg(True, True)
        for m in modes:
            m.fas_vcycle(True)
    out = [(sim.tree.get_cc(m.i_phi), sim.tree.get_cc(m.i_tmp)) for m in modes]
    sim.tree.close()
    return out


@pytest.mark.parametrize("cyl", [False, True])
def test_three_multigrids_interleaved(cyl):
    """Each multigrid owns its spare image, its V-cycle graphs and its level-1
    tables: interleaved on one tree, every mode ends bitwise as alone on a
    fresh tree (modes 1, 2 on their own rhs / tmp, mode 3 on the shared)."""
    src = _source_field(_af(), seed=9)
    together = _interleaved(cyl, src)
    assert not np.array_equal(together[0][0], together[2][0])
    for k in range(3):
        (phi, tmp), = _interleaved(cyl, src, only=k)
        assert phi.any()
        assert np.array_equal(together[k][0], phi), k
        assert np.array_equal(together[k][1], tmp), k


# ----------------------------------------- 4. cylindrical Helmholtz operator
def _uniform2(c):
    L = c.ra("domain_len")
    af = AfTree(8, c.ra("domain_origin") + L, [16, 16], r_min=c.ra("domain_origin"))
    af.refine_up_to_lvl(2)
    return af


def _to_global(af, lvl, a):
    nc = af.nc
    n = 16 * 2 ** (lvl - 1)
    g = np.zeros((n, n))
    for b in af.lvls[lvl]["ids"]:
        i0, j0 = (af.ix[b][0] - 1) * nc, (af.ix[b][1] - 1) * nc
        g[j0:j0 + nc, i0:i0 + nc] = a[b - 1][1:-1, 1:-1]
    return g


def test_cylindrical_helmholtz_converges_to_the_discrete_solution():
    """tests/test_cyl_gpu.py's dense check with helmholtz_lambda = the square
    of the largest Bourdon-3 lambda and photoi_helmh_bc (Neumann 0 on the axis
    and the outer r face, Dirichlet 0 on the z faces): PFMG level-1 solve, an
    FMG, V-cycles until stationary, against numpy's dense solve; 1e-10."""
    from afh.driver import Case
    af = _uniform2(Case(golden.load(CASE)))
    sim = _sim(True, af=af)
    k = int(np.argmax(sim.helm_lambdas))
    mg, lam = sim.helm[k], sim.helm_lambdas[k]
    bc = [("n", 0.0), ("n", 0.0), ("d", 0.0), ("d", 0.0)]
    dr2 = af.dr[af.lvls[2]["ids"][0]]
    ng = af.nc + 2
    rhs = np.zeros((af.highest_id, ng, ng))
    Lx = af.domain[0] - af.r_base[0]
    for b in _used(af):
        xx, yy = state2d._cells(af, b)
        rhs[b - 1] = 1e20 * (3 * np.cos(2 * xx / Lx) + np.sin(5 * yy / Lx) + 40 * xx * yy / Lx ** 2)
    sim.tree.put_cc(mg.i_rhs, rhs)
    mg.fas_fmg(True, False)
    prev = None
    for n_v in range(1, 31):
        mg.fas_vcycle(True)
        cur = sim.tree.get_cc(mg.i_phi)
        if prev is not None and np.array_equal(cur, prev):
            break
        prev = cur
    got = _to_global(af, 2, cur)
    sim.tree.close()
    c2 = cn.lpl_coef(dr2, lam=lam * lam)
    row = sorted((af.ix[b][0], af.r_min[b][0]) for b in af.lvls[2]["ids"] if af.ix[b][1] == 1)
    t2 = cn.level_radius_tables(c2, [r for _, r in row], dr2[0], af.nc)
    n = got.shape[0]
    A, _ = cn.level_matrix(c2, t2, n, n, bc)
    ref = np.linalg.solve(A, _to_global(af, 2, rhs).reshape(-1)).reshape(n, n)
    rel = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("Helmholtz (lambda %.4g /m) FMG + %d V-cycles vs dense solve: max rel %.3g, "
          "lambda^2 / |c1| %.3g" % (lam, n_v, rel, lam * lam / abs(c2[0])))
    assert rel <= 1e-10


# ------------------------------------------------------------ 5. update term
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("cyl", [False, True])
def test_update_adds_the_photoionization_rate(cyl, fold):
    """Electrons 0, the photo_species ion uniform, every other species 0, a
    nonzero field: without the source every derivative vanishes, so one
    forward Euler step gives e = dt * photo and ion = n0 + dt * photo on the
    leaf interiors, bitwise; a fluid with i_photo = 0 changes nothing."""
    af = _af()
    rng = np.random.default_rng(23)
    ng, nf = af.nc + 2, af.nc + 1
    shape = (af.highest_id, ng, ng)
    dt, n0 = 3e-12, 2.5e15
    photo = 1e27 * rng.random(shape)
    photo[rng.random(shape) < 0.1] = 0.0
    _, inner = _leaf_mask(af)
    for with_photo in (True, False):
        sim = _sim(cyl, photoi=with_photo)
        iv_ion = sim.species_itree[sim.plasma[sim.photo_species - 1]]
        assert iv_ion != sim.i_electron
        sim.tree.put_cc(sim.i_efld, 2e6 + 4e6 * rng.random(shape))
        sim.tree.put_fc(sim.f_field, 4e6 * rng.standard_normal((af.highest_id, 2, nf, nf)))
        sim.tree.put_cc(iv_ion, np.full(shape, n0))
        sim.tree.put_cc(sim.i_photo, photo)
        if fold:
            sim.fluid.forward_euler_fold(dt, 0, [0], [1.0], 1, False)
            sim.fluid.fetch_step(False)
        else:
            sim.fluid.forward_euler(dt, 0, [0], [1.0], 1, False)
        for iv in sim.densities:
            got = sim.tree.get_cc(iv + 1)[inner]
            if iv == sim.i_electron:
                want = dt * photo[inner] if with_photo else np.zeros(inner.sum())
            elif iv == iv_ion:
                want = n0 + dt * photo[inner] if with_photo else np.full(inner.sum(), n0)
            else:
                want = np.zeros(inner.sum())
            assert np.array_equal(got, want), (iv, with_photo)
        if with_photo:
            assert np.count_nonzero(sim.tree.get_cc(sim.i_electron + 1)[inner]) > inner.sum() // 2
        sim.tree.close()


# -------------------------------------------------------------- 6. time loops
# Every case runs whole (on an MI355X 2.7 s, 3.3 s and 5.5 s per run). Measured
# maximum relative deviation from the reference's logs: 4.73e-8, 4.19e-8 and
# 4.25e-8, the logs' print precision; the bound is 10 x that, never
# above compare_logs' own 1e-5.
RTOL = {"rtest_test_2d_photoi": 4.8e-7, "rtest_test_2d_photoi_chem": 4.2e-7,
        "rtest_test_cyl_photoi_chem": 4.3e-7}


def _run_case(name):
    sim = Simulation(capi.hip_library_2d(), golden.load(name), device=0, **PFMG)
    assert sim.ndim == 2 and sim.photoi
    log = sim.run()
    sim.tree.close()
    return log


@pytest.mark.parametrize("name", sorted(RTOL))
def test_photoi_rtest_hip(name):
    """test_2d_photoi.cfg and test_2d_photoi_chem.cfg (7 ns, rows 0 .. 7) and
    test_cyl_photoi_chem.cfg (1.5 ns, rows 0 .. 6), each run whole: every row
    of the committed log is covered. Every row is within compare_logs'
    criterion, the reference's own (rtol 1e-5, atol 1e-8), and within RTOL;
    `it` equal and `time` within 1e-12; a second run of test_cyl_photoi_chem is
    bitwise the first."""
    ref = golden.load(name)["rtest_log"]
    log = _run_case(name)
    assert log.shape == ref.shape
    rel = np.abs(log - ref) / np.maximum(np.abs(ref), 1e-300)
    print("%s: %d rows, max rel per row" % (name, len(log)), rel[:, 2:].max(axis=1),
          "max", rel[:, 2:].max())
    assert np.array_equal(log[:, 0], ref[:, 0])
    assert np.allclose(log[:, 1], ref[:, 1], rtol=1e-12, atol=0)
    assert np.allclose(log, ref, rtol=1e-5, atol=1e-8)
    bad = ~np.isclose(log, ref, rtol=RTOL[name], atol=1e-8)
    assert not bad.any(), (np.argwhere(bad)[:5], rel.max())
    if "cyl" in name:
        assert np.array_equal(_run_case(name), log)

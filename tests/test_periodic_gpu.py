"""Periodic domains in the 3-D library (afh_tree_desc.periodic), on the GPU.

Trees (tests/periodic_numpy.py): P, 1 x 2 x 2 level-1 boxes periodic
(T, T, F) with three levels and a refinement boundary through the y seam,
and its tiled twin T, 3 x 3 copies without any periodic flag, whose centre
tile must equal P box by box, bit for bit, for every operation that reaches
less than a tile. The level-1 solves are held to numpy.linalg.solve of the
wrapped operator.
"""
import ctypes as C

import numpy as np
import pytest

import periodic_numpy as pn
from afh import capi
from afh.amr import AfTree
from afh.model import Multigrid, Tree, tree_desc

pytestmark = pytest.mark.gpu

I_PHI, I_RHS, I_TMP = 1, 2, 3
DIRZ = [(capi.BC_NEUMANN, 0.0)] * 4 + [(capi.BC_DIRICHLET, 0.0)] * 2
MODES = {"direct": dict(coarse_mode=capi.COARSE_DIRECT, coarse_cycles=0),
         "cycles": dict(coarse_mode=capi.COARSE_CYCLES, coarse_cycles=50, coarse_tol=1e-6),
         "pfmg": dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)}


def _lib():
    return capi.hip_library()


def _mg_tree(af, bc=DIRZ, **mg):
    tree = Tree(_lib(), af.topology(), 3, 0, device=0)
    for iv in (I_PHI, I_RHS, I_TMP):
        tree.set_cc_methods(iv, bc, capi.RB_MG_SIDES if iv == I_PHI else capi.RB_GC_INTERP)
    return tree, Multigrid(tree, I_PHI, I_RHS, I_TMP, **mg)


# ------------------------------------------------------------------- rules
def test_tree_create_accepts_the_flags():
    """afh_tree_create with periodic flags (refused before this feature), and
    what goes with it: a regrid must keep the flags, a sharded tree refuses
    them, the bc entries of a periodic dimension are accepted."""
    lib = _lib()
    P = pn.tree_P(levels=2)
    tree = Tree(lib, P.topology(), 1, 0, device=0)
    # Dirichlet 'values' on the periodic faces: accepted, never read
    tree.set_cc_methods(1, [(capi.BC_DIRICHLET, 7.0)] * 4 + [(capi.BC_NEUMANN, 0.0)] * 2)
    tree.set_bc(1, 1, capi.BC_NEUMANN, 3.0)
    tree.set_cc_prolong(1, capi.PROLONG_LINEAR)
    topo3 = pn.grow(P, (1, 1, 1), 3).topology()
    d, _keep = tree_desc(topo3, 1, 0)
    d.periodic[1] = 0
    h = C.c_void_p()
    with pytest.raises(capi.AfhError, match=r"\(-1\).*periodic flags differ"):
        lib.call("tree_regrid", tree.h, C.byref(d), C.byref(h))
    new = tree.regrid(topo3)
    assert new.get_cc(1).shape[0] == P.highest_id
    # a periodic extent is whole boxes
    d, _keep = tree_desc(topo3, 1, 0)
    d.coarse_grid_size[0] = 12
    with pytest.raises(capi.AfhError, match=r"\(-1\).*periodic dimension 1 of 12 cells"):
        lib.call("tree_create", C.byref(d), 0, C.byref(h))
    owner = np.zeros(P.highest_id, np.int32)
    with pytest.raises(capi.AfhError, match=r"\(-2\).*periodic.*sharded"):
        lib.call("tree_create_sharded", C.byref(tree_desc(topo3, 1, 0)[0]),
                 owner.ctypes.data_as(capi.P_i32), 0, 0, C.byref(h))
    new.close()
    tree.close()


def test_mg_create_rules():
    """The singular operator (periodic in all three dimensions, lambda = 0)
    is refused in every mode, with lambda > 0 it is fine; PFMG refuses a
    periodic extent that is no power of two (and takes one that is)."""
    full = AfTree(8, [1.0] * 3, [8, 8, 8], periodic=(True,) * 3)
    tree = Tree(_lib(), full.topology(), 3, 0, device=0)
    for iv in (1, 2, 3):
        tree.set_cc_methods(iv, DIRZ)
    for mode in MODES.values():
        with pytest.raises(capi.AfhError, match=r"\(-2\).*singular"):
            Multigrid(tree, 1, 2, 3, **mode)
        Multigrid(tree, 1, 2, 3, helmholtz_lambda=4.0, **mode).close()
    tree.close()
    odd = AfTree(4, [1.0] * 3, [12, 8, 8], periodic=(True, False, False))
    tree = Tree(_lib(), odd.topology(), 3, 0, device=0)
    for iv in (1, 2, 3):
        tree.set_cc_methods(iv, DIRZ)
    with pytest.raises(capi.AfhError, match=r"\(-2\).*power of two"):
        Multigrid(tree, 1, 2, 3, coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
    Multigrid(tree, 1, 2, 3, **MODES["cycles"]).close()
    tree.close()
    # 12 cells in a direction that is not periodic: PFMG's own business
    ok = AfTree(4, [1.0] * 3, [8, 12, 8], periodic=(True, False, False))
    tree = Tree(_lib(), ok.topology(), 3, 0, device=0)
    for iv in (1, 2, 3):
        tree.set_cc_methods(iv, DIRZ)
    Multigrid(tree, 1, 2, 3, **MODES["pfmg"]).close()
    tree.close()


# ---------------------------------------------------------- level-1 solves
def _level1_case(n, nc, periodic, seed, bc=DIRZ, lam=0.0, **mg):
    """Random phi and rhs on a level-1-only tree of n cells, one
    fas_vcycle(True, 1); returns (x, A, b, tmp): the solve's result, the numpy
    operator, the folded right-hand side, the library's residual."""
    dr = (2.0 ** -3, 2.0 ** -4, 2.0 ** -3)
    af = AfTree(nc, [n[d] * dr[d] for d in range(3)], list(n), periodic=periodic)
    tree, m = _mg_tree(af, bc, helmholtz_lambda=lam, **mg)
    rng = np.random.default_rng(seed)
    phi = rng.standard_normal(tree.cc_shape)
    rhs = rng.standard_normal(tree.cc_shape) * 100
    tree.put_cc(I_PHI, phi)
    tree.put_cc(I_RHS, rhs)
    m.fas_vcycle(True, 1)
    x = pn.gather_level1(af, tree.get_cc(I_PHI)).reshape(-1)
    tmp = pn.gather_level1(af, tree.get_cc(I_TMP)).reshape(-1)
    got = tree.get_cc(I_PHI)
    tree.close()
    if n[0] * n[1] * n[2] > 2048:  # too large for a dense matrix: its action
        shape = (n[2], n[1], n[0])
        A = _Apply(lambda u: pn.level1_apply(u.reshape(shape), dr, periodic, bc, lam).reshape(-1))
        fold = pn.level1_fold(n, dr, periodic, bc)
    else:
        A, fold = pn.level1_operator(n, dr, periodic, bc, lam)
    return x, A, fold(pn.gather_level1(af, rhs)), tmp, (af, got)


class _Apply:
    def __init__(self, f):
        self.f = f

    def __matmul__(self, u):
        return self.f(u)


WALLS = [(capi.BC_NEUMANN, 0.5)] * 4 + [(capi.BC_DIRICHLET, 2.0), (capi.BC_DIRICHLET, -1.0)]


@pytest.mark.parametrize("small", ["1", "0"])
def test_level1_direct(small, monkeypatch):
    """AFH_COARSE_DIRECT on 8 x 16 x 8 cells periodic (T, T, F), inhomogeneous
    z walls, against numpy.linalg.solve of the wrapped operator: the relative
    max-norm error is at most ten times that of the same grid built without
    the flags (today's cosine tables) in the same comparison. One workgroup
    (k_cs_direct_small) and the six transforms (k_cs_transform).

    Measured on an MI355X (profiles/periodic_pytest_gpu.txt), both launch
    forms: 1.056e-15 periodic, 1.267e-15 not periodic (the bound: 1.267e-14)."""
    monkeypatch.setenv("AFH_CS_DIRECT_SMALL", small)
    err = {}
    for per in (pn.PERIODIC, (False,) * 3):
        x, A, b, tmp, (af, got) = _level1_case((8, 16, 8), 8, per, 5, WALLS, **MODES["direct"])
        ref = np.linalg.solve(A, b)
        err[per] = np.max(np.abs(x - ref)) / np.max(np.abs(ref))
        # the library's own residual agrees with the numpy operator's
        assert np.max(np.abs(tmp - (b - A @ x))) <= 1e-9 * np.max(np.abs(b))
        if per == pn.PERIODIC:  # level 1's ghost cells after the solve: wrapped
            assert np.array_equal(pn.wrap_ghosts(af, got, 1), got)
    print("level-1 direct: relative max error periodic %.3e, not periodic %.3e (small=%s)"
          % (err[pn.PERIODIC], err[(False,) * 3], small))
    assert err[pn.PERIODIC] <= 10 * err[(False,) * 3]


@pytest.mark.parametrize("n,nc,per", [
    ((8, 16, 8), 8, (True, True, False)),    # the issue's grid
    ((4, 4, 4), 4, (True, True, False)),     # one coarsening, to 2 points per direction
    ((4, 8, 4), 4, (False, True, True)),     # a 2-point periodic bottom level
    ((16, 32, 16), 8, (True, True, False)),  # the multi-launch levels (k_cs_gsrb ...)
    ((24, 8, 8), 8, (True, False, False)),   # 24 -> 12 -> 6: never an odd periodic count
])
def test_level1_cycles_stopping_rule(n, nc, per):
    """AFH_COARSE_CYCLES with coarse_tol = 1e-6: |r|_2 <= tol |b|_2 by the
    numpy operator. (The walls of the first dimension that is not periodic
    are Dirichlet: without one the operator is singular.) The hierarchy
    halves a grid while every extent is even and at least 4, so 4 x 4 x 4
    has a second level of 2 x 2 x 2, where the one neighbour of a periodic
    direction enters twice."""
    _stopping_rule("cycles", n, nc, per)


def _stopping_rule(mode, n, nc, per):
    d = per.index(False)
    walls = [(capi.BC_NEUMANN, 0.5)] * 6
    walls[2 * d], walls[2 * d + 1] = (capi.BC_DIRICHLET, 2.0), (capi.BC_DIRICHLET, -1.0)
    x, A, b, tmp, _ = _level1_case(n, nc, per, 7, walls, **MODES[mode])
    ratio = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print("level-1", mode, n, per, "|r|/|b| = %.3e" % ratio)
    assert ratio <= 1e-6


@pytest.mark.parametrize("n,nc,per", [
    ((8, 16, 8), 8, (True, True, False)),    # the issue's grid: x goes 8, 4, 2, 1 (the fold)
    ((4, 4, 4), 4, (True, True, False)),
    ((4, 8, 4), 4, (False, True, True)),
    ((8, 8, 8), 8, (False, False, False)),   # the same test on today's path
    ((16, 32, 16), 8, (True, True, False)),  # too large for LDS: the vectors in global memory
])
def test_level1_pfmg_stopping_rule(n, nc, per):
    """AFH_COARSE_PFMG (k_cs_pfmg with the wrapped set-up of afh_pfmg.h) with
    coarse_tol = 1e-6, at most 50 iterations: |r|_2 <= tol |b|_2 by the numpy
    operator. Every periodic direction is semicoarsened down to one point,
    through the level of 2 points whose odd point has one coarse neighbour
    twice and the 1-point level whose offsets fold onto the centre. The
    set-up (weights, R A P) is checked through this solve only: the host
    code of afh_pfmg.h is reached on the CPU through the oracle's probes,
    which take no flags (tests/test_periodic_cpu.py checks the set-up itself
    through a probe of its own).

    Iterations: with x periodic the means of the operator's coefficients no
    longer tie between x and z (z loses its wall entries), PFMG's rules then
    coarsen y, x, y, z instead of y, y, x, z and skip the relaxation of level
    1, and the solve takes about twice the iterations (37 against 17 on
    8 x 16 x 8; a numpy restatement of the cycle from the host tables takes
    33 against 18), within its 50."""
    if not any(per):
        x, A, b, tmp, _ = _level1_case(n, nc, per, 7, WALLS, **MODES["pfmg"])
        assert np.linalg.norm(b - A @ x) <= 1e-6 * np.linalg.norm(b)
        return
    _stopping_rule("pfmg", n, nc, per)


@pytest.mark.parametrize("mode", ["direct", "cycles", "pfmg"])
def test_level1_fully_periodic_helmholtz(mode):
    """Periodic in all three dimensions with lambda > 0 (the photoionization
    modes): against numpy.linalg.solve."""
    x, A, b, tmp, _ = _level1_case((8, 8, 8), 8, (True,) * 3, 9, DIRZ, lam=50.0, **MODES[mode])
    ref = np.linalg.solve(A, b)
    err = np.max(np.abs(x - ref)) / np.max(np.abs(ref))
    ratio = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print("fully periodic helmholtz", mode, "relative max error %.3e |r|/|b| %.3e" % (err, ratio))
    if mode == "direct":
        assert err <= 1e-12  # (a well-conditioned 512 x 512 system, errors of some 1e-15)
    else:
        assert ratio <= 1e-6


def test_tables_follow_the_bc_types():
    """The cached tables key on the bc types next to the flags: changing a
    physical wall's type on a periodic tree rebuilds them (tab_bc / q_bc,
    PFMG's hierarchy). The iterative modes get 200 iterations here: this is
    about the operator they solve, not about how soon (PFMG needs some 35
    iterations for six decades on this grid, below)."""
    for mode in ("direct", "cycles", "pfmg"):
        n, dr = (8, 16, 8), (2.0 ** -3, 2.0 ** -4, 2.0 ** -3)
        af = AfTree(8, [n[d] * dr[d] for d in range(3)], list(n), periodic=pn.PERIODIC)
        tree, m = _mg_tree(af, DIRZ, **dict(MODES[mode], coarse_cycles=0 if mode == "direct" else 200))
        rng = np.random.default_rng(2)
        phi, rhs = rng.standard_normal(tree.cc_shape), rng.standard_normal(tree.cc_shape)
        for bc in (DIRZ, DIRZ[:5] + [(capi.BC_NEUMANN, 0.0)]):
            tree.set_cc_methods(I_PHI, bc, capi.RB_MG_SIDES)
            tree.put_cc(I_PHI, phi)
            tree.put_cc(I_RHS, rhs)
            m.fas_vcycle(True, 1)
            x = pn.gather_level1(af, tree.get_cc(I_PHI)).reshape(-1)
            A, fold = pn.level1_operator(n, dr, pn.PERIODIC, bc)
            b = fold(pn.gather_level1(af, rhs))
            assert np.linalg.norm(b - A @ x) <= 1e-6 * np.linalg.norm(b), (mode, bc[5])
        tree.close()


# --------------------------------------------------------- whole field solve
def _cycles_to(af, phi, rhs, mode, n_max=40):
    tree, m = _mg_tree(af, DIRZ, **MODES[mode])
    tree.put_cc(I_PHI, phi)
    tree.put_cc(I_RHS, rhs)
    r = [m.fas_vcycle_maxres() for _ in range(n_max)]
    tree.close()
    return r


@pytest.mark.parametrize("mode", ["direct", "cycles", "pfmg"])
def test_vcycles_converge_on_P(mode):
    """V-cycles on P (three levels, refinement boundary through the seam):
    the cycles the same tree without the flags needs to fall below 1e-9 of
    its first residual, plus two, bring P below 1e-9 too."""
    P = pn.tree_P()
    W = pn.walled_like(P)
    rng = np.random.default_rng(11)
    phi_p, phi_w = pn.fill_by_location(P, W, rng)
    rhs_p, rhs_w = pn.fill_by_location(P, W, rng, scale=1e6)
    rw, rp = _cycles_to(W, phi_w, rhs_w, mode), _cycles_to(P, phi_p, rhs_p, mode)
    need = next(k for k, v in enumerate(rw) if v < 1e-9 * rw[0])
    print("V-cycles", mode, "walled needs", need, "residuals P", rp[:need + 3])
    assert rp[min(need + 2, len(rp) - 1)] < 1e-9 * rp[0]


def _order_error(lvl, mode):
    L = 1.0
    af = AfTree(8, [L] * 3, [16] * 3, periodic=pn.PERIODIC)
    af.refine_up_to_lvl(lvl)
    tree, m = _mg_tree(af, DIRZ, **MODES[mode])
    ng = 10
    rhs = np.zeros(tree.cc_shape)
    exact = np.zeros(tree.cc_shape)
    idx = np.arange(ng) - 0.5
    for b in range(1, af.highest_id + 1):
        x = af.r_min[b][0] + idx * af.dr[b][0]
        y = af.r_min[b][1] + idx * af.dr[b][1]
        z = af.r_min[b][2] + idx * af.dr[b][2]
        u = (np.sin(np.pi * z / L)[:, None, None] * np.sin(2 * np.pi * y / L)[None, :, None] *
             np.sin(2 * np.pi * x / L)[None, None, :])
        exact[b - 1] = u
        rhs[b - 1] = -(9 * np.pi ** 2 / L ** 2) * u   # lpl(phi) = rhs, i.e. -lpl(phi) = f
    tree.put_cc(I_RHS, rhs)
    m.fas_fmg(True, have_guess=False)
    res = [m.fas_vcycle_maxres() for _ in range(12)]
    phi = tree.get_cc(I_PHI)
    tree.close()
    leaves = np.asarray(af.lvls[lvl]["ids"]) - 1
    inner = (slice(None),) + (slice(1, -1),) * 3
    return np.max(np.abs(phi[leaves][inner] - exact[leaves][inner])), res


@pytest.mark.parametrize("mode", ["direct", "cycles", "pfmg"])
def test_second_order(mode):
    """-lpl(phi) = f with phi = sin(2 pi x / L) sin(2 pi y / L) sin(pi z / L),
    periodic in x and y, Dirichlet 0 in z, on uniform trees of 32^3 and 64^3
    cells (FMG, then V-cycles to rounding): the max error falls by more than
    3 per doubling (second order: 4 in the limit)."""
    e2, r2 = _order_error(2, mode)
    e3, r3 = _order_error(3, mode)
    print("order", mode, "errors %.4e %.4e ratio %.3f" % (e2, e3, e2 / e3), r3[-3:])
    assert r3[-1] < 1e-8 * 9 * np.pi ** 2  # (max |rhs| = 9 pi^2)
    assert e2 / e3 > 3.0


# ------------------------------------------- ghost cells and transfers, P / T
NEUZ = [(capi.BC_NEUMANN, 0.0)] * 4 + [(capi.BC_DIRICHLET, 1.5), (capi.BC_DIRICHLET, -0.5)]


def _pair_trees(P, T, nvar, nface=0):
    lib = _lib()
    return (Tree(lib, P.topology(), nvar, nface, device=0, box_capacity=64),
            Tree(lib, T.topology(), nvar, nface, device=0, box_capacity=600))


def _same_centre(P, T, a, b, what):
    for p, q in pn.box_map(P, T).items():
        assert np.array_equal(a[p - 1], b[q - 1], equal_nan=True), (what, pn.box_key(P, p))


@pytest.mark.parametrize("rb", [capi.RB_GC_INTERP, capi.RB_GC_INTERP_LIM, capi.RB_MG_SIDES])
def test_gc_tree_and_restrict_equal_the_twin(rb):
    """afh_gc_tree (with and without corners) and afh_restrict_tree on P
    against the twin's centre tile, every cell of every box bitwise."""
    P, T = pn.tree_P(), pn.tree_T()
    tp, tt = _pair_trees(P, T, 1)
    ap, at = pn.fill_by_location(P, T, np.random.default_rng(3))
    for corners in (False, True):
        out = []
        for tree, a in ((tp, ap), (tt, at)):
            tree.set_cc_methods(1, NEUZ, rb)
            tree.put_cc(1, a)
            tree.gc_tree(1, corners)
            out.append(tree.get_cc(1))
        assert not np.array_equal(out[0], ap)
        _same_centre(P, T, out[0], out[1], ("gc_tree", rb, corners))
    out = []
    for tree, a in ((tp, ap), (tt, at)):
        tree.put_cc(1, a)
        tree.restrict_tree(1)
        tree.gc_tree(1, True)
        out.append(tree.get_cc(1))
    _same_centre(P, T, out[0], out[1], ("restrict_tree", rb))
    tp.close(), tt.close()


@pytest.mark.parametrize("method", [capi.PROLONG_LINEAR, capi.PROLONG_LIMIT])
def test_regrid_equals_the_twin(method):
    """afh_tree_regrid from two levels to three (new boxes on levels 2 and 3,
    prolonged from parents whose ghost cells came by wrap; their own ghost
    cells filled, corners included)."""
    P, T = pn.tree_P(levels=2), pn.tree_T(levels=2)
    tp, tt = _pair_trees(P, T, 1)
    ap, at = pn.fill_by_location(P, T, np.random.default_rng(4))
    for tree, a in ((tp, ap), (tt, at)):
        tree.set_cc_methods(1, NEUZ, capi.RB_GC_INTERP_LIM)
        tree.set_cc_prolong(1, method)
        tree.put_cc(1, a)
        tree.restrict_tree(1)
        tree.gc_tree(1, True)
    pn.grow(P, (1, 1, 1), 3), pn.grow(T, (3, 3, 1), 3)
    assert P.highest_lvl == 3 and P.highest_id == 44
    np_, nt = tp.regrid(P.topology()), tt.regrid(T.topology())
    _same_centre(P, T, np_.get_cc(1), nt.get_cc(1), ("regrid", method))
    for t in (np_, nt, tp, tt):
        t.close()


def test_gc_tree_is_a_wrap_of_interiors():
    """Not everything rests on the twin: on a uniform two-level periodic
    tree the face ghost cells of both levels are the neighbours' interiors
    by direct wrap (tests/periodic_numpy.py wrap_ghosts)."""
    af = AfTree(8, [8 * pn.DR, 16 * pn.DR, 16 * pn.DR], [8, 16, 16], periodic=pn.PERIODIC)
    af.refine_up_to_lvl(2)
    tree = Tree(_lib(), af.topology(), 1, 0, device=0)
    tree.set_cc_methods(1, NEUZ, capi.RB_GC_INTERP)
    a = np.random.default_rng(5).standard_normal(tree.cc_shape)
    tree.put_cc(1, a)
    tree.gc_tree(1, True)
    got = tree.get_cc(1)
    tree.close()
    assert np.array_equal(got[:, 1:-1, 1:-1, 1:-1], a[:, 1:-1, 1:-1, 1:-1])
    for lvl in (1, 2):
        want = pn.wrap_ghosts(af, got, lvl)
        ids = np.asarray(af.lvls[lvl]["ids"]) - 1
        assert np.array_equal(want[ids], got[ids])
        # and they are not what was put there
        assert not np.array_equal(got[ids][:, 1:-1, 1:-1, 0], a[ids][:, 1:-1, 1:-1, 0])


# ------------------------------------------------------------- species step
def _sim(af, monkeypatch=None, env=None, case_name="rtest_test_3d"):
    """The rtest_test_3d model (tabulated rates) bound to the tree `af`."""
    import golden
    from afh.driver import Simulation
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    case = dict(golden.load(case_name))
    case["periodic"] = np.array([int(p) for p in af.periodic])
    sim = Simulation(_lib(), case, device=0)
    sim.af = af
    sim._bind(sim._create_tree())
    return sim


def _species_state(sim, arrays):
    """Densities (both states), phi and |E| from box arrays by location."""
    k = 0
    for iv in sim.densities:
        for s in (0, 1):
            sim.tree.put_cc(iv + s, arrays[k])
            k += 1
    sim.tree.put_cc(sim.i_phi, arrays[k])
    sim.tree.gc_tree(sim.i_phi)
    sim.field_from_potential()


def _heun(sim, arrays=None):
    """Heun's two stages; with `arrays` the second starts from that state
    again (put by location) instead of from the first stage's result."""
    lims = [sim.fluid.forward_euler(1e-12, 0, [0], [1.0], 1, False)]
    out = [sim.tree.get_cc(iv + 1) for iv in sim.densities]
    if arrays is not None:
        _species_state(sim, arrays)
    lims.append(sim.fluid.forward_euler(5e-13, 1, [0, 1], [0.5, 0.5], 0, True))
    return lims, out + [sim.tree.get_cc(iv) for iv in sim.densities]


def test_species_step_equals_the_twin():
    """afh_fluid_forward_euler, Heun stages 1 and 2, on P against the twin
    whose every tile holds P's data: the centre tile's densities and all
    four limits (extremes over tiles of equal values) bitwise. Each stage
    starts from data put by location: the first stage's result differs next
    to T's outer walls, which P does not have. (For the same reason a cell at
    T's outer wall could own an extreme that P lacks; with these data none
    does.)"""
    P, T = pn.tree_P(), pn.tree_T()
    sp, st = _sim(P), _sim(T)
    rng = np.random.default_rng(6)
    n = 2 * len(sp.densities)
    pairs = [pn.fill_by_location(P, T, rng, scale=1e16, positive=True) for _ in range(n)]
    pairs.append(pn.fill_by_location(P, T, rng, scale=2e3))  # phi: |E| of some 1e6 V/m
    _species_state(sp, [a for a, _ in pairs])
    _species_state(st, [b for _, b in pairs])
    lp, dp = _heun(sp, [a for a, _ in pairs])
    lt, dt = _heun(st, [b for _, b in pairs])
    print("limits P", lp, "T", lt)
    assert lp == lt
    inner = (slice(1, -1),) * 3
    leaves = P.leaves()
    m = pn.box_map(P, T)
    for a, b in zip(dp, dt):
        for p in leaves:
            assert np.array_equal(a[p - 1][inner], b[m[p] - 1][inner]), pn.box_key(P, p)
    assert not np.array_equal(dp[0], pairs[0][0])
    sp.tree.close(), st.tree.close()


def test_species_step_equals_the_reference(monkeypatch):
    """The device step on P against the reference's forward_euler with
    periodic = T T F (tests/golden/replay_periodic.npz): the densities of
    both Heun stages and dt_lim, bitwise."""
    import state_periodic as sp
    sp.replay_against_reference(_lib(), 0, monkeypatch)


def test_fused_species_step_64_periodic(monkeypatch):
    """k_fe_lds<64> on one level of 1 x 2 x 2 boxes of 64^3, periodic
    (T, T, F): AFH_FE_FUSED=1 against 0, both Heun stages, bitwise; the
    fused kernel did run (its launches are counted)."""
    out = {}
    for fused in ("1", "0"):
        af = AfTree(64, [64 * pn.DR, 128 * pn.DR, 128 * pn.DR], [64, 128, 128],
                    periodic=pn.PERIODIC)
        sim = _sim(af, monkeypatch, {"AFH_FE_FUSED": fused})
        rng = np.random.default_rng(8)
        shape = sim.tree.cc_shape
        arrays = [np.abs(rng.standard_normal(shape)) * 1e16 + 1e15
                  for _ in range(2 * len(sim.densities))]
        arrays.append(rng.standard_normal(shape) * 2e3)
        _species_state(sim, arrays)
        sim.lib.call("profile_enable", sim.tree.h, capi.PROF_FE)
        res = _heun(sim)
        ms, nl, by = C.c_double(), C.c_int64(), C.c_double()
        sim.lib.call("profile_read", sim.tree.h, C.byref(ms), C.byref(nl), C.byref(by))
        assert (nl.value > 0) == (fused == "1"), nl.value
        out[fused] = res
        sim.tree.close()
    assert out["1"][0] == out["0"][0]
    assert len(out["1"][1]) == 2 * len(sim.densities)
    for a, b in zip(out["1"][1], out["0"][1]):
        assert np.array_equal(a[:, 1:-1, 1:-1, 1:-1], b[:, 1:-1, 1:-1, 1:-1])


# ----------------------------------------------------------------- smoothers
PLAIN = {"AFH_GSRB_FUSED_MIN_BOXES": "0", "AFH_PAIR_PUSH": "0", "AFH_PROLONG_PUSH": "0",
         "AFH_RSTR_PUSH": "0"}


def _vcycle_snaps(af, env, monkeypatch, seed, stages):
    for k in PLAIN:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tree, m = _mg_tree(af, NEUZ, **MODES["direct"])
    rng = np.random.default_rng(seed)
    tree.put_cc(I_PHI, rng.standard_normal(tree.cc_shape))
    tree.put_cc(I_RHS, rng.standard_normal(tree.cc_shape) * 1e6)
    snaps = []
    for k in range(4):  # without the residual pass, then eager, capture, replay
        m.fas_vcycle(k > 0)
        if k in stages:
            phi = tree.get_cc(I_PHI)
            # phi with its face ghost cells: the edges and corners out
            keep = np.zeros(phi.shape[1:], bool)
            keep[1:-1, 1:-1, :] = keep[1:-1, :, 1:-1] = keep[:, 1:-1, 1:-1] = True
            inner = (slice(None),) + (slice(1, -1),) * 3
            snaps.append((np.where(keep, phi, 0.0), tree.get_cc(I_RHS)[inner],
                          tree.get_cc(I_TMP)[inner]))
    tree.close()
    return snaps


def _used(af):
    return np.asarray([b for b in range(1, af.highest_id + 1) if af.in_use[b]]) - 1


@pytest.mark.parametrize("nc", [8, 4, 16])
def test_smoother_launch_variants_on_P(nc, monkeypatch):
    """The default launch set (fused pairs on every level of small boxes,
    pushing pair / correction / restriction: a box one wide pushes into its
    own ghost layer) against the split half-sweeps with level fills, on P:
    phi with its face ghost cells, rhs and tmp bitwise after a V-cycle
    without the residual pass and after each of three with it (eager,
    capture, replay)."""
    af = pn.tree_P(nc)
    a = _vcycle_snaps(af, {}, monkeypatch, 12, (0, 1, 2, 3))
    b = _vcycle_snaps(af, PLAIN, monkeypatch, 12, (0, 1, 2, 3))
    ix = _used(af)
    for k, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(("phi", "rhs", "tmp"), x, y):
            assert np.array_equal(u[ix], v[ix]), (nc, k, name)
    assert not np.array_equal(a[0][0][ix], a[3][0][ix])


def test_smoother_launch_variants_64_self_neighbour(monkeypatch):
    """64^3 boxes, 1 x 2 x 2 on level 1, all refined once, with
    AFH_GSRB_FUSED_MIN_BOXES=1: k_gsrb_pair2 (and the tiled pair) on a level
    whose box is its own x neighbour, against the split set."""
    af = AfTree(64, [64 * pn.DR, 128 * pn.DR, 128 * pn.DR], [64, 128, 128],
                periodic=pn.PERIODIC)
    af.refine_up_to_lvl(2)
    a = _vcycle_snaps(af, {"AFH_GSRB_FUSED_MIN_BOXES": "1"}, monkeypatch, 13, (0, 1, 2, 3))
    b = _vcycle_snaps(af, PLAIN, monkeypatch, 13, (0, 1, 2, 3))
    for k, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(("phi", "rhs", "tmp"), x, y):
            assert np.array_equal(u, v), (k, name)


# -------------------------------------------------------------------- driver
def test_driver_ten_steps_periodic():
    """Simulation on rtest_test_3d with periodic = [1, 1, 0]: the initial
    refinement (three regrids of the periodic tree), ten steps, and on until
    a regrid inside the time loop has changed the tree; then every density's
    face ghost cells across both seams are the neighbour's interior, the log
    rows are finite, and a refined box has a same-level neighbour by wrap."""
    import golden
    from afh.driver import Simulation
    case = dict(golden.load("rtest_test_3d"))
    case["periodic"] = np.array([1, 1, 0])
    sim = Simulation(_lib(), case, device=0)
    regrids = []
    orig = sim.adjust_refinement

    def counted():
        info = orig()
        regrids.append((sim.it, info.n_add, info.n_rm))
        return info

    sim.adjust_refinement = counted
    sim.start()
    for _ in range(10):
        assert sim.step()
    while not any(it > 0 and (n_add or n_rm) for it, n_add, n_rm in regrids) and sim.it < 120:
        assert sim.step()
    print("periodic driver: boxes", sim.af.highest_id, "levels", sim.af.highest_lvl,
          "regrids (step, added, removed)", regrids)
    assert any(it == 0 and n_add for it, n_add, _ in regrids)
    assert any(it > 0 and (n_add or n_rm) for it, n_add, n_rm in regrids)
    rows = [sim.regression_row()] + list(sim.log)
    assert all(np.all(np.isfinite(r)) for r in rows)
    af, nc = sim.af, sim.af.nc
    wrapped = 0
    for iv in sim.densities:
        sim.tree.restrict_tree(iv)
        sim.tree.gc_tree(iv)
        a = sim.tree.get_cc(iv)
        for b in range(1, af.highest_id + 1):
            if not af.in_use[b]:
                continue
            for nb in range(4):  # the x and y faces
                o = af.neighbors[b][nb]
                d, up = nb // 2, nb % 2
                if o <= 0 or (o != b and (af.ix[o][d] > af.ix[b][d]) == bool(up)):
                    continue  # no same-level neighbour, or not across a seam
                wrapped += af.lvl[b] >= 2
                ghost = [slice(1, -1)] * 3
                inner = [slice(1, -1)] * 3
                ghost[2 - d] = nc + 1 if up else 0
                inner[2 - d] = 1 if up else nc
                assert np.array_equal(a[b - 1][tuple(ghost)], a[o - 1][tuple(inner)]), (iv, b, nb)
    assert wrapped > 0
    sim.tree.close()

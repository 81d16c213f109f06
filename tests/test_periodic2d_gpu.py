"""Periodic domains in the 2-D library (afh_tree_desc.periodic[0..1]), on the
GPU.

Trees (tests/periodic2d_numpy.py): P, 1 x 2 level-1 boxes periodic (T, F)
with three levels, level 3 wrapping onto itself in x and with a refinement
boundary through the x seam; its tiled twin T, three copies in x without any
flag, whose centre tile must equal P box by box, bit for bit, for every
operation that reaches less than a tile; Py / Ty the same for (F, T), also on
cylindrical trees (z is translation invariant, r is not). The level-1 solves
are held to numpy.linalg.solve of the wrapped operator.
"""
import ctypes as C

import numpy as np
import pytest

import periodic2d_numpy as p2
from afh import capi
from afh.amr import AF_CYL, AF_XYZ, AfTree
from afh.model import Multigrid, Tree, tree_desc

pytestmark = pytest.mark.gpu

I_PHI, I_RHS, I_TMP = 1, 2, 3
DIRY = [(capi.BC_NEUMANN, 0.0)] * 2 + [(capi.BC_DIRICHLET, 0.0)] * 2
WALLS = [(capi.BC_NEUMANN, 0.5)] * 2 + [(capi.BC_DIRICHLET, 2.0), (capi.BC_DIRICHLET, -1.0)]
MODES = {"direct": dict(coarse_mode=capi.COARSE_DIRECT, coarse_cycles=0),
         "pfmg": dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)}


def _lib():
    return capi.hip_library_2d()


def _bare_tree(af, nvar, nface=0):
    tree = Tree(_lib(), af.topology(), nvar, nface, device=0)
    if af.coord == AF_CYL:
        tree.set_coord(capi.COORD_CYL)
    return tree


def _mg_tree(af, bc=DIRY, **mg):
    tree = _bare_tree(af, 3)
    for iv in (I_PHI, I_RHS, I_TMP):
        tree.set_cc_methods(iv, bc, capi.RB_MG_SIDES if iv == I_PHI else capi.RB_GC_INTERP)
    return tree, Multigrid(tree, I_PHI, I_RHS, I_TMP, **mg)


# ------------------------------------------------------------------- rules
def test_tree_rules():
    """afh_tree_create keeps both flags: a regrid hands them on and refuses
    other flags, a periodic extent is whole boxes, cylindrical with a periodic
    r stays refused and with a periodic z is allowed, the bc entries of a
    periodic dimension are accepted."""
    lib = _lib()
    P = p2.tree_P(levels=2)
    tree = Tree(lib, P.topology(), 1, 0, device=0)
    # Dirichlet 'values' on the periodic faces: accepted, never read
    tree.set_cc_methods(1, [(capi.BC_DIRICHLET, 7.0)] * 2 + [(capi.BC_NEUMANN, 0.0)] * 2)
    tree.set_bc(1, 1, capi.BC_NEUMANN, 3.0)
    tree.set_cc_prolong(1, capi.PROLONG_LINEAR)
    topo3 = p2.grow(P, 0, 3).topology()
    h = C.c_void_p()
    for flags in ((0, 0), (1, 1), (0, 1)):
        d, _keep = tree_desc(topo3, 1, 0)
        d.periodic[0], d.periodic[1] = flags
        with pytest.raises(capi.AfhError, match=r"\(-1\).*periodic flags differ"):
            lib.call("tree_regrid", tree.h, C.byref(d), C.byref(h))
    new = tree.regrid(topo3)
    assert new.get_cc(1).shape[0] == P.highest_id
    # the regridded tree kept the flags: a regrid of it without them is refused
    d, _keep = tree_desc(topo3, 1, 0)
    d.periodic[0] = 0
    with pytest.raises(capi.AfhError, match=r"\(-1\).*periodic flags differ"):
        lib.call("tree_regrid", new.h, C.byref(d), C.byref(h))
    # periodic[2] is ignored
    d, _keep = tree_desc(topo3, 1, 0)
    d.periodic[2] = 1
    lib.call("tree_create", C.byref(d), 0, C.byref(h))
    lib.call("tree_destroy", h)
    # a periodic extent is whole boxes
    for q in (0, 1):
        d, _keep = tree_desc(topo3, 1, 0)
        d.periodic[0], d.periodic[1] = int(q == 0), int(q == 1)
        d.coarse_grid_size[q] = 12
        with pytest.raises(capi.AfhError,
                           match=r"\(-1\).*periodic dimension %d of 12 cells" % (q + 1)):
            lib.call("tree_create", C.byref(d), 0, C.byref(h))
    with pytest.raises(capi.AfhError, match=r"\(-1\).*cylindrical with a periodic r"):
        new.set_coord(capi.COORD_CYL)
    new.close()
    tree.close()
    Py = p2.tree_P(levels=2, pd=1)
    tree = Tree(lib, Py.topology(), 1, 0, device=0)
    tree.set_coord(capi.COORD_CYL)
    assert tree.coord == capi.COORD_CYL
    tree.close()


def test_mg_create_rules():
    """Periodic in both dimensions with lambda = 0 is refused as singular in
    both modes, with lambda > 0 it is fine; PFMG refuses a periodic extent
    that is no power of two, DIRECT takes it, and PFMG takes such an extent
    in the walled dimension."""
    full = AfTree(8, [1.0] * 2, [8, 8], periodic=(True, True))
    tree = Tree(_lib(), full.topology(), 3, 0, device=0)
    for iv in (1, 2, 3):
        tree.set_cc_methods(iv, DIRY)
    for mode in MODES.values():
        with pytest.raises(capi.AfhError, match=r"\(-2\).*singular"):
            Multigrid(tree, 1, 2, 3, **mode)
        Multigrid(tree, 1, 2, 3, helmholtz_lambda=4.0, **mode).close()
    tree.close()
    for grid, per, ok in (([12, 8], (True, False), False), ([8, 12], (False, True), False),
                          ([8, 12], (True, False), True)):
        af = AfTree(4, [1.0] * 2, grid, periodic=per)
        tree = Tree(_lib(), af.topology(), 3, 0, device=0)
        for iv in (1, 2, 3):
            tree.set_cc_methods(iv, DIRY)
        if ok:
            Multigrid(tree, 1, 2, 3, **MODES["pfmg"]).close()
        else:
            with pytest.raises(capi.AfhError, match=r"\(-2\).*power of two"):
                Multigrid(tree, 1, 2, 3, **MODES["pfmg"])
        Multigrid(tree, 1, 2, 3, **MODES["direct"]).close()
        tree.close()


# ---------------------------------------------------------- level-1 solves
def _level1_case(n, nc, periodic, seed, bc=DIRY, lam=0.0, cyl=False, stencil=None, **mg):
    """Random phi and rhs on a level-1-only tree of n cells, one
    fas_vcycle(True, 1); returns (x, A, b, tmp, (af, phi after)): the solve's
    result, the numpy operator, the folded right-hand side, the library's
    residual. stencil: (box id, v (nc, nc, 5), bc_correction (nc, nc)) of an
    electrode box."""
    dr = p2.L1_DR
    af = AfTree(nc, [n[d] * dr[d] for d in range(2)], list(n), periodic=periodic,
                coord=AF_CYL if cyl else AF_XYZ)
    tree, m = _mg_tree(af, bc, helmholtz_lambda=lam, **mg)
    rng = np.random.default_rng(seed)
    phi = rng.standard_normal(tree.cc_shape)
    rhs = rng.standard_normal(tree.cc_shape) * 100
    v = None
    if stencil is not None:
        box, vb, fb = stencil
        m.set_box_stencil(box, vb, fb)
        o = [(x - 1) * nc for x in af.ix[box]]
        v = {(o[0] + i, o[1] + j): tuple(vb[j, i]) for j in range(nc) for i in range(nc)}
    tree.put_cc(I_PHI, phi)
    tree.put_cc(I_RHS, rhs)
    m.fas_vcycle(True, 1)
    got = tree.get_cc(I_PHI)
    x = p2.gather_level1(af, got).reshape(-1)
    tmp = p2.gather_level1(af, tree.get_cc(I_TMP)).reshape(-1)
    tree.close()
    A, fold = p2.level1_operator(n, dr, periodic, bc, lam, cyl, v)
    g = p2.gather_level1(af, rhs)
    if stencil is not None:
        o = [(x_ - 1) * nc for x_ in af.ix[stencil[0]]]
        g[o[1]:o[1] + nc, o[0]:o[0] + nc] += stencil[2]
    return x, A, fold(g), tmp, (af, got)


@pytest.mark.parametrize("n,nc", [((8, 16), 8), ((12, 8), 4)])
def test_level1_direct(n, nc):
    """AFH_COARSE_DIRECT periodic (T, F) with inhomogeneous Dirichlet y
    walls, on 8 x 16 cells and on 12 x 8 (no power of two, three boxes across
    the seam), against numpy.linalg.solve of the wrapped operator: the
    relative max-norm error is at most ten times that of the same grid built
    without the flags (the cosine tables) in the same comparison. The
    library's residual agrees with b - A x of the numpy operator, and level
    1's ghost cells across the seam are the wrapped interiors. Without the
    periodic level-1 solve the seam is a Neumann wall and the first bound
    fails by many orders (the parent commit's library: 6.4e-2 on 8 x 16).

    Measured on an MI355X (profiles/periodic2d_pytest_gpu.txt): 8 x 16
    1.989e-15 periodic against 1.422e-15 without flags; 12 x 8 1.441e-15
    against 1.416e-15; the residuals agree to 3.3e-16 max|b|."""
    err, res_err, wrapped = {}, {}, None
    for per in ((True, False), (False, False)):
        x, A, b, tmp, (af, got) = _level1_case(n, nc, per, 5, WALLS, **MODES["direct"])
        ref = np.linalg.solve(A, b)
        err[per] = np.max(np.abs(x - ref)) / np.max(np.abs(ref))
        res_err[per] = np.max(np.abs(tmp - (b - A @ x))) / np.max(np.abs(b))
        print("level-1 direct", n, per, "relative max error %.3e, residual difference / max|b| "
              "%.3e" % (err[per], res_err[per]))
        if per[0]:
            wrapped = np.array_equal(p2.wrap_ghosts(af, got, 1), got)
    assert err[(True, False)] <= 10 * err[(False, False)]
    assert max(res_err.values()) <= 1e-9
    assert wrapped


def _cycles_needed(n, nc, per, seed, bc, **kw):
    """The device's iteration count, without an entry point for it: the
    solve stops by its rule after k iterations, so every coarse_cycles >= k
    gives the same phi bit for bit and every smaller one another."""
    pf = dict(MODES["pfmg"])
    full = _level1_case(n, nc, per, seed, bc, **dict(kw, **pf))[0]
    lo, hi = 1, pf["coarse_cycles"]
    while lo < hi:
        mid = (lo + hi) // 2
        x = _level1_case(n, nc, per, seed, bc, **dict(kw, **dict(pf, coarse_cycles=mid)))[0]
        if np.array_equal(x, full):
            hi = mid
        else:
            lo = mid + 1
    return lo


def _dirichlet_walls(per):
    d = per.index(False)
    walls = [(capi.BC_NEUMANN, 0.5)] * 4
    walls[2 * d], walls[2 * d + 1] = (capi.BC_DIRICHLET, 2.0), (capi.BC_DIRICHLET, -1.0)
    return walls


@pytest.mark.parametrize("n,nc,per,cyl", [
    ((8, 16), 8, (True, False), False),   # x goes 8, 4, 2, 1 (the fold)
    ((4, 4), 4, (True, False), False),    # the 2-point and 1-point periodic levels
    ((8, 4), 4, (False, True), False),
    ((8, 16), 8, (False, False), False),  # the same test on the path without flags
    ((8, 16), 8, (False, True), True),    # cylindrical, periodic z
])
def test_level1_pfmg_stopping_rule(n, nc, per, cyl):
    """AFH_COARSE_PFMG (k2_cs_pfmg with afh_pfmg_setup_per, ndim = 2) with
    coarse_tol = 1e-6, at most 50 iterations: |b - A x|_2 <= 1e-6 |b|_2 by
    the numpy operator. The grids were fixed on the CPU first
    (tests/test_periodic2d_cpu.py restates the cycle from the host set-up:
    34, 19, 9, 11 and 14 iterations in this order); the device's counts are
    printed (29, 18, 12, 10 and 13 on an MI355X,
    profiles/periodic2d_pytest_gpu.txt)."""
    bc = WALLS if not any(per) else _dirichlet_walls(per)
    x, A, b, tmp, _ = _level1_case(n, nc, per, 7, bc, cyl=cyl, **MODES["pfmg"])
    ratio = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    its = _cycles_needed(n, nc, per, 7, bc, cyl=cyl)
    print("level-1 pfmg", n, per, "cyl" if cyl else "xy", "|r|/|b| = %.3e" % ratio,
          "device iterations", its)
    assert ratio <= 1e-6


@pytest.mark.parametrize("mode", ["direct", "pfmg"])
def test_level1_fully_periodic_helmholtz(mode):
    """8 x 8 periodic in both dimensions with lambda = 50 (the
    photoionization modes): against numpy.linalg.solve."""
    x, A, b, tmp, (af, got) = _level1_case((8, 8), 8, (True, True), 9, DIRY, lam=50.0,
                                           **MODES[mode])
    ref = np.linalg.solve(A, b)
    err = np.max(np.abs(x - ref)) / np.max(np.abs(ref))
    ratio = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print("fully periodic helmholtz", mode, "relative max error %.3e |r|/|b| %.3e" % (err, ratio))
    if mode == "direct":
        assert err <= 1e-12  # (a well-conditioned 64 x 64 system)
    else:
        assert ratio <= 1e-6
    assert np.array_equal(p2.wrap_ghosts(af, got, 1), got)


@pytest.mark.parametrize("mode", ["direct", "pfmg"])
def test_tables_follow_the_bc_types(mode):
    """The cached tables key on the bc types of the walled dimension: changing
    them between two solves changes the result as numpy says. The periodic
    dimension's entries enter nothing: changing them changes nothing, bit for
    bit. (PFMG gets 200 iterations: this is about the operator it solves.)"""
    n, dr, per = (8, 16), p2.L1_DR, (True, False)
    af = AfTree(8, [n[d] * dr[d] for d in range(2)], list(n), periodic=per)
    tree, m = _mg_tree(af, DIRY, **dict(MODES[mode], coarse_cycles=0 if mode == "direct" else 200))
    rng = np.random.default_rng(2)
    phi, rhs = rng.standard_normal(tree.cc_shape), rng.standard_normal(tree.cc_shape)
    out = []
    xbc = [[(capi.BC_NEUMANN, 0.0)] * 2, [(capi.BC_DIRICHLET, 3.0), (capi.BC_NEUMANN, -2.0)],
           [(capi.BC_DIRICHLET, 0.0)] * 2]
    ybc = [DIRY[2:], [(capi.BC_DIRICHLET, 1.0), (capi.BC_NEUMANN, 0.25)]]
    for yb in ybc:
        for xb in xbc:
            bc = xb + yb
            tree.set_cc_methods(I_PHI, bc, capi.RB_MG_SIDES)
            tree.put_cc(I_PHI, phi)
            tree.put_cc(I_RHS, rhs)
            m.fas_vcycle(True, 1)
            got = tree.get_cc(I_PHI)
            x = p2.gather_level1(af, got).reshape(-1)
            A, fold = p2.level1_operator(n, dr, per, bc)
            b = fold(p2.gather_level1(af, rhs))
            assert np.linalg.norm(b - A @ x) <= 1e-6 * np.linalg.norm(b), (mode, bc)
            out.append(got)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    assert np.array_equal(out[3], out[4]) and np.array_equal(out[3], out[5])
    assert not np.array_equal(out[0], out[3])
    tree.close()


@pytest.mark.parametrize("side", [0, 1])
def test_electrode_row_at_the_seam(side):
    """A level-1 box next to the seam (12 x 8 would be no power of two: 16 x 8
    cells, nc = 4, four boxes across; side 0: the first box, whose low-x
    entries wrap; side 1: the last) with a random diagonally dominant
    v(5, nc, nc) and a bc_correction: PFMG's stopping rule holds against the
    numpy operator assembled from v with the wrap."""
    n, nc, per = (16, 8), 4, (True, False)
    af = AfTree(nc, [n[d] * p2.L1_DR[d] for d in range(2)], list(n), periodic=per)
    box = next(b for b in af.lvls[1]["ids"]
               if af.ix[b][0] == (1 if side == 0 else 4) and af.ix[b][1] == 2)
    rng = np.random.default_rng(21 + side)
    v = np.zeros((nc, nc, 5))
    v[..., 1:] = (0.5 + rng.random((nc, nc, 4))) / p2.L1_DR[0] ** 2
    v[..., 0] = -(v[..., 1:].sum(axis=-1)) * (1.0 + 0.2 * rng.random((nc, nc)))
    fb = rng.standard_normal((nc, nc)) * 50
    bc = _dirichlet_walls(per)
    x, A, b, tmp, _ = _level1_case(n, nc, per, 8, bc, stencil=(box, v, fb), **MODES["pfmg"])
    # the row of the box's seam cell reaches across the seam
    i0, j0 = (af.ix[box][0] - 1) * nc, (af.ix[box][1] - 1) * nc
    p = j0 * n[0] + (i0 if side == 0 else i0 + nc - 1)
    q = j0 * n[0] + (n[0] - 1 if side == 0 else 0)
    assert A[p, q] == v[0, 0 if side == 0 else nc - 1, 1 + side]
    ratio = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print("electrode row at the seam, side", side, "|r|/|b| = %.3e" % ratio)
    assert ratio <= 1e-6


# --------------------------------------------------------- whole field solve
@pytest.mark.parametrize("mode,pd,coord", [("direct", 0, AF_XYZ), ("pfmg", 0, AF_XYZ),
                                           ("pfmg", 1, AF_CYL)])
def test_vcycles_converge_on_P(mode, pd, coord):
    """V-cycles on P (three levels, refinement boundary through the seam):
    the residual after 10 is at most 1e-9 of the first. Also on the
    cylindrical Py (periodic z) with a Dirichlet wall at the outer radius."""
    P = p2.tree_P(pd=pd, coord=coord)
    bc = DIRY if pd == 0 else [(capi.BC_NEUMANN, 0.0), (capi.BC_DIRICHLET, 0.0)] * 2
    tree, m = _mg_tree(P, bc, **MODES[mode])
    rng = np.random.default_rng(11)
    tree.put_cc(I_PHI, rng.standard_normal(tree.cc_shape))
    tree.put_cc(I_RHS, rng.standard_normal(tree.cc_shape) * 1e6)
    r = [m.fas_vcycle_maxres() for _ in range(11)]
    tree.close()
    print("V-cycles on P", mode, "pd", pd, "coord", coord, "residuals", ["%.3e" % v for v in r])
    assert r[10] <= 1e-9 * r[0]


def _order_error(lvl, mode):
    L = 1.0
    af = AfTree(8, [L] * 2, [16] * 2, periodic=(True, False))
    af.refine_up_to_lvl(lvl)
    tree, m = _mg_tree(af, DIRY, **MODES[mode])
    rhs = np.zeros(tree.cc_shape)
    exact = np.zeros(tree.cc_shape)
    idx = np.arange(10) - 0.5
    for b in range(1, af.highest_id + 1):
        x = af.r_min[b][0] + idx * af.dr[b][0]
        y = af.r_min[b][1] + idx * af.dr[b][1]
        u = np.sin(np.pi * y / L)[:, None] * np.sin(2 * np.pi * x / L)[None, :]
        exact[b - 1] = u
        rhs[b - 1] = -(5 * np.pi ** 2 / L ** 2) * u   # lpl(phi) = rhs
    tree.put_cc(I_RHS, rhs)
    m.fas_fmg(True, have_guess=False)
    res = [m.fas_vcycle_maxres() for _ in range(12)]
    phi = tree.get_cc(I_PHI)
    tree.close()
    leaves = np.asarray(af.lvls[lvl]["ids"]) - 1
    inner = (slice(None),) + (slice(1, -1),) * 2
    return np.max(np.abs(phi[leaves][inner] - exact[leaves][inner])), res


@pytest.mark.parametrize("mode", ["direct", "pfmg"])
def test_second_order(mode):
    """lpl(phi) = f with phi = sin(2 pi x / L) sin(pi y / L), periodic in x,
    Dirichlet 0 in y, on uniform trees of 32^2 and 64^2 cells (FMG, then
    V-cycles to rounding): the max error falls by more than 3 per doubling
    (second order: 4 in the limit)."""
    e2, r2 = _order_error(2, mode)
    e3, r3 = _order_error(3, mode)
    print("order", mode, "errors %.4e %.4e ratio %.3f" % (e2, e3, e2 / e3), r3[-3:])
    assert r3[-1] < 1e-8 * 5 * np.pi ** 2  # (max |rhs| = 5 pi^2)
    assert e2 / e3 > 3.0


# ------------------------------------------- ghost cells and transfers, P / T
def _neu(pd):
    """Neumann in the periodic dimension's (unread) entries and on T's outer
    walls there, inhomogeneous Dirichlet walls in the other."""
    bc = [(capi.BC_NEUMANN, 0.0)] * 4
    bc[2 * (1 - pd)], bc[2 * (1 - pd) + 1] = (capi.BC_DIRICHLET, 1.5), (capi.BC_DIRICHLET, -0.5)
    return bc


def _same_centre(P, T, pd, a, b, what, ids=None):
    m = p2.box_map(P, T, pd)
    for p in (ids if ids is not None else m):
        assert np.array_equal(a[p - 1], b[m[p] - 1], equal_nan=True), (what, p2.box_key(P, p))


TWINS = [(0, AF_XYZ), (1, AF_XYZ), (1, AF_CYL)]


@pytest.mark.parametrize("pd,coord", TWINS)
@pytest.mark.parametrize("rb", [capi.RB_GC_INTERP, capi.RB_GC_INTERP_LIM, capi.RB_MG_SIDES])
def test_gc_tree_and_restrict_equal_the_twin(rb, pd, coord):
    """afh_gc_tree (with and without corners) and afh_restrict_tree on P
    against the twin's centre tile, every cell of every box bitwise."""
    P, T = p2.tree_P(pd=pd, coord=coord), p2.tree_T(pd=pd, coord=coord)
    tp, tt = _bare_tree(P, 1), _bare_tree(T, 1)
    ap, at = p2.fill_by_location(P, T, np.random.default_rng(3), pd)
    for corners in (False, True):
        out = []
        for tree, a in ((tp, ap), (tt, at)):
            tree.set_cc_methods(1, _neu(pd), rb)
            tree.put_cc(1, a)
            tree.gc_tree(1, corners)
            out.append(tree.get_cc(1))
        assert not np.array_equal(out[0], ap)
        _same_centre(P, T, pd, out[0], out[1], ("gc_tree", rb, corners))
    out = []
    for tree, a in ((tp, ap), (tt, at)):
        tree.put_cc(1, a)
        tree.restrict_tree(1)
        tree.gc_tree(1, True)
        out.append(tree.get_cc(1))
    _same_centre(P, T, pd, out[0], out[1], ("restrict_tree", rb))
    assert p2.check_seam_ghosts(P, out[0], "gc_tree") > 0
    tp.close(), tt.close()


@pytest.mark.parametrize("pd,coord", TWINS)
@pytest.mark.parametrize("method", [capi.PROLONG_LINEAR, capi.PROLONG_LIMIT])
def test_regrid_equals_the_twin(method, pd, coord):
    """afh_tree_regrid from two levels to three (new boxes prolonged from
    parents whose ghost cells came by wrap; their own ghost cells filled,
    corners included)."""
    P, T = p2.tree_P(levels=2, pd=pd, coord=coord), p2.tree_T(levels=2, pd=pd, coord=coord)
    tp, tt = _bare_tree(P, 1), _bare_tree(T, 1)
    ap, at = p2.fill_by_location(P, T, np.random.default_rng(4), pd)
    for tree, a in ((tp, ap), (tt, at)):
        tree.set_cc_methods(1, _neu(pd), capi.RB_GC_INTERP_LIM)
        tree.set_cc_prolong(1, method)
        tree.put_cc(1, a)
        tree.restrict_tree(1)
        tree.gc_tree(1, True)
    p2.grow(P, pd, 3), p2.grow(T, pd, 3)
    assert P.highest_lvl == 3 and P.highest_id > ap.shape[0]
    np_, nt = tp.regrid(P.topology()), tt.regrid(T.topology())
    assert np_.coord == tp.coord
    _same_centre(P, T, pd, np_.get_cc(1), nt.get_cc(1), ("regrid", method))
    for t in (np_, nt, tp, tt):
        t.close()


# ------------------------------------------------------------- species step
PFMG = MODES["pfmg"]


def _sim(af, case_name, n_ions=None):
    """The case's model bound to the tree `af`."""
    import golden
    from afh.driver import Simulation
    case = dict(golden.load(case_name))
    case["periodic"] = np.array([int(p) for p in af.periodic])
    sim = Simulation(_lib(), case, device=0, **PFMG)
    assert sim.cylindrical == (af.coord == AF_CYL)
    sim.af = af
    if n_ions is not None:
        assert len(sim.ions) >= n_ions
        sim.ions = sim.ions[:n_ions]
    sim._bind(sim._create_tree())
    return sim


def _species_state(sim, arrays):
    """Densities (both states), |E| and the face field from box arrays by
    location."""
    k = 0
    for iv in sim.densities:
        for s in (0, 1):
            sim.tree.put_cc(iv + s, arrays[k])
            k += 1
    sim.tree.put_cc(sim.i_efld, arrays[k])
    sim.tree.put_fc(sim.f_field, arrays[k + 1])


def _heun(sim, arrays):
    """Heun's two stages, each from the state put by location."""
    lims = [sim.fluid.forward_euler(1e-12, 0, [0], [1.0], 1, False)]
    out = [sim.tree.get_cc(iv + 1) for iv in sim.densities]
    _species_state(sim, arrays)
    lims.append(sim.fluid.forward_euler(5e-13, 1, [0, 1], [0.5, 0.5], 0, True))
    return lims, out + [sim.tree.get_cc(iv) for iv in sim.densities]


@pytest.mark.parametrize("pd,coord,case,n_ions", [
    (0, AF_XYZ, "rtest_test_2d", None),
    (1, AF_CYL, "rtest_test_cyl", None),
    (1, AF_CYL, "rtest_test_cyl_ion_motion", 1),
])
def test_species_step_equals_the_twin(pd, coord, case, n_ions):
    """afh_fluid_forward_euler, Heun stages 1 and 2, on P against the twin
    whose every tile holds P's data: the centre tile's leaves and all limits
    (extremes over tiles of equal values) bitwise. Each stage starts from
    data put by location: the first stage's result differs next to T's outer
    walls, which P does not have. The face field is random per face, the same
    on both sides of a seam (a face belongs to two boxes)."""
    P, T = p2.tree_P(pd=pd, coord=coord), p2.tree_T(pd=pd, coord=coord)
    sp, st = _sim(P, case, n_ions), _sim(T, case, n_ions)
    if n_ions:
        assert len(sp.ions) == 1
    rng = np.random.default_rng(6)
    n = 2 * len(sp.densities)
    pairs = [p2.fill_by_location(P, T, rng, pd, scale=1e16, positive=True) for _ in range(n)]
    pairs.append(p2.fill_by_location(P, T, rng, pd, scale=2e6, positive=True))  # |E|
    nf = P.nc + 1
    fp, ft = p2.fill_by_location(P, T, rng, pd, scale=2e6, shape=(2, nf, nf))
    # a face shared by two boxes of a level holds one value: the high face of
    # a box takes its neighbour's low face (by wrap on P, by tile on T)
    for af, f in ((P, fp), (T, ft)):
        for b in p2.used(af):
            for d in range(2):
                o = af.neighbors[b][2 * d + 1]
                if o > 0:
                    if d == 0:
                        f[b - 1, 0, :, -1] = f[o - 1, 0, :, 0]
                    else:
                        f[b - 1, 1, -1, :] = f[o - 1, 1, 0, :]
    pairs.append((fp, ft))
    _species_state(sp, [a for a, _ in pairs])
    _species_state(st, [b for _, b in pairs])
    lp, dp = _heun(sp, [a for a, _ in pairs])
    lt, dt = _heun(st, [b for _, b in pairs])
    print("limits P", lp, "T", lt)
    assert lp == lt
    inner = (slice(1, -1),) * 2
    m = p2.box_map(P, T, pd)
    for a, b in zip(dp, dt):
        for p in P.leaves():
            assert np.array_equal(a[p - 1][inner], b[m[p] - 1][inner]), p2.box_key(P, p)
    assert not np.array_equal(dp[0], pairs[0][0])
    sp.tree.close(), st.tree.close()


def test_species_step_equals_the_reference():
    """The device step on P against the reference's forward_euler with
    periodic = T F (tests/golden/replay_periodic2d.npz): the densities of
    both Heun stages and dt_lim, bitwise."""
    import state_periodic2d as sp
    sp.replay_against_reference(_lib(), 0)


# ----------------------------------------------------------------- smoothers
@pytest.mark.parametrize("nc", [8, 4, 16, 6, 12])
def test_down_leg_equals_the_twin(nc, monkeypatch):
    """One V-cycle's down leg on P against the twin, with the fused pair
    (k2_pair_box) and with AFH_PAIR2D=0 (the split half-sweeps). fas_vcycle
    without the residual pass leaves on every parent the rhs its children's
    smoothing gave it (L phi + the restricted residual, phi the restricted
    phi after the sweeps): the smoothing of levels 3 and 2 as level 2's and
    level 1's rhs, bitwise on the centre tile; both launch forms agree too.
    (The up leg follows the level-1 solve, which sees T's outer walls.)"""
    P, T = p2.tree_P(nc), p2.tree_T(nc)
    rng = np.random.default_rng(12)
    pp, pt = p2.fill_by_location(P, T, rng)
    rp, rt = p2.fill_by_location(P, T, rng, scale=1e6)
    parents = [b for b in p2.used(P) if P.has_children(b)]
    assert {P.lvl[b] for b in parents} == {1, 2}
    res = {}
    for pair in ("1", "0"):
        monkeypatch.setenv("AFH_PAIR2D", pair)
        out = []
        for af, phi, rhs in ((P, pp, rp), (T, pt, rt)):
            tree, m = _mg_tree(af, _neu(0), **MODES["direct"])
            tree.put_cc(I_PHI, phi)
            tree.put_cc(I_RHS, rhs)
            m.fas_vcycle(False)
            out.append(tree.get_cc(I_RHS)[:, 1:-1, 1:-1])
            tree.close()
        _same_centre(P, T, 0, out[0], out[1], ("down leg", nc, pair), parents)
        res[pair] = out[0]
    ix = np.asarray(parents) - 1
    assert np.array_equal(res["1"][ix], res["0"][ix])
    assert not np.array_equal(res["1"][ix], rp[ix][:, 1:-1, 1:-1])


# -------------------------------------------------------------------- driver
def _count_regrids(sim):
    regrids = []
    orig = sim.adjust_refinement

    def counted():
        info = orig()
        regrids.append((sim.it, info.n_add, info.n_rm))
        return info

    sim.adjust_refinement = counted
    return regrids


def _seam_check(sim):
    deep = 0
    for iv in sim.densities:
        sim.tree.restrict_tree(iv)
        sim.tree.gc_tree(iv)
        deep += p2.check_seam_ghosts(sim.af, sim.tree.get_cc(iv), sim.cc_names[iv - 1])
    rows = [sim.regression_row()] + list(sim.log)
    assert all(np.all(np.isfinite(r)) for r in rows)
    return deep


def test_driver_periodic_x():
    """Simulation on rtest_test_2d with periodic = [1, 0]: the initial
    refinement, ten steps, and on (at most 120) until a regrid inside the
    time loop has changed the tree; then every density's face ghost cells
    across the seam are the neighbour's interior, the log rows are finite,
    and a refined box has a same-level neighbour by wrap."""
    import golden
    from afh.driver import Simulation
    case = dict(golden.load("rtest_test_2d"))
    case["periodic"] = np.array([1, 0])
    sim = Simulation(_lib(), case, device=0, **PFMG)
    regrids = _count_regrids(sim)
    sim.start()
    for _ in range(10):
        assert sim.step()
    while not any(it > 0 and (n_add or n_rm) for it, n_add, n_rm in regrids) and sim.it < 120:
        assert sim.step()
    print("periodic 2-D driver: boxes", sim.af.highest_id, "levels", sim.af.highest_lvl,
          "steps", sim.it, "regrids (step, added, removed)", regrids)
    assert any(it == 0 and n_add for it, n_add, _ in regrids)
    assert any(it > 0 and (n_add or n_rm) for it, n_add, n_rm in regrids)
    assert _seam_check(sim) > 0
    sim.tree.close()


def test_driver_cylindrical_periodic_z():
    """rtest_test_cyl with periodic = [0, 1], ten steps, the same seam
    check. The case's only Dirichlet walls are the two z walls
    (field_bc_homogeneous), which a periodic z takes away: with Neumann walls
    in r alone the Poisson problem is singular (out of scope, as the fully
    periodic one) and the initial field computation does not converge. The
    run here grounds the outer cylinder instead (Dirichlet 0 at r = R), which
    is what a periodic coaxial set-up has."""
    import golden
    from afh.driver import Simulation
    case = dict(golden.load("rtest_test_cyl"))
    case["periodic"] = np.array([0, 1])
    sim = Simulation(_lib(), case, device=0, **PFMG)
    sim.phi_bc = lambda: [(capi.BC_NEUMANN, 0.0), (capi.BC_DIRICHLET, 0.0),
                          (capi.BC_DIRICHLET, 0.0), (capi.BC_DIRICHLET, sim.voltage)]
    sim.start()
    assert sim.tree.coord == capi.COORD_CYL and sim.af.periodic == (False, True)
    for _ in range(10):
        assert sim.step()
    print("periodic cylindrical driver: boxes", sim.af.highest_id, "levels", sim.af.highest_lvl,
          "steps", sim.it)
    assert _seam_check(sim) > 0
    sim.tree.close()

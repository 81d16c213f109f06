"""Periodic domains in the 2-D library, host side: the trees the GPU tests
run on (tests/periodic2d_numpy.py), the flags' way from AfTree and the driver
to the library, and the host code of the two level-1 solves -- the PFMG set-up
as the 2-D library calls it and the periodic AFH_COARSE_DIRECT tables --
through probes compiled from the library's own headers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import periodic2d_numpy as p2
import periodic_numpy as pn
from afh import capi
from afh.amr import AF_CYL, AF_XYZ, NO_BOX, AfTree
from afh.model import tree_desc

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------- trees
@pytest.mark.parametrize("pd", [0, 1])
def test_tree_P_properties(pd):
    """P (pd = 0) and Py (pd = 1): a level-1 box is its own neighbour in the
    periodic dimension; same-level wrap on every level; a refinement boundary
    across the seam on level 3; a level-1 box refined by the balance alone."""
    t = p2.tree_P(pd=pd)
    od = 1 - pd
    assert t.highest_lvl == 3 and t.periodic == p2.periodic_of(pd)
    assert t.coarse_grid_size[pd] == 8 and t.coarse_grid_size[od] == 16
    for b in t.lvls[1]["ids"]:
        assert t.neighbors[b][2 * pd] == b and t.neighbors[b][2 * pd + 1] == b
        assert (t.neighbors[b][2 * od] < 0) != (t.neighbors[b][2 * od + 1] < 0)
        assert t.has_children(b)
    seams = p2.seam_faces(t)
    for lvl in (1, 2, 3):
        assert any(t.lvl[b] == lvl for b, _, _ in seams), lvl
    # level 3, rows 3 and 4 (of the walled dimension): half the width; across
    # the seam lies a level-2 leaf
    edge = [b for b in t.lvls[3]["ids"] if t.ix[b][od] == 3 and t.ix[b][pd] == 1]
    assert len(edge) == 1 and t.neighbors[edge[0]][2 * pd] == NO_BOX
    across = t.neighbors[t.parent[edge[0]]][2 * pd]
    assert across > NO_BOX and t.ix[across][pd] == 2 and not t.has_children(across)
    # 2:1 everywhere, the seam included
    for lvl in (2, 3):
        for b in t.lvls[lvl]["ids"]:
            for nb in range(4):
                if t.neighbors[b][nb] == NO_BOX:
                    assert t.neighbors[t.parent[b]][nb] > NO_BOX


@pytest.mark.parametrize("pd,coord", [(0, AF_XYZ), (1, AF_XYZ), (1, AF_CYL)])
def test_twin_centre_tile_matches_P(pd, coord):
    """T's centre tile has P's boxes, each with the neighbours P reaches by
    wrap (same level and place within the tile, or none) and the same
    corners and spacings bit for bit."""
    P, T = p2.tree_P(pd=pd, coord=coord), p2.tree_T(pd=pd, coord=coord)
    assert T.periodic == (False, False) and T.coarse_grid_size[pd] == 24
    m = p2.box_map(P, T, pd)
    assert len(m) == sum(P.in_use)
    for b, c in m.items():
        assert np.array_equal(P.dr[b], T.dr[c]) and np.array_equal(P.r_min[b], T.r_min[c])
        assert P.has_children(b) == T.has_children(c)
        for nb in range(4):
            p, q = P.neighbors[b][nb], T.neighbors[c][nb]
            if p <= NO_BOX:
                assert q == p, (b, nb)
            else:
                assert p2._tile_key(T, q, pd) == p2.box_key(P, p)
    W = p2.walled_like(P, pd)
    assert W.highest_id == P.highest_id


# ------------------------------------------------------------- flags' way
def test_tree_desc_carries_both_flags():
    for per in ((True, False), (False, True), (True, True)):
        t = AfTree(8, [1.0, 1.0], [8, 16], periodic=per)
        d, _keep = tree_desc(t.topology(), 1, 0)
        assert list(d.periodic) == [int(per[0]), int(per[1]), 0]
    with pytest.raises(ValueError, match="cylindrical"):
        AfTree(8, [1.0, 1.0], [8, 16], periodic=(True, False), coord=AF_CYL)
    AfTree(8, [1.0, 1.0], [8, 16], periodic=(False, True), coord=AF_CYL)


def test_driver_reads_the_2d_entry():
    """The 2-D driver takes a `periodic` entry (it raised NotImplementedError
    before the 2-D level-1 solves wrapped); a wrong count and a sharded run
    keep raising."""
    import golden
    from afh.driver import Simulation
    lib = capi.hip_library_2d()
    case = dict(golden.load("rtest_test_2d"))
    assert Simulation(lib, case).af.periodic == (False, False)
    case["periodic"] = np.array([1, 0])
    sim = Simulation(lib, case)
    assert sim.periodic == (True, False) and sim.af.periodic == (True, False)
    assert list(tree_desc(sim.af.topology(), 1, 0)[0].periodic) == [1, 0, 0]
    with pytest.raises(NotImplementedError, match="sharded"):
        sim.shard_over(None)
    case["periodic"] = np.array([1, 1, 0])
    with pytest.raises(ValueError, match="periodic"):
        Simulation(lib, case)
    cyl = dict(golden.load("rtest_test_cyl"))
    cyl["periodic"] = np.array([0, 1])
    pf = dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
    assert Simulation(lib, cyl, **pf).af.periodic == (False, True)
    cyl["periodic"] = np.array([1, 0])
    with pytest.raises(ValueError, match="cylindrical"):
        Simulation(lib, cyl, **pf)


# ------------------------------------------------------------------ probes
def _compile(tmp_path_factory, name):
    exe = str(tmp_path_factory.mktemp(name) / name)
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed for the host probes"
    subprocess.run([cc, "-O1", "-ffp-contract=off", "-o", exe,
                    os.path.join(HERE, name + ".c"), "-lm"], check=True)
    return exe


@pytest.fixture(scope="module")
def cs_tables_probe(tmp_path_factory):
    exe = _compile(tmp_path_factory, "cs_tables_probe")

    def run(n, bc_lo, bc_hi, periodic, h):
        out = subprocess.run([exe, str(n), str(bc_lo), str(bc_hi), str(int(periodic)), repr(h)],
                             capture_output=True, check=True).stdout
        a = np.frombuffer(out, np.float64)
        return a[:n * n].reshape(n, n), a[n * n:]
    return run


@pytest.mark.parametrize("n", [2, 4, 7, 8, 12, 16])
def test_periodic_cs_tables_diagonalise_the_circulant(n, cs_tables_probe):
    """afh2_cs_tables' periodic form against the dense circulant
    C = h tridiag(1, -2, 1) + corners (2 points: the one neighbour twice):
    Q orthogonal to 1e-14, Q^T C Q = diag(e) to 1e-12 |e|max; the bc types do
    not enter."""
    h = 2.0 ** 20
    Cm = np.zeros((n, n))
    for i in range(n):
        Cm[i, i] -= 2 * h
        Cm[i, (i - 1) % n] += h
        Cm[i, (i + 1) % n] += h
    q, e = cs_tables_probe(n, p2.BC_DIRICHLET, p2.BC_NEUMANN, 1, h)
    assert np.max(np.abs(q.T @ q - np.eye(n))) <= 1e-14
    assert np.max(np.abs(q.T @ Cm @ q - np.diag(e))) <= 1e-12 * np.max(np.abs(e))
    k = np.arange(n)
    assert np.allclose(np.sort(e), np.sort(h * (2 * np.cos(2 * np.pi * k / n) - 2)),
                       rtol=0, atol=1e-12 * 4 * h)
    for lo, hi in ((p2.BC_NEUMANN, p2.BC_NEUMANN), (p2.BC_DIRICHLET, p2.BC_DIRICHLET)):
        q2, e2 = cs_tables_probe(n, lo, hi, 1, h)
        assert np.array_equal(q, q2) and np.array_equal(e, e2)


@pytest.mark.parametrize("lo,hi", [(-10, -10), (-10, -11), (-11, -10), (-11, -11)])
def test_walled_cs_tables_diagonalise_the_folded_operator(lo, hi, cs_tables_probe):
    """The form without the flag (the cosine / sine tables, unchanged): the
    folded tridiagonal operator with end diagonals -3h (Dirichlet) / -h
    (Neumann)."""
    n, h = 8, 3.0
    T = np.zeros((n, n))
    for i in range(n):
        T[i, i] = -2 * h
        if i > 0:
            T[i, i - 1] = h
        if i < n - 1:
            T[i, i + 1] = h
    T[0, 0] += -h if lo == p2.BC_DIRICHLET else h
    T[-1, -1] += -h if hi == p2.BC_DIRICHLET else h
    q, e = cs_tables_probe(n, lo, hi, 0, h)
    assert np.max(np.abs(q.T @ q - np.eye(n))) <= 1e-14
    assert np.max(np.abs(q.T @ T @ q - np.diag(e))) <= 1e-12 * 4 * h


@pytest.fixture(scope="module")
def pfmg_probe2d(tmp_path_factory):
    exe = _compile(tmp_path_factory, "pfmg_probe2d")

    def run(n, per, a7):
        out = subprocess.run([exe, str(n[0]), str(n[1]), str(int(per[0])), str(int(per[1]))],
                             input=np.ascontiguousarray(a7).tobytes(), capture_output=True,
                             check=True).stdout
        nl = int(np.frombuffer(out, np.int32, 1)[0])
        o = 4
        nn = np.frombuffer(out, np.int32, 3 * nl, o).reshape(nl, 3)
        o += 12 * nl
        cdir = np.frombuffer(out, np.int32, nl, o)
        active = np.frombuffer(out, np.int32, nl, o + 4 * nl)
        o += 8 * nl
        w = np.frombuffer(out, np.float64, nl, o)
        o += 8 * nl
        npts = int(sum(np.prod(v) for v in nn))
        A = np.frombuffer(out, np.float64, 27 * npts, o).reshape(npts, 27)
        P = np.frombuffer(out, np.float64, 2 * npts, o + 8 * 27 * npts).reshape(npts, 2)
        return nn, cdir, active, w, A, P
    return run


def _walls(per, lo=2.0, hi=-1.0):
    """Dirichlet walls in the dimension that is not periodic (both when none
    is), Neumann entries elsewhere."""
    bc = [(p2.BC_NEUMANN, 0.5)] * 4
    for d in range(2):
        if not per[d]:
            bc[2 * d], bc[2 * d + 1] = (p2.BC_DIRICHLET, lo), (p2.BC_DIRICHLET, hi)
            if any(per):
                break
    return bc


# (n, periodic, cylindrical, lambda): the grids of the GPU stopping-rule test
# and the fully periodic Helmholtz grid
PFMG_GRIDS = [
    ((8, 16), (True, False), False, 0.0),
    ((4, 4), (True, False), False, 0.0),     # the 2-point and 1-point periodic levels
    ((8, 4), (False, True), False, 0.0),
    ((8, 16), (False, False), False, 0.0),   # the same statement of today's set-up
    ((8, 16), (False, True), True, 0.0),     # cylindrical, periodic z
    ((8, 8), (True, True), False, 50.0),
]


def _hierarchy(n, per, cyl, lam, probe):
    dr = p2.L1_DR
    per3, n3 = tuple(per) + (False,), (n[0], n[1], 1)
    a7, A0 = p2.level1_a7(n, dr, per, _walls(per), lam, cyl)
    nn, cdir, active, w, A, P = probe(n, per, a7)
    off = np.concatenate([[0], np.cumsum([np.prod(v) for v in nn])]).astype(int)
    M = [pn.pfmg_dense(nn[l], A[off[l]:off[l + 1]], per3) for l in range(len(nn))]
    Pm = [pn.pfmg_interp(nn[l], nn[l + 1], int(cdir[l]), P[off[l]:off[l + 1]], per3)
          for l in range(len(nn) - 1)]
    return dict(nn=nn, cdir=cdir, active=active, w=w, A=A, P=P, off=off, M=M, Pm=Pm,
                A0=A0, n3=n3)


@pytest.mark.parametrize("n,per,cyl,lam", PFMG_GRIDS)
def test_pfmg2d_periodic_setup_is_galerkin(n, per, cyl, lam, pfmg_probe2d):
    """afh_pfmg_setup_per with ndim = 2 against an independent dense
    statement: level 0 is the wrapped operator; every odd point's weights are
    -(row sum toward that side) / (row sum of the rest) along the coarsening
    direction; every coarse operator is P^T A P with the dense wrapped
    interpolation, through the 2-point level down to 1 point. Bound: 1e-14 of
    the finer operator's largest entry (sums of at most 3 x 9 x 3 products of
    its entries with weights of at most 1 in double; with lambda > 0 on the
    fully periodic grid the coarse entries are what is left after those
    cancel)."""
    H = _hierarchy(n, per, cyl, lam, pfmg_probe2d)
    nn, off, M = H["nn"], H["off"], H["M"]
    assert [int(v) for v in nn[-1]] == [1, 1, 1]
    assert np.max(np.abs(M[0] - H["A0"])) <= 1e-15 * np.max(np.abs(H["A0"]))
    folds = 0
    for l in range(len(nn) - 1):
        cd = int(H["cdir"][l])
        assert cd in (0, 1)
        Pl = H["P"][off[l]:off[l + 1]]
        nf = [int(v) for v in nn[l]]
        for p in range(M[l].shape[0]):
            q = [p % nf[0], (p // nf[0]) % nf[1], 0]
            if q[cd] % 2:  # (0-based odd = an even point: coarse)
                assert Pl[p, 0] == 0 and Pl[p, 1] == 0
                continue
            A27 = H["A"][off[l] + p]
            side = np.array([[s % 3, (s // 3) % 3, s // 9][cd] - 1 for s in range(27)])
            c, lo, hi = A27[side == 0].sum(), -A27[side == -1].sum(), -A27[side == 1].sum()
            assert np.allclose([Pl[p, 0], Pl[p, 1]], [lo / c, hi / c], rtol=1e-14, atol=0)
        G = H["Pm"][l].T @ M[l] @ H["Pm"][l]
        assert np.max(np.abs(G - M[l + 1])) <= 1e-14 * np.max(np.abs(M[l])), l
        folds += per[cd] and nf[cd] == 2
    assert folds == sum(per)


def pfmg_cycle_count(H, b, x, tol=1e-6, max_iter=50):
    """The solve of afh_pfmg.h's header restated on the dense levels:
    weighted Jacobi, r.r / b.b < tol^2 checked after the first relaxation of
    every iteration but the first. Returns (iterations, x)."""
    M, Pm, w, act = H["M"], H["Pm"], H["w"], H["active"]
    nl = len(M)
    D = [np.diag(m).copy() for m in M]

    def relax(l, xl, bl):
        return xl + w[l] * (bl - M[l] @ xl) / D[l]
    bb = b @ b
    if bb == 0.0:
        return 0, np.zeros_like(b)
    it = 0
    for i in range(max_iter):
        x = relax(0, x, b)
        r = b - M[0] @ x
        it = i + 1
        if i > 0 and (r @ r) / bb < tol * tol:
            it = i
            break
        xs, bs = [None] * nl, [None] * nl
        bs[1] = Pm[0].T @ r
        for l in range(1, nl - 1):
            if act[l]:
                xs[l] = w[l] * bs[l] / D[l]
                rl = bs[l] - M[l] @ xs[l]
            else:
                xs[l] = np.zeros_like(bs[l])
                rl = bs[l]
            bs[l + 1] = Pm[l].T @ rl
        xs[nl - 1] = bs[nl - 1] / D[nl - 1]
        for l in range(nl - 2, 0, -1):
            xs[l] = xs[l] + Pm[l] @ xs[l + 1]
            if act[l]:
                xs[l] = relax(l, xs[l], bs[l])
        x = x + Pm[0] @ xs[1]
        x = relax(0, x, b)
    return it, x


@pytest.mark.parametrize("n,per,cyl,lam", PFMG_GRIDS)
def test_pfmg2d_cycle_needs_at_most_50_iterations(n, per, cyl, lam, pfmg_probe2d):
    """The grids of the GPU stopping-rule test, chosen here before any
    device run: the host set-up and this numpy restatement of the cycle reach
    |r| <= 1e-6 |b| within PFMG's 50 iterations from a random guess, with
    room to spare (the device count may differ by a few: its sums run in
    another order)."""
    H = _hierarchy(n, per, cyl, lam, pfmg_probe2d)
    rng = np.random.default_rng(7)
    N = n[0] * n[1]
    x0, b = rng.standard_normal(N), rng.standard_normal(N) * 100
    it, x = pfmg_cycle_count(H, b, x0)
    ratio = np.linalg.norm(b - H["M"][0] @ x) / np.linalg.norm(b)
    print("numpy PFMG cycle", n, per, "cyl" if cyl else "xy", "lambda", lam,
          "iterations", it, "|r|/|b| %.3e" % ratio, "cdir", list(H["cdir"][:-1]),
          "active", list(H["active"]))
    assert it <= 40 and ratio <= 1e-6


def test_level1_operator_rows():
    """The wrapped 2-D operator: symmetric (Cartesian), zero row sums away
    from the Dirichlet walls, the 2-point line's neighbour entered twice; the
    cylindrical rows sum to zero too and weight r's neighbours."""
    dr = (0.5, 0.25)
    bc = [(p2.BC_NEUMANN, 0.0)] * 2 + [(p2.BC_DIRICHLET, 1.0), (p2.BC_DIRICHLET, 2.0)]
    A, fold = p2.level1_operator((2, 4), dr, (True, False), bc)
    assert np.array_equal(A, A.T)
    rows = A.sum(axis=1).reshape(4, 2)
    assert np.allclose(rows[1:-1], 0.0)
    assert np.allclose(rows[0], -2 / dr[1] ** 2) and np.allclose(rows[-1], -2 / dr[1] ** 2)
    assert A[0, 1] == 2 / dr[0] ** 2
    f = fold(np.zeros((4, 2))).reshape(4, 2)
    assert np.all(f[0] == -2 / dr[1] ** 2 * 1.0) and np.all(f[-1] == -2 / dr[1] ** 2 * 2.0)
    bc = [(p2.BC_NEUMANN, 0.0)] * 4
    A, _ = p2.level1_operator((4, 4), dr, (False, True), bc, cyl=True)
    assert np.allclose(A.sum(axis=1), 0.0, atol=1e-12)
    assert A[0, 1] == pytest.approx(2 / dr[0] ** 2) and A[1, 0] == pytest.approx(2 / 3 / dr[0] ** 2)
    assert A[0, 12] == 1 / dr[1] ** 2  # z wraps


def test_replay_fixture_belongs_to_the_state():
    """tests/golden/replay_periodic2d.npz holds data only -- the leaves, both
    stages' densities on their interiors and dt_lim -- and belongs to the
    state tests/state_periodic2d.py builds now."""
    import golden
    import state_periodic2d as sp
    c, af, cc, fc = sp.build_state()
    fx = golden.load("replay_periodic2d")
    assert sorted(fx.keys()) == ["dens_1", "dens_2", "dt_lim_1", "dt_lim_2", "leaves"]
    assert list(fx["leaves"]) == af.leaves()
    n = len(c.ia("all_densities"))
    for k in (1, 2):
        assert fx["dens_%d" % k].shape == (n, len(af.leaves()), af.nc, af.nc)
        assert np.all(np.isfinite(fx["dens_%d" % k])) and fx["dt_lim_%d" % k][0] < 1e-6
    # the state is periodic in x: the ghost cells across the seam hold the
    # neighbours' values to rounding
    for iv, a in cc.items():
        for b, nb, o in p2.seam_faces(af):
            if nb >= 2:
                continue
            g, i = (af.nc + 1, 1) if nb % 2 else (0, af.nc)
            assert np.allclose(a[b - 1][1:-1, g], a[o - 1][1:-1, i], rtol=1e-12, atol=0), (iv, b)

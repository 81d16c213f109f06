"""Periodic domains, host side: the trees the GPU tests run on
(tests/periodic_numpy.py), the flags' way from AfTree to the libraries, and
the numpy statement of the wrapped level-1 operator."""
import numpy as np
import pytest

import periodic_numpy as pn
from afh import capi
from afh.amr import NO_BOX, AfTree
from afh.model import Tree, tree_desc


def _wrapped(t, b, nb):
    """Whether box b's same-level neighbour nb is reached across a seam."""
    o = t.neighbors[b][nb]
    if o <= NO_BOX:
        return False
    d, up = nb // 2, nb % 2
    return (t.ix[o][d] > t.ix[b][d]) != bool(up) or o == b


def test_tree_P_properties():
    """P: a self-neighbour in x, the same box on both sides in y, physical
    walls in z; same-level wrap on every level; a refinement boundary across
    the y seam; and a box refined by the 2:1 balance across the seam alone."""
    t = pn.tree_P()
    assert t.highest_lvl == 3
    assert t.coarse_grid_size == [8, 16, 16] and t.periodic == (True, True, False)
    for b in t.lvls[1]["ids"]:
        assert t.neighbors[b][0] == b and t.neighbors[b][1] == b       # x: itself
        assert t.neighbors[b][2] == t.neighbors[b][3] not in (b, NO_BOX)  # y: one box twice
        assert (t.neighbors[b][4] < 0) != (t.neighbors[b][5] < 0)      # z: one wall each
    for lvl in (1, 2, 3):
        assert any(_wrapped(t, b, nb) for b in t.lvls[lvl]["ids"] for nb in range(4)), lvl
    # level 3 sits under the y seam (top of the level-2 grid of 4 boxes in y):
    # across it lies a level-2 leaf -- a refinement boundary through the seam
    top = [b for b in t.lvls[3]["ids"] if t.ix[b][1] == 8]
    assert top and all(t.neighbors[b][3] == NO_BOX for b in top)
    across = t.neighbors[t.parent[top[0]]][3]
    assert across > NO_BOX and t.ix[across][1] == 1 and not t.has_children(across)
    # nobody asked for the level-1 boxes with ix(2) = 1: the balance did
    lo = [b for b in t.lvls[1]["ids"] if t.ix[b] == (1, 1, 1)]
    assert len(lo) == 1 and t.has_children(lo[0])
    other = [b for b in t.lvls[1]["ids"] if t.ix[b] == (1, 1, 2)]
    assert not t.has_children(other[0])
    # 2:1 everywhere, seams included: a leaf's missing neighbour has a parent-level one
    for lvl in (2, 3):
        for b in t.lvls[lvl]["ids"]:
            for nb in range(6):
                if t.neighbors[b][nb] == NO_BOX:
                    assert t.neighbors[t.parent[b]][nb] > NO_BOX


def test_twin_centre_tile_matches_P():
    """T's centre tile has P's boxes, and each has the neighbours P reaches
    by wrap (same level and place within the tile, or none)."""
    P, T = pn.tree_P(), pn.tree_T()
    assert T.periodic == (False,) * 3 and T.coarse_grid_size == [24, 48, 16]
    m = pn.box_map(P, T)
    assert len(m) == sum(P.in_use)
    for b, c in m.items():
        assert np.array_equal(P.dr[b], T.dr[c]) and np.array_equal(P.r_min[b], T.r_min[c])
        assert P.has_children(b) == T.has_children(c)
        for nb in range(6):
            p, q = P.neighbors[b][nb], T.neighbors[c][nb]
            if p <= NO_BOX:
                assert q == p, (b, nb)
                continue
            n = pn._boxes_per_dim((1, 1, 1), T.lvl[q])
            assert (T.lvl[q],) + tuple((T.ix[q][d] - 1) % n[d] + 1 for d in range(3)) == \
                pn.box_key(P, p)


def test_topology_carries_the_flags_to_the_hip_libraries_only():
    t = AfTree(8, [1.0] * 3, [8, 16, 8], periodic=(True, False, True))
    topo = t.topology()
    assert list(topo["periodic"]) == [1, 0, 1]
    d, _keep = tree_desc(topo, 1, 0)
    assert list(d.periodic) == [1, 0, 1]
    d, _keep = tree_desc(topo, 1, 0, periodic=False)
    assert list(d.periodic) == [0, 0, 0]
    t2 = AfTree(8, [1.0] * 2, [8, 16], periodic=(False, True))
    d, _keep = tree_desc(t2.topology(), 1, 0)
    assert list(d.periodic) == [0, 1, 0]
    # a topology from before the entry existed: nothing periodic
    topo.pop("periodic")
    d, _keep = tree_desc(topo, 1, 0)
    assert list(d.periodic) == [0, 0, 0]


def test_oracle_keeps_getting_zeros():
    """The C oracle refuses the flag; afh.model.Tree clears it there."""
    lib = capi.oracle_library()
    topo = pn.tree_P().topology()
    tree = Tree(lib, topo, 1, 0)
    tree.close()
    d, _keep = tree_desc(topo, 1, 0)
    import ctypes as C
    h = C.c_void_p()
    with pytest.raises(capi.AfhError, match="periodic"):
        lib.call("tree_create", C.byref(d), -1, C.byref(h))


def test_driver_reads_the_case_entry():
    import golden
    from afh.driver import Simulation
    lib = capi.oracle_library()
    case = dict(golden.load("rtest_test_3d"))
    assert Simulation(lib, case).af.periodic == (False,) * 3
    case["periodic"] = np.array([1, 1, 0])
    sim = Simulation(lib, case)
    assert sim.periodic == (True, True, False) and sim.af.periodic == (True, True, False)
    with pytest.raises(NotImplementedError, match="sharded"):
        sim.shard_over(None)
    case["periodic"] = np.array([1, 0])
    with pytest.raises(ValueError, match="periodic"):
        Simulation(lib, case)


@pytest.mark.parametrize("n", [2, 4, 7, 8])
def test_fourier_basis_diagonalises_the_circulant(n):
    """The table the direct solve is given for a periodic dimension, stated
    here in numpy: orthonormal, and Q^T C Q = diag(h (2 cos(2 pi m / n) - 2))
    for the circulant C = h tridiag(1, -2, 1) + corners (on 2 points the one
    neighbour twice)."""
    h = 3.0
    Cm = np.zeros((n, n))
    for i in range(n):
        Cm[i, i] -= 2 * h
        Cm[i, (i - 1) % n] += h
        Cm[i, (i + 1) % n] += h
    q, e = np.zeros((n, n)), np.zeros(n)
    for p in range(n):
        m = (p + 1) // 2
        th = 2 * np.pi * m / n
        i = np.arange(n)
        v = np.sin(th * i) if (p > 0 and p % 2 == 0) else np.cos(th * i)
        q[:, p] = v / np.sqrt(np.sum(v * v))
        e[p] = h * (2 * np.cos(th) - 2)
    assert np.allclose(q.T @ q, np.eye(n), atol=1e-14)
    assert np.allclose(q.T @ Cm @ q, np.diag(e), atol=1e-13 * h)


def test_level1_operator_rows():
    """The wrapped operator: zero row sums away from the Dirichlet walls
    (periodic faces fold nothing), symmetric, and the 2-point line's
    neighbour entered twice."""
    dr = (0.5, 0.25, 0.125)
    bc = [(pn.BC_NEUMANN, 0.0)] * 4 + [(pn.BC_DIRICHLET, 1.0), (pn.BC_DIRICHLET, 2.0)]
    A, fold = pn.level1_operator((2, 4, 4), dr, pn.PERIODIC, bc)
    assert np.array_equal(A, A.T)
    rows = A.sum(axis=1).reshape(4, 4, 2)
    assert np.allclose(rows[1:-1], 0.0)
    assert np.allclose(rows[0], -2 / dr[2] ** 2) and np.allclose(rows[-1], -2 / dr[2] ** 2)
    assert A[0, 1] == 2 / dr[0] ** 2
    f = fold(np.zeros((4, 4, 2))).reshape(4, 4, 2)
    assert np.all(f[0] == -2 / dr[2] ** 2 * 1.0) and np.all(f[-1] == -2 / dr[2] ** 2 * 2.0)
    assert np.all(f[1:-1] == 0.0)


def test_level1_apply_equals_the_dense_operator():
    dr = (0.5, 0.25, 0.125)
    bc = [(pn.BC_NEUMANN, 0.0), (pn.BC_DIRICHLET, 0.0)] * 3
    rng = np.random.default_rng(0)
    for per in ((True, True, False), (False, False, True), (False,) * 3):
        n = (2, 4, 6)
        A, _ = pn.level1_operator(n, dr, per, bc, lam=3.0)
        u = rng.standard_normal((n[2], n[1], n[0]))
        assert np.allclose(pn.level1_apply(u, dr, per, bc, 3.0).reshape(-1),
                           A @ u.reshape(-1), rtol=1e-13, atol=1e-12)


def test_oracle_species_step_equals_the_reference(monkeypatch):
    """The C oracle never sees the flag, only the wrapped neighbours: its
    species step on P equals the reference's forward_euler with
    periodic = T T F (tests/golden/replay_periodic.npz) bit for bit."""
    import state_periodic as sp
    sp.replay_against_reference(capi.oracle_library(), -1, monkeypatch)


@pytest.fixture(scope="module")
def pfmg_probe(tmp_path_factory):
    """tests/pfmg_probe.c compiled: afh_pfmg.h's host set-up on the CPU."""
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path_factory.mktemp("pfmg") / "pfmg_probe")
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler is needed for the PFMG set-up probe"
    subprocess.run([cc, "-O1", "-ffp-contract=off", "-o", exe,
                    os.path.join(here, "pfmg_probe.c"), "-lm"], check=True)

    def run(n, per, a7):
        out = subprocess.run([exe] + [str(v) for v in n] + [str(int(v)) for v in per],
                             input=np.ascontiguousarray(a7).tobytes(), capture_output=True,
                             check=True).stdout
        nl = int(np.frombuffer(out, np.int32, 1)[0])
        o = 4
        nn = np.frombuffer(out, np.int32, 3 * nl, o).reshape(nl, 3)
        o += 12 * nl
        cdir = np.frombuffer(out, np.int32, nl, o)
        o += 8 * nl  # (cdir, then active)
        o += 8 * nl  # (w)
        npts = int(sum(np.prod(v) for v in nn))
        A = np.frombuffer(out, np.float64, 27 * npts, o).reshape(npts, 27)
        P = np.frombuffer(out, np.float64, 2 * npts, o + 8 * 27 * npts).reshape(npts, 2)
        return nn, cdir, A, P
    return run


@pytest.mark.parametrize("n,per", [
    ((8, 16, 8), (True, True, False)),   # the GPU tests' grid
    ((4, 4, 4), (True, True, False)),
    ((4, 8, 4), (False, True, True)),
    ((4, 8, 2), (True, False, True)),    # a direction of 2 points from the start
    ((8, 8, 8), (False, False, False)),  # the same statement of today's set-up
])
def test_pfmg_periodic_setup_is_galerkin(n, per, pfmg_probe):
    """The periodic PFMG set-up (afh_pfmg_setup_per) against an independent
    dense statement: level 0 is the wrapped operator; every odd point's
    weights are -(row sum toward that side) / (row sum of the rest) of its
    dense row along the coarsening direction; every coarse operator is
    P^T A P with P the dense wrapped interpolation -- through the level of 2
    points (one coarse neighbour, twice) down to 1 point, where nothing of
    that direction is left beside the centre. Bound: 1e-14 of the largest
    entry (sums of at most 3 x 27 x 3 products in double precision)."""
    dr = (2.0 ** -3, 2.0 ** -4, 2.0 ** -3)
    d = per.index(False)
    bc = [(pn.BC_NEUMANN, 0.0)] * 6
    bc[2 * d] = bc[2 * d + 1] = (pn.BC_DIRICHLET, 0.0)
    a7, A0 = pn.level1_a7(n, dr, per, bc)
    nn, cdir, A, P = pfmg_probe(n, per, a7)
    assert [int(v) for v in nn[-1]] == [1, 1, 1]
    off = np.concatenate([[0], np.cumsum([np.prod(v) for v in nn])]).astype(int)
    M = [pn.pfmg_dense(nn[l], A[off[l]:off[l + 1]], per) for l in range(len(nn))]
    assert np.array_equal(M[0], A0)
    folds = 0
    for l in range(len(nn) - 1):
        cd = int(cdir[l])
        Pl = P[off[l]:off[l + 1]]
        Pm = pn.pfmg_interp(nn[l], nn[l + 1], cd, Pl, per)
        # the weights from the dense rows: entries by their (wrapped) step along cd
        nf = [int(v) for v in nn[l]]
        for p in range(M[l].shape[0]):
            q = [p % nf[0], (p // nf[0]) % nf[1], p // (nf[0] * nf[1])]
            if q[cd] % 2:  # (0-based odd = an even point: coarse)
                assert Pl[p, 0] == 0 and Pl[p, 1] == 0
                continue
            A27 = A[off[l] + p]
            side = np.array([[s % 3, (s // 3) % 3, s // 9][cd] - 1 for s in range(27)])
            c, lo, hi = A27[side == 0].sum(), -A27[side == -1].sum(), -A27[side == 1].sum()
            assert np.allclose([Pl[p, 0], Pl[p, 1]], [lo / c, hi / c], rtol=1e-14, atol=0)
        G = Pm.T @ M[l] @ Pm
        assert np.max(np.abs(G - M[l + 1])) <= 1e-14 * np.max(np.abs(M[l + 1])), l
        folds += per[cd] and nf[cd] == 2
    assert folds == sum(per)

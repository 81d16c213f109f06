"""Independent numpy statements for the 2-D periodic-domain tests, and the
trees those tests run on (the 2-D restatement of tests/periodic_numpy.py).

Every tree is periodic in one dimension ``pd`` (0: x, the trees P / T; 1: y,
the trees Py / Ty) and walled in the other. Box keys below are written for
pd = 0; for pd = 1 the two indices are swapped.

* ``tree_P``: level-1 grid nc x 2nc cells (1 x 2 boxes), periodic (T, F):
  a level-1 box is its own x neighbour. The level-1 box (1, 1) is refined,
  then the level-2 boxes (1, 1), (2, 1) and (1, 2): level 3 covers the whole
  width in its two lower rows (a level-3 box has a same-level neighbour by
  wrap) and half of it in the two rows above, where the level-3 box (1, 3)
  has the level-2 leaf (2, 2) across the seam -- a refinement boundary through
  the seam. The level-1 box (1, 2) is refined by the 2:1 balance alone.
* ``tree_T``: the walled twin: three copies of P tiled along pd, P's boxes
  asked for by location in every tile. The centre tile has the neighbours P
  reaches by wrap, on code paths that never see a flag.
* ``level1_operator``: the wrapped 5-point operator of a level-1 grid as a
  dense matrix with the walls folded in (stencil_handle_boundaries,
  m_coarse_solver.f90:442-491), Cartesian or cylindrical (af_cyl: the r
  neighbours weighted by their face radius over the cell's), and the folded
  right-hand side.
* ``wrap_ghosts``: the face ghost cells of a uniform level across the seam
  by direct wrap of the neighbours' interiors.
"""
import numpy as np

from afh.amr import AF_CYL, AF_XYZ, DO_REF, KEEP_REF, AfTree

BC_DIRICHLET, BC_NEUMANN = -10, -11
DR = 2.0 ** -10  # a power of two: every box corner and 1 / dr are exact
L1_DR = (2.0 ** -3, 2.0 ** -4)  # the level-1-only grids (as the 3-D tests')

STEP1 = {(1, 1, 1)}
STEP2 = {(2, 1, 1), (2, 2, 1), (2, 1, 2)}


def periodic_of(pd):
    return (pd == 0, pd == 1)


def _swap(key, pd):
    return key if pd == 0 else (key[0], key[2], key[1])


def _base(pd):
    """Level-1 boxes of one tile per dimension."""
    return (1, 2) if pd == 0 else (2, 1)


def _boxes_per_dim(pd, lvl):
    return [b * 2 ** (lvl - 1) for b in _base(pd)]


def _tile_key(t, b, pd):
    n = _boxes_per_dim(pd, t.lvl[b])
    return (t.lvl[b],) + tuple((t.ix[b][d] - 1) % n[d] + 1 for d in range(2))


def _refine_by_location(t, want, pd):
    """One af_adjust_refinement asking for the boxes whose (level, index
    within their tile) is in `want`."""
    def fn(ids):
        f = [DO_REF if _tile_key(t, b, pd) in want else KEEP_REF for b in ids]
        return np.array(f), np.zeros(len(ids), np.uint32)
    return t.adjust_refinement(fn)


def _tree(nc, tiles, pd, periodic, levels, coord=AF_XYZ):
    base = _base(pd)
    ext = np.array([nc * base[0], nc * base[1]]) * DR
    n_t = [tiles if d == pd else 1 for d in range(2)]
    r_min = np.array([-(n_t[d] // 2) * ext[d] for d in range(2)])
    if coord == AF_CYL:
        r_min[0] = 0.0
    r_max = r_min + ext * np.array(n_t)
    t = AfTree(nc, r_max, [nc * base[d] * n_t[d] for d in range(2)], periodic=periodic,
               r_min=r_min, coord=coord)
    if levels >= 2:
        _refine_by_location(t, {_swap(k, pd) for k in STEP1}, pd)
    if levels >= 3:
        _refine_by_location(t, {_swap(k, pd) for k in STEP2}, pd)
    return t


def tree_P(nc=8, levels=3, pd=0, coord=AF_XYZ):
    return _tree(nc, 1, pd, periodic_of(pd), levels, coord)


def _like(P, t, pd):
    for lvl in range(1, P.highest_lvl):
        _refine_by_location(t, {box_key(P, b) for b in P.lvls[lvl]["parents"]}, pd)
    return t


def tree_T(nc=8, levels=3, pd=0, coord=AF_XYZ):
    """Every tile gets P's boxes, those the 2:1 balance added across P's seam
    too (asked for by location: at T's outer walls no seam would add them)."""
    P = tree_P(nc, levels, pd, coord)
    return _like(P, _tree(nc, 3, pd, (False, False), 1, coord), pd)


def walled_like(P, pd=0):
    """P's boxes on a tree without periodic flags."""
    t = _like(P, _tree(P.nc, 1, pd, (False, False), 1, P.coord), pd)
    assert sorted(box_key(t, b) for b in used(t)) == sorted(box_key(P, b) for b in used(P))
    return t


def grow(t, pd, levels):
    """The refinement of tree_P / tree_T(levels) on an existing tree with
    fewer levels (for regrid tests); the box ids of the old tree persist."""
    return _like(tree_P(t.nc, levels, pd, t.coord), t, pd)


def used(t):
    return [b for b in range(1, t.highest_id + 1) if t.in_use[b]]


def box_key(t, b):
    return (t.lvl[b],) + tuple(t.ix[b])


def box_map(P, T, pd=0):
    """{box id of P: box id of T's centre tile at the same place}."""
    at = {box_key(T, b): b for b in used(T)}
    out = {}
    for b in used(P):
        n = _boxes_per_dim(pd, P.lvl[b])
        k = [P.lvl[b], P.ix[b][0], P.ix[b][1]]
        k[1 + pd] += n[pd]
        out[b] = at[tuple(k)]
    return out


def fill_by_location(P, T, rng, pd=0, scale=1.0, positive=False, shape=None):
    """Random box arrays (n_boxes,) + shape (default (ng, ng)) of P and T:
    every box of T holds what P's box at the same place within its tile
    holds."""
    shape = (P.nc + 2,) * 2 if shape is None else shape
    a = rng.standard_normal((P.highest_id,) + shape) * scale
    out = rng.standard_normal((T.highest_id,) + shape) * scale
    if positive:
        a, out = np.abs(a) + 0.1 * scale, np.abs(out) + 0.1 * scale
    of = {box_key(P, b): b for b in used(P)}
    for b in used(T):
        k = _tile_key(T, b, pd)
        if k in of:
            out[b - 1] = a[of[k] - 1]
    return a, out


def level1_operator(n, dr, periodic, bc, lam=0.0, cyl=False, v=None):
    """(A, fold): the level-1 operator lpl - lam of a grid of n = (nx, ny)
    cells (unknown p = j nx + i, 0-based) with wrapped neighbours in the
    periodic dimensions and the walls of the others folded in; bc = four
    (type, value). cyl: the first dimension is r from 0, its neighbours
    weighted (r -+ dr / 2) / r (af_stencil_get_box, m_af_stencil.f90). v: rows
    given per cell, {(i, j): (c, -x, +x, -y, +y)}, instead of the Laplacian's
    (an electrode box). fold(rhs) adds the walls' values to a right-hand side
    of shape (ny, nx)."""
    nx, ny = n
    N = nx * ny
    A = np.zeros((N, N))
    add = np.zeros(N)
    h = [1.0 / (dr[d] * dr[d]) for d in range(2)]
    for j in range(ny):
        for i in range(nx):
            p = j * nx + i
            q = [i, j]
            if v is not None and (i, j) in v:
                c = list(v[(i, j)])
            else:
                c = [0.0, h[0], h[0], h[1], h[1]]
                if cyl:
                    r = (i + 0.5) * dr[0]
                    c[1] = h[0] * (r - 0.5 * dr[0]) / r
                    c[2] = h[0] * (r + 0.5 * dr[0]) / r
                c[0] = -(c[1] + c[2] + c[3] + c[4]) - lam
            A[p, p] += c[0]
            for d in range(2):
                for side, step in ((0, -1), (1, 1)):
                    cn = c[1 + 2 * d + side]
                    m = list(q)
                    m[d] += step
                    if 0 <= m[d] < n[d]:
                        pass
                    elif periodic[d]:
                        m[d] %= n[d]
                    else:
                        typ, val = bc[2 * d + side]
                        if typ == BC_DIRICHLET:
                            A[p, p] -= cn
                            add[p] += -2 * cn * val
                        else:
                            A[p, p] += cn
                            add[p] += -(cn * dr[d]) * step * val
                        continue
                    # (+=: on a line of 2 points the one neighbour enters twice)
                    A[p, m[1] * nx + m[0]] += cn
    return A, (lambda rhs: rhs.reshape(-1) + add)


def level1_a7(n, dr, periodic, bc, lam=0.0, cyl=False):
    """The folded operator as PFMG's set-up takes it: per point the centre,
    then -x, +x, -y, +y, and two zeros (0 toward a wall, kept across a
    periodic face)."""
    A, _ = level1_operator(n, dr, periodic, bc, lam, cyl)
    nx, ny = n
    a7 = np.zeros((nx * ny, 7))
    for j in range(ny):
        for i in range(nx):
            p, q = j * nx + i, (i, j)
            a7[p, 0] = A[p, p]
            for d in range(2):
                for side, step in ((0, -1), (1, 1)):
                    if 0 <= q[d] + step < n[d] or periodic[d]:
                        m = list(q)
                        m[d] = (m[d] + step) % n[d]
                        a = A[p, m[1] * nx + m[0]]
                        # (2 points: the one neighbour's entry is the sum of both)
                        a7[p, 1 + 2 * d + side] = a / 2 if (n[d] == 2 and periodic[d]) else a
    return a7, A


def gather_level1(t, a):
    """Box array (n_boxes, ng, ng) -> the level-1 grid (ny, nx)."""
    nc = t.nc
    nx, ny = t.coarse_grid_size
    g = np.zeros((ny, nx))
    for b in t.lvls[1]["ids"]:
        o = [(x - 1) * nc for x in t.ix[b]]
        g[o[1]:o[1] + nc, o[0]:o[0] + nc] = a[b - 1, 1:-1, 1:-1]
    return g


def wrap_ghosts(t, a, lvl):
    """The face ghost cells, in the periodic dimensions, of every box of the
    uniform level `lvl` from the interiors of the level as one wrapped grid;
    the other faces are left as they are in `a`. Returns a copy of `a`."""
    nc = t.nc
    n = [x * nc * 2 ** (lvl - 1) // nc for x in t.coarse_grid_size]
    g = np.zeros((n[1], n[0]))
    ids = t.lvls[lvl]["ids"]
    for b in ids:
        o = [(x - 1) * nc for x in t.ix[b]]
        g[o[1]:o[1] + nc, o[0]:o[0] + nc] = a[b - 1, 1:-1, 1:-1]
    out = a.copy()
    for b in ids:
        o = [(x - 1) * nc for x in t.ix[b]]
        ys, xs = slice(o[1], o[1] + nc), slice(o[0], o[0] + nc)
        if t.periodic[0]:
            out[b - 1, 1:-1, 0] = g[ys, (o[0] - 1) % n[0]]
            out[b - 1, 1:-1, -1] = g[ys, (o[0] + nc) % n[0]]
        if t.periodic[1]:
            out[b - 1, 0, 1:-1] = g[(o[1] - 1) % n[1], xs]
            out[b - 1, -1, 1:-1] = g[(o[1] + nc) % n[1], xs]
    return out


def seam_faces(af):
    """(box, face nb 0..3, neighbour) of every same-level neighbour reached
    across a seam."""
    out = []
    for b in used(af):
        for nb in range(4):
            o = af.neighbors[b][nb]
            d, up = nb // 2, nb % 2
            if o <= 0 or (o != b and (af.ix[o][d] > af.ix[b][d]) == bool(up)):
                continue
            out.append((b, nb, o))
    return out


def check_seam_ghosts(af, a, what):
    """Box array a: every face ghost layer across a seam equals the
    neighbour's interior layer. Returns the number of such faces on levels
    >= 2."""
    nc, deep = af.nc, 0
    for b, nb, o in seam_faces(af):
        d, up = nb // 2, nb % 2
        ghost, inner = [slice(1, -1)] * 2, [slice(1, -1)] * 2
        ghost[1 - d] = nc + 1 if up else 0
        inner[1 - d] = 1 if up else nc
        assert np.array_equal(a[b - 1][tuple(ghost)], a[o - 1][tuple(inner)]), (what, b, nb)
        deep += af.lvl[b] >= 2
    return deep

"""Independent numpy statements for the periodic-domain tests, and the two
trees those tests run on.

* ``tree_P``: level-1 grid nc x 2nc x 2nc cells (1 x 2 x 2 boxes), periodic
  (T, T, F): x has a box that is its own neighbour, y the same box on both
  sides, z physical walls. The level-1 boxes with ix(2) = 2 are refined, then
  the level-2 boxes (1, 4, 1) and (2, 4, 1), which touch the y seam from
  below (the pair spans the x seam, so level 3 wraps onto itself in x): three
  levels, a refinement boundary across the seam, and the level-1 box across
  the seam refined by the 2:1 balance alone.
* ``tree_T``: the tiled twin, not periodic: 3 x 3 copies of P in x and y with
  P's boxes requested by location in every tile. Its centre tile has the
  neighbours P reaches by wrap, so an operation that reaches less than a tile
  gives the centre tile P's values bit for bit -- on code paths that never see
  a periodic flag.
* ``level1_operator``: the wrapped 7-point operator of a level-1 grid as a
  dense matrix, physical walls folded in (stencil_handle_boundaries,
  m_coarse_solver.f90:442-491), and the folded right-hand side.
* ``pfmg_dense`` / ``pfmg_interp``: a level of the PFMG hierarchy and its
  interpolation as dense matrices with wrapped indices, for R A P.
* ``wrap_ghosts``: the face ghost cells of a uniform level by direct wrap of
  the neighbours' interiors.
"""
import numpy as np

from afh.amr import DO_REF, KEEP_REF, AfTree

BC_DIRICHLET, BC_NEUMANN = -10, -11
PERIODIC = (True, True, False)
DR = 2.0 ** -10  # a power of two: every box corner and 1 / dr are exact


def _boxes_per_dim(tiles, lvl):
    return [t * b * 2 ** (lvl - 1) for t, b in zip(tiles, (1, 2, 2))]


def _refine_by_location(t, want, tiles):
    """One af_adjust_refinement asking for the boxes whose (level, index
    within their tile) is in `want`."""
    def fn(ids):
        f = []
        for b in ids:
            n = _boxes_per_dim((1, 1, 1), t.lvl[b])
            key = (t.lvl[b],) + tuple((t.ix[b][d] - 1) % n[d] + 1 for d in range(3))
            f.append(DO_REF if key in want else KEEP_REF)
        return np.array(f), np.zeros(len(ids), np.uint32)
    return t.adjust_refinement(fn)


STEP1 = {(1, 1, 2, 1), (1, 1, 2, 2)}   # the level-1 boxes with ix(2) = 2
# their children under the y seam at z = 0: both of them in x, so that level
# 3 spans the x seam and has a same-level neighbour by wrap as well
STEP2 = {(2, 1, 4, 1), (2, 2, 4, 1)}


def _tree(nc, tiles, periodic, levels):
    ext = np.array([nc, 2 * nc, 2 * nc]) * DR
    r_min = np.array([-(tiles[0] // 2) * ext[0], -(tiles[1] // 2) * ext[1], 0.0])
    r_max = r_min + ext * np.array(tiles)
    t = AfTree(nc, r_max, [nc * tiles[0], 2 * nc * tiles[1], 2 * nc * tiles[2]],
               periodic=periodic, r_min=r_min)
    if levels >= 2:
        _refine_by_location(t, STEP1, tiles)
    if levels >= 3:
        _refine_by_location(t, STEP2, tiles)
    return t


def tree_P(nc=8, levels=3):
    return _tree(nc, (1, 1, 1), PERIODIC, levels)


def tree_T(nc=8, levels=3):
    """Every tile gets P's boxes, those the 2:1 balance added across P's seam
    too (asked for by location: at T's outer walls no seam would add them)."""
    P = tree_P(nc, levels)
    t = _tree(nc, (3, 3, 1), (False,) * 3, 1)
    for lvl in range(1, P.highest_lvl):
        _refine_by_location(t, {box_key(P, b) for b in P.lvls[lvl]["parents"]}, (3, 3, 1))
    return t


def walled_like(P):
    """P's boxes (the ones the 2:1 balance added across the seam too) on a
    tree without periodic flags."""
    t = _tree(P.nc, (1, 1, 1), (False,) * 3, 1)
    for lvl in range(1, P.highest_lvl):
        _refine_by_location(t, {box_key(P, b) for b in P.lvls[lvl]["parents"]}, (1, 1, 1))
    assert sorted(box_key(t, b) for b in range(1, t.highest_id + 1) if t.in_use[b]) == \
        sorted(box_key(P, b) for b in range(1, P.highest_id + 1) if P.in_use[b])
    return t


def grow(t, tiles, levels):
    """The refinement of tree_P / tree_T(levels) on an existing tree with
    fewer levels (for regrid tests); the box ids of the old tree persist."""
    P = tree_P(t.nc, levels)
    for lvl in range(1, P.highest_lvl):
        _refine_by_location(t, {box_key(P, b) for b in P.lvls[lvl]["parents"]}, tiles)
    return t


def box_key(t, b):
    return (t.lvl[b],) + tuple(t.ix[b])


def box_map(P, T):
    """{box id of P: box id of T's centre tile at the same place}."""
    at = {box_key(T, b): b for b in range(1, T.highest_id + 1) if T.in_use[b]}
    out = {}
    for b in range(1, P.highest_id + 1):
        if not P.in_use[b]:
            continue
        n = _boxes_per_dim((1, 1, 1), P.lvl[b])
        k = (P.lvl[b], P.ix[b][0] + n[0], P.ix[b][1] + n[1], P.ix[b][2])
        out[b] = at[k]
    return out


def fill_by_location(P, T, rng, scale=1.0, positive=False):
    """Random box arrays (n_boxes, ng, ng, ng) of P and T: every box of T
    holds what P's box at the same place within its tile holds."""
    ng = P.nc + 2
    a = rng.standard_normal((P.highest_id, ng, ng, ng)) * scale
    if positive:
        a = np.abs(a) + 0.1 * scale
    of = {box_key(P, b): b for b in range(1, P.highest_id + 1) if P.in_use[b]}
    out = rng.standard_normal((T.highest_id, ng, ng, ng)) * scale
    if positive:
        out = np.abs(out) + 0.1 * scale
    for b in range(1, T.highest_id + 1):
        if not T.in_use[b]:
            continue
        n = _boxes_per_dim((1, 1, 1), T.lvl[b])
        k = (T.lvl[b],) + tuple((T.ix[b][d] - 1) % n[d] + 1 for d in range(3))
        if k in of:
            out[b - 1] = a[of[k] - 1]
    return a, out


def level1_operator(n, dr, periodic, bc, lam=0.0):
    """(A, fold): the level-1 operator lpl - lam of a grid of n = (nx, ny, nz)
    cells (unknown p = (k ny + j) nx + i, 0-based) with wrapped neighbours in
    the periodic dimensions and the walls of the others folded in; bc = six
    (type, value). fold(rhs) adds the walls' values to a right-hand side of
    shape (nz, ny, nx)."""
    nx, ny, nz = n
    N = nx * ny * nz
    A = np.zeros((N, N))
    add = np.zeros(N)
    h = [1.0 / (dr[d] * dr[d]) for d in range(3)]
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                p = (k * ny + j) * nx + i
                q = [i, j, k]
                A[p, p] -= lam
                for d in range(3):
                    A[p, p] -= 2 * h[d]
                    for side, step in ((0, -1), (1, 1)):
                        m = list(q)
                        m[d] += step
                        if 0 <= m[d] < n[d]:
                            pass
                        elif periodic[d]:
                            m[d] %= n[d]
                        else:
                            typ, val = bc[2 * d + side]
                            if typ == BC_DIRICHLET:
                                A[p, p] -= h[d]
                                add[p] += -2 * h[d] * val
                            else:
                                A[p, p] += h[d]
                                add[p] += -(h[d] * dr[d]) * step * val
                            continue
                        # (+=: on a line of 2 points the one neighbour enters twice)
                        A[p, (m[2] * ny + m[1]) * nx + m[0]] += h[d]
    return A, (lambda rhs: rhs.reshape(-1) + add)


def level1_fold(n, dr, periodic, bc):
    """fold of level1_operator without the matrix."""
    nx, ny, nz = n
    add = np.zeros((nz, ny, nx))
    for d, axis in ((0, 2), (1, 1), (2, 0)):
        if periodic[d]:
            continue
        h = 1.0 / (dr[d] * dr[d])
        for side, step, at in ((0, -1, 0), (1, 1, -1)):
            sl = [slice(None)] * 3
            sl[axis] = at
            typ, val = bc[2 * d + side]
            add[tuple(sl)] += -2 * h * val if typ == BC_DIRICHLET else -(h * dr[d]) * step * val
    return lambda rhs: rhs.reshape(-1) + add.reshape(-1)


def level1_apply(u, dr, periodic, bc, lam=0.0):
    """The same operator applied to u of shape (nz, ny, nx) without a matrix
    (for grids too large for a dense one): a wall's ghost value is -u
    (Dirichlet) or u (Neumann), the wall's own value being in the folded
    right-hand side."""
    out = -lam * u
    for d, axis in ((0, 2), (1, 1), (2, 0)):
        h = 1.0 / (dr[d] * dr[d])
        lo, hi = np.roll(u, 1, axis), np.roll(u, -1, axis)
        if not periodic[d]:
            first = [slice(None)] * 3
            last = [slice(None)] * 3
            first[axis], last[axis] = 0, -1
            first, last = tuple(first), tuple(last)
            lo[first] = -u[first] if bc[2 * d][0] == BC_DIRICHLET else u[first]
            hi[last] = -u[last] if bc[2 * d + 1][0] == BC_DIRICHLET else u[last]
        out = out + h * (lo - 2 * u + hi)
    return out


def gather_level1(t, a):
    """Box array (n_boxes, ng, ng, ng) -> the level-1 grid (nz, ny, nx)."""
    nc = t.nc
    nx, ny, nz = t.coarse_grid_size
    g = np.zeros((nz, ny, nx))
    for b in t.lvls[1]["ids"]:
        o = [(x - 1) * nc for x in t.ix[b]]
        g[o[2]:o[2] + nc, o[1]:o[1] + nc, o[0]:o[0] + nc] = a[b - 1, 1:-1, 1:-1, 1:-1]
    return g


def wrap_ghosts(t, a, lvl):
    """The face ghost cells of every box of the uniform level `lvl` from the
    interiors of the level as one wrapped grid; physical faces (z) are left
    as they are in `a`. Returns a copy of `a` with those ghost cells set."""
    nc = t.nc
    nb = _boxes_per_dim((1, 1, 1), lvl)
    n = [x * nc for x in nb]
    g = np.zeros((n[2], n[1], n[0]))
    ids = t.lvls[lvl]["ids"]
    for b in ids:
        o = [(x - 1) * nc for x in t.ix[b]]
        g[o[2]:o[2] + nc, o[1]:o[1] + nc, o[0]:o[0] + nc] = a[b - 1, 1:-1, 1:-1, 1:-1]
    out = a.copy()
    for b in ids:
        o = [(x - 1) * nc for x in t.ix[b]]
        zs, ys, xs = (slice(o[2], o[2] + nc), slice(o[1], o[1] + nc), slice(o[0], o[0] + nc))
        if t.periodic[0]:
            out[b - 1, 1:-1, 1:-1, 0] = g[zs, ys, (o[0] - 1) % n[0]]
            out[b - 1, 1:-1, 1:-1, -1] = g[zs, ys, (o[0] + nc) % n[0]]
        if t.periodic[1]:
            out[b - 1, 1:-1, 0, 1:-1] = g[zs, (o[1] - 1) % n[1], xs]
            out[b - 1, 1:-1, -1, 1:-1] = g[zs, (o[1] + nc) % n[1], xs]
        if t.periodic[2]:
            out[b - 1, 0, 1:-1, 1:-1] = g[(o[2] - 1) % n[2], ys, xs]
            out[b - 1, -1, 1:-1, 1:-1] = g[(o[2] + nc) % n[2], ys, xs]
    return out


def level1_a7(n, dr, periodic, bc, lam=0.0):
    """The folded operator as PFMG's set-up takes it: per point the centre,
    then -x, +x, -y, +y, -z, +z (0 toward a wall, kept across a periodic
    face)."""
    A, _ = level1_operator(n, dr, periodic, bc, lam)
    nx, ny, nz = n
    a7 = np.zeros((nx * ny * nz, 7))
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                p, q = (k * ny + j) * nx + i, (i, j, k)
                a7[p, 0] = A[p, p]
                for d in range(3):
                    for side, step in ((0, -1), (1, 1)):
                        if 0 <= q[d] + step < n[d] or periodic[d]:
                            a7[p, 1 + 2 * d + side] = 1.0 / (dr[d] * dr[d])
    return a7, A


def pfmg_dense(nn, Al, periodic):
    """A level's 27-point operator (points x 27, offset (dx, dy, dz) at
    (dz+1) 9 + (dy+1) 3 + (dx+1)) as a dense matrix; an entry that leaves the
    grid in a direction that is not periodic must be 0."""
    nx, ny, nz = (int(v) for v in nn)
    M = np.zeros((nx * ny * nz,) * 2)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                p = (k * ny + j) * nx + i
                for s in np.nonzero(Al[p])[0]:
                    g = [i + s % 3 - 1, j + (s // 3) % 3 - 1, k + s // 9 - 1]
                    for d in range(3):
                        if not 0 <= g[d] < nn[d]:
                            assert periodic[d], (tuple(nn), p, s)
                            g[d] %= nn[d]
                    M[p, (g[2] * ny + g[1]) * nx + g[0]] += Al[p, s]
    return M


def pfmg_interp(nf, nc, cd, Pl, periodic):
    """Interpolation from the even points of direction cd (1-based) as a
    dense matrix: 1 at an even point; at an odd point f the weights Pl[:, 0]
    toward (f - 1) / 2 -- for f = 1 the last coarse point when periodic, else
    nothing -- and Pl[:, 1] toward (f + 1) / 2."""
    nf, nc = [int(v) for v in nf], [int(v) for v in nc]
    M = np.zeros((int(np.prod(nf)), int(np.prod(nc))))
    for k in range(nf[2]):
        for j in range(nf[1]):
            for i in range(nf[0]):
                q, p = [i, j, k], (k * nf[1] + j) * nf[0] + i
                f = q[cd] + 1

                def at(m):
                    c = list(q)
                    c[cd] = m - 1
                    return (c[2] * nc[1] + c[1]) * nc[0] + c[0]
                if f % 2 == 0:
                    M[p, at(f // 2)] += 1.0
                    continue
                if f >= 3:
                    M[p, at((f - 1) // 2)] += Pl[p, 0]
                elif periodic[cd]:
                    M[p, at(nc[cd])] += Pl[p, 0]
                else:
                    assert Pl[p, 0] == 0.0
                if (f + 1) // 2 <= nc[cd]:
                    M[p, at((f + 1) // 2)] += Pl[p, 1]
                else:
                    assert Pl[p, 1] == 0.0
    return M

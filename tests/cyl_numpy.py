"""The cylindrical (af_cyl) operators of afivo, stated in numpy (test reference).

Written from the reference's formulas, float64 operations in the order the
Fortran writes them (numpy neither reorders nor contracts them):

  af_cyl_radius_cc        r_i   = r_min + (i - 0.5) dr          (m_af_types.f90)
  af_cyl_flux_factors     rfac  = (r -+ 0.5 dr) * (1 / r)
  af_cyl_child_weights    w     = 1 -+ 0.25 dr / r
  stencil, per i          c2    = rfac1 c(2), c3 = rfac2 c(3),
                          c1    = c(1) - (c2 - c(2)) - (c3 - c(3))  (m_af_stencil.f90)
  af_restrict_box         0.25 (w1 sum(cc(i_f, j_f:j_f+1)) + w2 sum(cc(i_f+1, j_f:j_f+1)))
  flux_from_children      0.5 (w1 F(2n-1) + w2 F(2n)) on faces normal to z
  flux_update_densities   dt_dr(1) (rfac1 F_i - rfac2 F_{i+1}) + dt_dr(2) (G_j - G_{j+1})
  af_tree_sum_cc          2 pi sum cc**p r_i per box, times product(dr)
  af_total_volume         pi (r1^2 - r0^2) L_z per coarse box

Arrays follow the device layout: a box's cell data is (nc + 2, nc + 2) indexed
[j, i] (i, the radial index, fastest), face data (2, nc + 1, nc + 1) indexed
[dim, j, i]. Indices i, j in the signatures are the reference's 1-based ones.
"""
import numpy as np

TWO_PI = 2 * np.arccos(-1.0)


def radius_cc(r_min, dr, nc):
    """r_i for i = 1 .. nc."""
    i = np.arange(1, nc + 1, dtype=np.float64)
    return r_min + (i - 0.5) * dr


def flux_factors(r_min, dr, nc):
    r = radius_cc(r_min, dr, nc)
    inv_r = 1 / r
    return (r - 0.5 * dr) * inv_r, (r + 0.5 * dr) * inv_r


def child_weights(r_min, dr, i):
    """(inner, outer) of coarse cell(s) i of a box with r_min, dr."""
    i = np.asarray(i, dtype=np.float64)
    tmp = 0.25 * dr / (r_min + (i - 0.5) * dr)
    return 1 - tmp, 1 + tmp


def lpl_coef(dr, lam=0.0):
    """mg_box_lpl_stencil: c(1..5) of a box with spacings dr = (dr_r, dr_z)."""
    c = np.zeros(5)
    for d in range(2):
        inv = 1 / (dr[d] * dr[d])
        c[1 + 2 * d] = inv
        c[2 + 2 * d] = inv
    s = c[1]
    for q in range(2, 5):
        s = s + c[q]
    c[0] = -s - lam
    return c


def cyl_coef(c, r_min, dr, nc):
    """Per i = 1 .. nc: (c1, c2, c3, 1 / c1) of the cylindrical stencil."""
    f1, f2 = flux_factors(r_min, dr, nc)
    c2 = f1 * c[1]
    c3 = f2 * c[2]
    c1 = c[0] - (c2 - c[1]) - (c3 - c[2])
    return c1, c2, c3, 1 / c1


def apply(p, c, r_min, dr):
    """stencil_apply_357 with cylindrical_gradient on the interior of box image
    p ((nc + 2)^2, ghost cells filled): an (nc, nc) array [j, i]."""
    nc = p.shape[0] - 2
    c1, c2, c3, _ = cyl_coef(c, r_min, dr, nc)
    return (c1 * p[1:-1, 1:-1] + c2 * p[1:-1, :-2] + c3 * p[1:-1, 2:] +
            c[3] * p[:-2, 1:-1] + c[4] * p[2:, 1:-1])


def residual(p, rhs, c, r_min, dr):
    return rhs[1:-1, 1:-1] - apply(p, c, r_min, dr)


def gsrb_half(p, rhs, c, r_min, dr, redblack):
    """One half sweep of stencil_gsrb_357 (cylindrical_gradient) on box image p,
    in place: cells with i0 = 2 - iand(ieor(redblack, j), 1), step 2."""
    nc = p.shape[0] - 2
    _, c2, c3, inv = cyl_coef(c, r_min, dr, nc)
    for j in range(1, nc + 1):
        i0 = 2 - ((redblack ^ j) & 1)
        i = np.arange(i0, nc + 1, 2)
        p[j, i] = (rhs[j, i] - c2[i - 1] * p[j, i - 1] - c3[i - 1] * p[j, i + 1] -
                   c[3] * p[j - 1, i] - c[4] * p[j + 1, i]) * inv[i - 1]
    return p


def restrict(child, parent, ix_child, p_r_min, p_dr, geometry=True):
    """af_restrict_box: the interior of `child` into its quadrant of `parent`
    (both (nc + 2)^2 images, in place on parent). ix_child: the child's
    (ix_r, ix_z); p_r_min, p_dr: the parent's radial origin and spacing."""
    nc = child.shape[0] - 2
    h = nc // 2
    oi, oj = ((ix_child[0] - 1) & 1) * h, ((ix_child[1] - 1) & 1) * h
    f = child[1:-1, 1:-1]
    a, b = f[0::2, 0::2], f[0::2, 1::2]      # (i_f, j_f), (i_f + 1, j_f)
    cc, d = f[1::2, 0::2], f[1::2, 1::2]     # (i_f, j_f + 1), (i_f + 1, j_f + 1)
    if geometry:
        w1, w2 = child_weights(p_r_min, p_dr, oi + np.arange(1, h + 1))
        val = 0.25 * (w1 * (a + cc) + w2 * (b + d))
    else:
        # 0.25 * sum(cc(i_f:i_f+1, j_f:j_f+1)): column-major element order
        val = 0.25 * (a + b + cc + d)
    parent[1 + oj:1 + oj + h, 1 + oi:1 + oi + h] = val
    return parent


def consistent_zface(f1, f2, r_min, dr, i):
    """flux_from_children on a face normal to z: fine fluxes F(2n-1), F(2n)
    into coarse cell(s) i of the coarse neighbour (r_min, dr)."""
    w1, w2 = child_weights(r_min, dr, i)
    return 0.5 * (w1 * f1 + w2 * f2)


def update_divergence(F, dt, r_min, dr):
    """The flux term of flux_update_densities for one box: F (2, nc+1, nc+1),
    dr = (dr_r, dr_z); an (nc, nc) array [j, i]."""
    nc = F.shape[1] - 1
    f1, f2 = flux_factors(r_min, dr[0], nc)
    dt_dr = dt / np.asarray(dr, dtype=np.float64)
    Fr, Fz = F[0, :nc, :], F[1, :, :nc]
    return (dt_dr[0] * (f1 * Fr[:, :nc] - f2 * Fr[:, 1:]) +
            dt_dr[1] * (Fz[:nc, :] - Fz[1:, :]))


def ipow(x, n):
    """gfortran's real ** integer: binary powering."""
    p = np.ones_like(x)
    while True:
        if n & 1:
            p = p * x
        n >>= 1
        if not n:
            return p
        x = x * x


def sum_2pr_box(cc, r_min, dr, power=1):
    """sum_2pr_box: res = res + cc(i, j)**power * r_i (j outer, i inner), then
    res * 2 pi."""
    nc = cc.shape[0] - 2
    r = radius_cc(r_min, dr, nc)
    res = 0.0
    for t in (ipow(cc[1:-1, 1:-1], power) * r).reshape(-1):
        res = res + t
    return res * TWO_PI


def tree_sum(boxes, power=1):
    """af_tree_sum_cc: boxes = [(cc image, r_min, (dr_r, dr_z))] of the leaves
    in the reference's loop order (levels, then leaves)."""
    s = 0.0
    for cc, r_min, dr in boxes:
        s = s + (dr[0] * dr[1]) * sum_2pr_box(cc, r_min, dr[0], power)
    return s


def total_volume(r_mins, box_len):
    """af_total_volume: the coarse boxes' r_min(1) and box_len = n_cell dr_base."""
    vol = 0.0
    for r0 in r_mins:
        r1 = r0 + box_len[0]
        vol = vol + np.pi * (r1 * r1 - r0 * r0) * box_len[1]
    return vol


# ---- a uniform level as one global array (every box of the level the same
# size, neighbours by copy): the box decomposition disappears except for the
# per-box radii, which are kept (r_min of the box + (i - 0.5) dr)
def level_radius_tables(c, box_r_mins, dr, nc):
    """Per global i: (c1, c2, c3, inv) concatenated over the boxes of one row."""
    parts = [cyl_coef(c, r0, dr, nc) for r0 in box_r_mins]
    return [np.concatenate([p[k] for p in parts]) for k in range(4)]


def fill_bc(g, bc, dr):
    """Side ghost cells of the global image g ((ny + 2, nx + 2)) from the
    physical boundaries, bc_to_gc: bc = 4 (type, value), type 'd' or 'n';
    order low r, high r, low z, high z."""
    def gc(kind, val, x1, h, low):
        if kind == "d":
            return 2 * val + -1 * x1
        return (h * (-1 if low else 1)) * val + 1 * x1
    g[1:-1, 0] = gc(bc[0][0], bc[0][1], g[1:-1, 1], dr[0], True)
    g[1:-1, -1] = gc(bc[1][0], bc[1][1], g[1:-1, -2], dr[0], False)
    g[0, 1:-1] = gc(bc[2][0], bc[2][1], g[1, 1:-1], dr[1], True)
    g[-1, 1:-1] = gc(bc[3][0], bc[3][1], g[-2, 1:-1], dr[1], False)
    return g


def level_gsrb_half(g, rhs, c, tabs, redblack):
    """gsrb_half on the global image (interior indices are box-local parity
    compatible: nc is even)."""
    _, c2, c3, inv = tabs
    ny, nx = g.shape[0] - 2, g.shape[1] - 2
    for j in range(1, ny + 1):
        i0 = 2 - ((redblack ^ j) & 1)
        i = np.arange(i0, nx + 1, 2)
        g[j, i] = (rhs[j, i] - c2[i - 1] * g[j, i - 1] - c3[i - 1] * g[j, i + 1] -
                   c[3] * g[j - 1, i] - c[4] * g[j + 1, i]) * inv[i - 1]
    return g


def level_apply(g, c, tabs):
    c1, c2, c3, _ = tabs
    return (c1 * g[1:-1, 1:-1] + c2 * g[1:-1, :-2] + c3 * g[1:-1, 2:] +
            c[3] * g[:-2, 1:-1] + c[4] * g[2:, 1:-1])


def level_matrix(c, tabs, nx, ny, bc):
    """The dense matrix and boundary vector of the level's discrete problem
    L phi = rhs with the ghost cells eliminated (bc as in fill_bc, dr folded by
    the caller through bvec): returns (A, ghost) with A (nx ny, nx ny) and
    ghost(k, face) the coefficient that multiplies the face's ghost value."""
    c1, c2, c3, _ = tabs
    n = nx * ny
    A = np.zeros((n, n))
    G = np.zeros((n, 4))
    for j in range(ny):
        for i in range(nx):
            k = j * nx + i
            A[k, k] = c1[i]
            for (di, dj, cf, face) in ((-1, 0, c2[i], 0), (1, 0, c3[i], 1),
                                       (0, -1, c[3], 2), (0, 1, c[4], 3)):
                ii, jj = i + di, j + dj
                if 0 <= ii < nx and 0 <= jj < ny:
                    A[k, jj * nx + ii] += cf
                else:
                    # ghost = a * bv + b * phi_k
                    b = -1.0 if bc[face][0] == "d" else 1.0
                    A[k, k] += cf * b
                    G[k, face] = cf
    return A, G

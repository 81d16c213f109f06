"""The seven limiters, af_prolong_limit and the branch census of the limiter
tests' inputs, stated in numpy (test reference).

Written from afivo/src/m_af_limiters.f90 (af_limiter_apply and the functions
it selects) and m_af_prolong.f90:311-420 (af_prolong_limit), float64
operations in the order the Fortran writes them; numpy neither reorders nor
contracts them, so comparisons with the libraries can be bitwise.

The census (`census`, `assert_census`) looks at the inputs only: it takes the
slope pairs (a, b) the flux and the prolongation form along each dimension
and counts how many fall into every branch of the Koren limiter and of the
generalised minmod limiter with theta = 1, 2 and 4/3, equalities included. A
test that is meant to exercise a branch asserts, on its own input, that the
branch is reached at least MIN_PAIRS times per dimension.
"""
import numpy as np

LIM_NONE, LIM_VANLEER, LIM_KOREN, LIM_MINMOD, LIM_MC, LIM_GMINMOD43, LIM_ZERO = range(1, 8)
LIMITERS = list(range(1, 8))
LIM_NAMES = {1: "none", 2: "vanleer", 3: "koren", 4: "minmod", 5: "mc", 6: "gminmod43",
             7: "zero"}
THETA = {LIM_MINMOD: 1.0, LIM_MC: 2.0, LIM_GMINMOD43: 4 / 3.0}
MIN_PAIRS = 3
LATTICE = 2.0 ** 50


# ------------------------------------------------------------------ limiters
def koren(a, b):
    """af_limiter_koren (m_af_limiters.f90:72-95), the branches in its order."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    third = 1 / 3.0
    aa, ab = a * a, a * b
    out = 2 * b
    out = np.where(aa <= 2.5 * ab, third * (b + 2 * a), out)
    out = np.where(aa <= 0.25 * ab, 2 * a, out)
    return np.where(ab <= 0, 0.0, out)


def vanleer(a, b):
    """af_limiter_vanleer (97-110)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ab = a * b
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ab > 0, 2 * ab / (a + b), 0.0)


def gminmod(a, b, theta):
    """af_limiter_gminmod (139-149): sign(minval(abs([theta a, theta b,
    0.5 (a + b)])), a) where a b > 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = np.minimum(np.minimum(np.abs(theta * a), np.abs(theta * b)), np.abs(0.5 * (a + b)))
    return np.where(a * b > 0, np.copysign(m, a), 0.0)


def limiter(lim, a, b):
    """af_limiter_apply (41-66)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if lim == LIM_NONE:
        return 0.5 * (a + b)
    if lim == LIM_VANLEER:
        return vanleer(a, b)
    if lim == LIM_KOREN:
        return koren(a, b)
    if lim in THETA:
        return gminmod(a, b, THETA[lim])
    if lim == LIM_ZERO:
        return np.zeros(np.broadcast(a, b).shape)
    raise ValueError("limiter %r" % lim)


# --------------------------------------------------------------- prolongation
def prolong_limit(cp, off, lim):
    """af_prolong_limit (m_af_prolong.f90:311-420) of one child from its
    parent's cells cp ((nc + 2,) * ndim, ghost cells included, [k][j][i]);
    off = af_get_child_offset in (i, j[, k]) order. Returns the child's
    interior (nc,) * ndim: f0 -+ f1 -+ f2 [-+ f3] in that order of
    operations, f_d = 0.25 limiter(c - c_{-d}, c_{+d} - c)."""
    ndim = cp.ndim
    nc = cp.shape[0] - 2
    h = nc // 2
    # parent cells under the child: index 1 + off .. h + off per dimension,
    # array axes are reversed ([k][j][i])
    sl = tuple(slice(1 + off[ndim - 1 - ax], 1 + off[ndim - 1 - ax] + h) for ax in range(ndim))

    def shifted(ax, s):
        q = list(sl)
        q[ax] = slice(sl[ax].start + s, sl[ax].stop + s)
        return cp[tuple(q)]

    f0 = cp[sl]
    f = []
    for d in range(ndim):  # d = 0 is x: the last axis
        ax = ndim - 1 - d
        f.append(0.25 * limiter(lim, f0 - shifted(ax, -1), shifted(ax, 1) - f0))
    out = np.zeros((nc,) * ndim)
    for corner in range(2 ** ndim):
        r = f0
        dst = [None] * ndim
        for d in range(ndim):
            up = (corner >> d) & 1
            r = r + f[d] if up else r - f[d]
            dst[ndim - 1 - d] = slice(up, nc, 2)
        out[tuple(dst)] = r
    return out


# --------------------------------------------------------------------- inputs
def lattice(rng, shape):
    """k 2^50 with k uniform in 0..8: neighbour differences are small integers
    times a power of two, so the limiter arguments land on the equalities of
    every branch."""
    return rng.integers(0, 9, size=shape).astype(np.float64) * LATTICE


# On the lattice the two sides of a Koren threshold give the same number: the
# limiter is continuous and third * (6 a) rounds to 2 a. These (a, b) sit on
# the thresholds in floating point only -- a a == 0.25 (a b) with b one ulp
# from 4 a; a a == 2.5 (a b) with a one ulp from 2.5 b, after the products are
# rounded -- and there the two sides differ in the last bit, so a `<` in place
# of a `<=` changes the result. 0, a, a + b are exact sums and differences.
KOREN_EDGES = ((8775936924003012.0, 35103747696012044.0),
               (12780040261468158.0, 5112016104587264.0))


def plant_koren_edges(cc, ndim, sites, reverse=False):
    """Three cells in a row (0, a, a + b) along every dimension, for the
    first pair of KOREN_EDGES from cell (1 + o,) * ndim and for the second
    from (2 + o,) * ndim, in every (box, o) of sites (as the harness'
    plant_edges, o = 0). reverse: (0, b, a + b), the pair as a flow in the
    positive direction takes it."""
    for b, o in sites:
        for q, (ea, eb) in enumerate(KOREN_EDGES):
            vals = (0.0, eb, eb + ea) if reverse else (0.0, ea, ea + eb)
            for d in range(ndim):
                for s, v in enumerate(vals):
                    ix = [q + 1 + o] * ndim
                    ix[d] += s
                    cc[(b,) + tuple(reversed(ix))] = v


def plant_edge_fields(fc_field, phi, ndim, sites):
    """A face field > 0 on the two faces between the planted cells, stored
    and as the gradient of phi (fac = -1: phi falls along the row)."""
    for b, o in sites:
        for q in range(len(KOREN_EDGES)):
            for d in range(ndim):
                for s in (0, 1, 2):
                    ix = [q + 1 + o] * ndim
                    ix[d] += s
                    phi[(b,) + tuple(reversed(ix))] = 64.0 * (2 - s)
                    if s:
                        fc_field[(b, d) + tuple(i - 1 for i in reversed(ix))] = 2.0 ** 18


def slope_pairs(lines, both=True):
    """The (a, b) formed along lines (..., n): for every three cells in a row
    (x0, x1, x2), reconstruct_upwind_1d takes (x1 - x0, x2 - x1) on the face
    between x0 and x1 when the flow is negative and (x2 - x1, x1 - x0) on the
    face between x1 and x2 when it is positive; the prolongation takes the
    first of the two only (both = False)."""
    lines = np.asarray(lines, np.float64)
    d0 = lines[..., 1:-1] - lines[..., :-2]
    d1 = lines[..., 2:] - lines[..., 1:-1]
    if not both:
        return d0.ravel(), d1.ravel()
    return (np.concatenate([d0.ravel(), d1.ravel()]),
            np.concatenate([d1.ravel(), d0.ravel()]))


def classes(a, b):
    """{class name: count} of the pairs, by the comparisons the limiters make
    (in floating point, as they make them)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    aa, ab = a * a, a * b
    pos = ab > 0
    mid = (1 / 3.0) * (b + 2 * a)
    out = {
        "koren ab<0": ab < 0,
        "koren ab==0": ab == 0,
        "koren aa<ab/4": pos & (aa < 0.25 * ab),
        "koren aa==ab/4": pos & (aa == 0.25 * ab),
        "koren middle": pos & (aa > 0.25 * ab) & (aa < 2.5 * ab),
        "koren aa==2.5ab": pos & (aa == 2.5 * ab),
        "koren aa>2.5ab": pos & (aa > 2.5 * ab),
        # on a threshold, and its two sides give different numbers
        "koren aa==ab/4, sides differ": pos & (aa == 0.25 * ab) & (2 * a != mid),
        "koren aa==2.5ab, sides differ": pos & (aa == 2.5 * ab) & (2 * b != mid),
    }
    for name, th in (("1", 1.0), ("2", 2.0), ("4/3", 4 / 3.0)):
        x, y, z = np.abs(th * a), np.abs(th * b), np.abs(0.5 * (a + b))
        m = np.minimum(np.minimum(x, y), z)
        n_min = (x == m).astype(int) + (y == m) + (z == m)
        out["theta %s: theta a" % name] = pos & (x == m) & (n_min == 1)
        out["theta %s: theta b" % name] = pos & (y == m) & (n_min == 1)
        if th > 1:  # |a + b| / 2 lies between |a| and |b|: never alone below both
            out["theta %s: (a+b)/2" % name] = pos & (z == m) & (n_min == 1)
        out["theta %s: tie" % name] = pos & (n_min > 1)
    return {k: int(np.count_nonzero(v)) for k, v in out.items()}


def census(boxes, ndim, both=True):
    """Per dimension, classes() of the slope pairs along that dimension of
    every box in `boxes` ((n, (nc + 2,) * ndim) with one ghost layer); the
    lines run through the cells 1..nc of the other dimensions."""
    boxes = np.asarray(boxes)
    out = []
    for d in range(ndim):
        ax = boxes.ndim - 1 - d
        sl = tuple(slice(None) if q == ax or q < boxes.ndim - ndim else slice(1, -1)
                   for q in range(boxes.ndim))
        a, b = slope_pairs(np.moveaxis(boxes[sl], ax, -1), both)
        out.append(classes(a, b))
    return out


def assert_census(boxes, ndim, what="", both=True):
    """At least MIN_PAIRS pairs in every class along every dimension."""
    for d, c in enumerate(census(boxes, ndim, both)):
        low = {k: v for k, v in c.items() if v < MIN_PAIRS}
        assert not low, "%s dimension %d: classes with fewer than %d pairs: %r" % (
            what, d, MIN_PAIRS, low)


def in_use(topo):
    """0-based indices of the boxes in use."""
    return np.concatenate([np.asarray(topo["lvl_ids_%d" % l])
                           for l in range(1, int(topo["highest_lvl"]) + 1)]) - 1


def leaves(topo):
    """0-based indices of the leaves."""
    return np.concatenate([np.asarray(topo["lvl_leaves_%d" % l])
                           for l in range(1, int(topo["highest_lvl"]) + 1)]) - 1


# ------------------------------------------------- the 2-D flux, electrons
BC_DIRICHLET, BC_NEUMANN, BC_CONTINUOUS, BC_DIRICHLET_COPY = -10, -11, -12, -13


class TopoTree:
    """The records ions2d_numpy's tree functions read (ids 1-based), from a
    topology dict."""

    def __init__(self, topo):
        self.nc = int(topo["nc"])
        self.highest_id = int(topo["n_boxes"])
        self.neighbors = [None] + [list(r) for r in topo["meta_neighbors"]]
        self.children = [None] + [list(r) for r in topo["meta_children"]]
        self.parent = [0] + list(topo["meta_parent"])
        self.ix = [None] + [list(r) for r in topo["meta_ix"]]
        self.dr = [None] + [np.array(r) for r in topo["meta_dr"]]
        self.r_min = [None] + [np.array(r) for r in topo["meta_r_min"]]
        self.in_use = [False] + [l > 0 for l in topo["meta_lvl"]]

    def has_children(self, b):
        return self.children[b][0] > 0


def _line(c, d, n):
    """Cells 1..nc of row (d = 1) or column (d = 0) n of a box [j][i]."""
    return c[1:-1, n] if d == 0 else c[n, 1:-1]


def bc_coefficients(bc_type, dr, nb, layers):
    """(c0, c1, c2) of bc_to_gc (layers = 1, m_af_ghostcell.f90:173-279: the
    ghost cell is c0 b + c1 x1 + c2 x2) or of bc_to_gc2 (layers = 2, 282-375:
    c0 b + c1 x1 and c2 b + c1 x2; 2-D has no high-y exception)."""
    d, pm = nb >> 1, 1.0 if nb & 1 else -1.0
    if bc_type == BC_DIRICHLET:
        return 2.0, -1.0, (0.0 if layers == 1 else 2.0)
    if bc_type == BC_NEUMANN:
        c0 = dr[d] * pm
        return c0, 1.0, (0.0 if layers == 1 else 3 * c0)
    if bc_type == BC_CONTINUOUS and layers == 1:
        return 0.0, 2.0, -1.0
    if bc_type == BC_DIRICHLET_COPY:
        return 1.0, 0.0, (0.0 if layers == 1 else 1.0)
    raise ValueError("bc type %r" % bc_type)


def bc_ghost_2d(c, nb, bc, dr, nc):
    """bc_to_gc of face nb (0-based) of box c [j][i]: the nc ghost cells."""
    c0, c1, c2 = bc_coefficients(bc[0], dr, nb, 1)
    d, low = nb >> 1, (nb & 1) == 0
    x1, x2 = _line(c, d, 1 if low else nc), _line(c, d, 2 if low else nc - 1)
    return c0 * bc[1] + c1 * x1 + c2 * x2


def gc2_layers_2d(af, a, b, bc, prolong):
    """af_gc2_box of leaf b (ions2d_numpy.gc2_layers with the boundary types
    of bc_to_gc2 and the prolongation limiter open)."""
    nc = af.nc
    c = a[b - 1]
    l1, l2 = np.zeros((4, nc)), np.zeros((4, nc))
    for nb in range(4):
        d, low = nb >> 1, (nb & 1) == 0
        nid = af.neighbors[b][nb]
        if nid > 0:
            l1[nb] = _line(a[nid - 1], d, nc if low else 1)
            l2[nb] = _line(a[nid - 1], d, nc - 1 if low else 2)
        elif nid < 0:
            c0, c1, c2 = bc_coefficients(bc[nb][0], af.dr[b], nb, 2)
            l1[nb] = c0 * bc[nb][1] + c1 * _line(c, d, 1 if low else nc)
            l2[nb] = c2 * bc[nb][1] + c1 * _line(c, d, 2 if low else nc - 1)
        else:
            # gc2_prolong_rb: limited slopes of the parent's neighbour
            hnc, td = nc // 2, 1 - d
            cp = a[af.neighbors[af.parent[b]][nb] - 1]
            n_ = nc if low else 1
            for t in range(1, nc + 1):
                tc = ((af.ix[b][td] - 1) & 1) * hnc + ((t + 1) >> 1)
                j, i = (tc, n_) if d == 0 else (n_, tc)
                f0 = cp[j, i]
                fx = 0.25 * float(limiter(prolong, f0 - cp[j, i - 1], cp[j, i + 1] - f0))
                fy = 0.25 * float(limiter(prolong, f0 - cp[j - 1, i], cp[j + 1, i] - f0))
                st = -1.0 if (t & 1) else 1.0

                def val(sn):
                    sx, sy = (sn, st) if d == 0 else (st, sn)
                    r = f0
                    r = r - fx if sx < 0 else r + fx
                    r = r - fy if sy < 0 else r + fy
                    return r
                l1[nb, t - 1] = val(1.0 if low else -1.0)
                l2[nb, t - 1] = val(-1.0 if low else 1.0)
    return l1, l2


def upwind_faces(lines, positive, lim):
    """reconstruct_upwind_1d (m_af_flux_schemes.f90:282-303): lines (n, nc +
    4) along the flux dimension -> face values (n, nc + 1)."""
    n = lines.shape[1] - 4
    LL, L, R, RR = (lines[:, k:k + n + 1] for k in range(4))
    return np.where(positive, L + 0.5 * limiter(lim, R - L, L - LL),
                    R - 0.5 * limiter(lim, R - L, RR - R))


def box_flux_2d(pads, E, Ef, dr, td, N_inv, lim, mob=(), q=(-1.0,)):
    """flux_upwind_box of one box (ions2d_numpy.box_fluxes with the limiter
    open): pads (1 + n_ions, nc + 4, nc + 4) the padded densities of the flux
    species, the electrons first; E the cell-centred |E|; Ef (2, nc + 1,
    nc + 1) the face field; mob the ions' mobilities x N, q the charge signs
    (q[0] = -1). Returns F (1 + n_ions, 2, nc + 1, nc + 1), the cell CFL sums
    and the largest conductivity sum mu_e u_e + sum_n mu_n u_n."""
    import ions2d_numpy as inp
    nc = pads[0].shape[0] - 4
    nf = nc + 1
    F = np.zeros((len(pads), 2, nf, nf))
    cfl = np.zeros((nc, nc))
    smax = -np.inf
    for d in range(2):
        idx = 1 / dr[d]
        El = (E if d == 0 else E.T)[1:nc + 1, :]
        ex = Ef[0][0:nc, :] if d == 0 else Ef[1][:, 0:nc].T
        tfc = 0.5 * (El[:, 0:nf] + El[:, 1:nf + 1]) * 1e21 * N_inv
        mu = inp.lt_col(td, 1, tfc) * N_inv
        dc = inp.lt_col(td, 2, tfc) * N_inv
        v = -mu * ex
        ne = (pads[0] if d == 0 else pads[0].T)[2:nc + 2, :]
        u = upwind_faces(ne, q[0] * ex > 0, lim)
        flux = [v * u - dc * idx * (ne[:, 2:nf + 2] - ne[:, 1:nf + 1])]
        sig = mu * u
        term = (1.0 * np.maximum(np.abs(v[:, 1:]), np.abs(v[:, :-1])) * idx +
                2 * np.maximum(dc[:, 1:], dc[:, :-1]) * (idx * idx))
        cfl = cfl + (term if d == 0 else term.T)
        for n in range(1, len(pads)):
            mu_n = mob[n - 1] * N_inv
            un = upwind_faces((pads[n] if d == 0 else pads[n].T)[2:nc + 2, :], q[n] * ex > 0, lim)
            flux.append((q[n] * mu_n * ex) * un)
            sig = sig + mu_n * un
        smax = max(smax, sig.max())
        for n in range(len(pads)):
            if d == 0:
                F[n, 0, 0:nc, :] = flux[n]
            else:
                F[n, 1, :, 0:nc] = flux[n].T
    return F, cfl, smax


def flux_2d(topo, dens, efld, fc_field, td, N_inv, lim, prolong, bc, mob=(), q=(-1.0,),
            cyl=False):
    """flux_upwind_tree on a 2-D tree (m_af_flux_schemes.f90:666-848) over the
    flux species dens = [electrons, ions ...] (a single array: the electrons
    alone): af_restrict_ref_boundary, per level and leaf af_gc2_box (the first
    layer written back) and the fluxes, then af_consistent_fluxes; cyl: the
    radial weights of the restriction and of the coarse z faces. Returns (F
    per species tree-wide, the densities as the call leaves them, (dt_cfl,
    dt_drt)); for a single array in, single arrays out."""
    import cyl_numpy as cn
    import ions2d_numpy as inp
    single = isinstance(dens, np.ndarray)
    a = [np.array(x, np.float64) for x in ([dens] if single else dens)]
    af = TopoTree(topo)
    nc = af.nc
    h = nc // 2
    # af_restrict_ref_boundary: children with a refinement boundary
    for p in range(1, af.highest_id + 1):
        if not af.in_use[p] or not af.has_children(p):
            continue
        for k, c in enumerate(af.children[p]):
            if all(n != 0 for n in af.neighbors[c]):
                continue
            i0, j0 = (k & 1) * h, (k >> 1) * h
            for y in a:
                x = y[c - 1][1:-1, 1:-1]
                c00, c10, c01, c11 = x[0::2, 0::2], x[0::2, 1::2], x[1::2, 0::2], x[1::2, 1::2]
                if cyl:
                    w1, w2 = cn.child_weights(af.r_min[p][0], af.dr[p][0],
                                              np.arange(i0 + 1, i0 + h + 1))
                    r = 0.25 * (w1[None, :] * (c00 + c01) + w2[None, :] * (c10 + c11))
                else:
                    r = 0.25 * (c00 + c10 + c01 + c11)
                y[p - 1][1 + j0:1 + j0 + h, 1 + i0:1 + i0 + h] = r
    F = np.zeros((len(a),) + np.shape(fc_field))
    cfl_max, sig_max = -np.inf, -np.inf
    for l in range(1, int(topo["highest_lvl"]) + 1):
        for b in topo["lvl_leaves_%d" % l]:
            b = int(b)
            pads = []
            for y in a:
                l1, l2 = gc2_layers_2d(af, y, b, bc, prolong)
                P = np.zeros((nc + 4, nc + 4))
                P[2:-2, 2:-2] = y[b - 1][1:-1, 1:-1]
                P[2:-2, 1], P[2:-2, 0] = l1[0], l2[0]
                P[2:-2, nc + 2], P[2:-2, nc + 3] = l1[1], l2[1]
                P[1, 2:-2], P[0, 2:-2] = l1[2], l2[2]
                P[nc + 2, 2:-2], P[nc + 3, 2:-2] = l1[3], l2[3]
                g = y[b - 1]
                g[1:-1, 0], g[1:-1, -1], g[0, 1:-1], g[-1, 1:-1] = l1[0], l1[1], l1[2], l1[3]
                pads.append(P)
            F[:, b - 1], cfl, smax = box_flux_2d(pads, efld[b - 1], fc_field[b - 1], af.dr[b],
                                                 td, N_inv, lim, mob, q)
            cfl_max, sig_max = max(cfl_max, cfl.max()), max(sig_max, smax)
    for n in range(len(a)):
        inp.consistent_fluxes(af, F[n], cyl)
    lims = inp.limits(cfl_max, sig_max)
    return (F[0], a[0], lims) if single else (list(F), a, lims)

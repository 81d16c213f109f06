"""The 2-D species step with mobile ions, stated in numpy (test reference).

Written from the reference's formulas (src/m_fluid.f90:102-227, afivo/src/
m_af_flux_schemes.f90:320-430 and 666-848, m_af_ghostcell.f90:672-818,
m_af_core.f90:1257-1357), float64 operations in the order the Fortran writes
them (numpy neither reorders nor contracts them), so comparisons with the
library can be bitwise.

The flux species are the electrons (charge sign -1) and then the mobile ions.
For one box, from the padded cells of every flux species (`padded`: the box's
cells with both ghost layers of af_gc2_box):

  u_f       Koren-limited upwind value, upwind where q_n E_f > 0
  F_e       v u_e - dc / dx (n_R - n_L),  v = -mu_e E_f
  F_n       (q_n (mobility_n N_inv) E_f) u_n
  sigma_f   mu_e u_e, then + (mobility_n N_inv) u_n for n = 1 .. n_ions
  cfl       0 + x term + y term of the electrons alone
  update    y + dt/dx (rf1 F_i - rf2 F_{i+1}) + dt/dy (G_j - G_{j+1}) per species

Arrays follow the device layout: cell data (nc + 2, nc + 2) indexed [j, i] (i
fastest), face data (2, nc + 1, nc + 1) indexed [dim, j, i]; a padded box is
(nc + 4, nc + 4). Tree-wide arrays carry the box id - 1 first.
"""
import numpy as np

import cyl_numpy as cn

EPS0 = 8.8541878176e-12
ELEM_CHARGE = 1.6022e-19
NO_BOX = 0


# ------------------------------------------------------------------ limiters
def koren(a, b):
    """af_limiter_koren_t (m_af_limiters.f90): the branches in its order."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    third = 1 / 3.0
    aa, ab = a * a, a * b
    out = 2 * b
    out = np.where(aa <= 2.5 * ab, third * (b + 2 * a), out)
    out = np.where(aa <= 0.25 * ab, 2 * a, out)
    return np.where(ab <= 0, 0.0, out)


def mc(a, b):
    """af_limiter_gminmod with theta = 2 (the prolongation limiter of
    af_set_cc_methods in 2-D)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = np.minimum(np.minimum(np.abs(2.0 * a), np.abs(2.0 * b)), np.abs(0.5 * (a + b)))
    return np.where(a * b > 0, np.copysign(m, a), 0.0)


def lt_col(lt, col, x):
    """LT_get_col (m_lookup_table.f90:330-406); col is 1-based."""
    rc = np.asarray(lt["rows_cols"], np.float64)
    n = rc.shape[0]
    x = np.asarray(x, np.float64)
    frac = (x - float(lt["x_min"])) * float(lt["inv_fac"])
    low = np.where(frac <= 0, 1, np.where(frac >= n - 1, n - 1,
                                          np.ceil(np.clip(frac, 0, n - 1)))).astype(int)
    lf = np.where(frac <= 0, 1.0, np.where(frac >= n - 1, 0.0, low - frac))
    r = rc[:, col - 1]
    return lf * r[low - 1] + (1 - lf) * r[low]


# --------------------------------------------------------------- ghost cells
def _at(d, n, tg):
    """[j, i] of cell n along d with tangential index tg."""
    return (tg, n) if d == 0 else (n, tg)


def gc2_layers(af, a, b, lim=mc):
    """af_gc2_box of leaf b for the tree-wide array a (ghost layer 1 of the
    coarser leaves filled, as the level loop leaves them): (l1, l2), each
    (4, nc), neighbour nb - 1 first. Physical boundaries are Neumann 0."""
    nc = af.nc
    c = a[b - 1]
    l1, l2 = np.zeros((4, nc)), np.zeros((4, nc))
    for nb in range(4):
        d, low = nb >> 1, (nb & 1) == 0
        nid = af.neighbors[b][nb]
        for t in range(1, nc + 1):
            if nid > NO_BOX:
                cn_ = a[nid - 1]
                l1[nb, t - 1] = cn_[_at(d, nc if low else 1, t)]
                l2[nb, t - 1] = cn_[_at(d, nc - 1 if low else 2, t)]
            elif nid < NO_BOX:
                c0 = af.dr[b][d] * (-1 if low else 1)
                l1[nb, t - 1] = c0 * 0.0 + 1.0 * c[_at(d, 1 if low else nc, t)]
                l2[nb, t - 1] = (3 * c0) * 0.0 + 1.0 * c[_at(d, 2 if low else nc - 1, t)]
            else:
                # gc2_prolong_rb: limited slopes of the parent's neighbour
                hnc, td = nc // 2, 1 - d
                p = af.parent[b]
                cp = a[af.neighbors[p][nb] - 1]
                tc = ((af.ix[b][td] - 1) & 1) * hnc + ((t + 1) >> 1)
                n_ = nc if low else 1
                j, i = _at(d, n_, tc)
                f0 = cp[j, i]
                fx = 0.25 * lim(cp[j, i] - cp[j, i - 1], cp[j, i + 1] - cp[j, i])
                fy = 0.25 * lim(cp[j, i] - cp[j - 1, i], cp[j + 1, i] - cp[j, i])
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


def padded(af, a, b, lim=mc):
    """Box b with both ghost layers, (nc + 4, nc + 4) (corners zero: no flux
    reads them)."""
    nc = af.nc
    l1, l2 = gc2_layers(af, a, b, lim)
    P = np.zeros((nc + 4, nc + 4))
    P[2:-2, 2:-2] = a[b - 1][1:-1, 1:-1]
    P[2:-2, 1], P[2:-2, 0] = l1[0], l2[0]
    P[2:-2, nc + 2], P[2:-2, nc + 3] = l1[1], l2[1]
    P[1, 2:-2], P[0, 2:-2] = l1[2], l2[2]
    P[nc + 2, 2:-2], P[nc + 3, 2:-2] = l1[3], l2[3]
    return P


# --------------------------------------------------------------------- fluxes
def upwind_faces(lines, positive):
    """reconstruct_upwind_1d with Koren: lines (n, nc + 4) along the flux
    dimension, positive (n, nc + 1) -> face values (n, nc + 1)."""
    n = lines.shape[1] - 4
    LL, L, R, RR = (lines[:, k:k + n + 1] for k in range(4))
    return np.where(positive, L + 0.5 * koren(R - L, L - LL), R - 0.5 * koren(R - L, RR - R))


def _lines(P, d, lo, hi):
    """Rows lo:hi of P (d = 0) or of its transpose (d = 1)."""
    return (P if d == 0 else P.T)[lo:hi, :]


def box_fluxes(pads, E, Ef, dr, td, N_inv, mob, q):
    """The fluxes of one box. pads (1 + n_ions, nc + 4, nc + 4); E (nc + 2,
    nc + 2) the cell-centred |E|; Ef (2, nc + 1, nc + 1) the face field; mob
    (n_ions,) the mobilities as the descriptor carries them; q (1 + n_ions,)
    the charge signs, q[0] = -1. Returns F (1 + n_ions, 2, nc + 1, nc + 1)
    (entries no face owns stay zero), the cell CFL sums (nc, nc), sigma per
    face [(nc, nc + 1) per dimension] and its terms per species."""
    nsp = len(pads)
    nc = pads[0].shape[0] - 4
    nf = nc + 1
    F = np.zeros((nsp, 2, nf, nf))
    cfl = np.zeros((nc, nc))
    sigma, terms = [], []
    for d in range(2):
        idx = 1 / dr[d]
        El = _lines(E, d, 1, nc + 1)
        ex = Ef[0][0:nc, :] if d == 0 else Ef[1][:, 0:nc].T
        tfc = 0.5 * (El[:, 0:nf] + El[:, 1:nf + 1]) * 1e21 * N_inv
        mu = lt_col(td, 1, tfc) * N_inv
        dc = lt_col(td, 2, tfc) * N_inv
        v = -mu * ex
        ne = _lines(pads[0], d, 2, nc + 2)
        u = upwind_faces(ne, q[0] * ex > 0)
        flux = [v * u - dc * idx * (ne[:, 2:nf + 2] - ne[:, 1:nf + 1])]
        sig = mu * u
        tm = [mu * u]
        term = (1.0 * np.maximum(np.abs(v[:, 1:]), np.abs(v[:, :-1])) * idx +
                2 * np.maximum(dc[:, 1:], dc[:, :-1]) * (idx * idx))
        cfl = cfl + (term if d == 0 else term.T)
        for n in range(1, nsp):
            mu_n = mob[n - 1] * N_inv
            un = upwind_faces(_lines(pads[n], d, 2, nc + 2), q[n] * ex > 0)
            flux.append((q[n] * mu_n * ex) * un)
            sig = sig + mu_n * un
            tm.append(mu_n * un)
        for n in range(nsp):
            if d == 0:
                F[n, 0, 0:nc, :] = flux[n]
            else:
                F[n, 1, :, 0:nc] = flux[n].T
        sigma.append(sig)
        terms.append(tm)
    return F, cfl, sigma, terms


def limits(cfl_max, sigma_max):
    """dt_lim of flux_upwind_tree: 1 / max CFL sum, the dielectric relaxation
    time of the largest per-face conductivity."""
    return 1 / cfl_max, EPS0 / (ELEM_CHARGE * max(sigma_max, 1e-100))


def face_valid(nc):
    """(2, nc + 1, nc + 1) booleans: the entries a face owns."""
    m = np.zeros((2, nc + 1, nc + 1), bool)
    m[0, 0:nc, :] = True
    m[1, :, 0:nc] = True
    return m


def consistent_fluxes(af, F, cyl):
    """af_consistent_fluxes on the tree-wide face array F (boxes, 2, nf, nf),
    in place: a leaf's face next to a refined box is the mean of the two fine
    faces, on faces normal to z of a cylindrical tree with the coarse box's
    child weights."""
    nc = af.nc
    nch = nc // 2
    adj = ((1, 3), (2, 4), (1, 2), (3, 4))
    cdix = ((0, 0), (1, 0), (0, 1), (1, 1))
    for p in range(1, af.highest_id + 1):
        if not af.in_use[p] or not af.has_children(p):
            continue
        for nb in range(4):
            nid = af.neighbors[p][nb]
            if nid <= NO_BOX or af.has_children(nid):
                continue
            d, low = nb >> 1, (nb & 1) == 0
            i, i_nb = (1, nc + 1) if low else (nc + 1, 1)
            for i_ch in adj[nb]:
                fc, fn = F[af.children[p][i_ch - 1] - 1, d], F[nid - 1, d]
                for n in range(1, nch + 1):
                    if d == 0:
                        jn = nch * cdix[i_ch - 1][1] + n
                        fn[jn - 1, i_nb - 1] = 0.5 * (fc[2 * n - 2, i - 1] + fc[2 * n - 1, i - 1])
                    else:
                        i_n = nch * cdix[i_ch - 1][0] + n
                        f1, f2 = fc[i - 1, 2 * n - 2], fc[i - 1, 2 * n - 1]
                        if cyl:
                            w1, w2 = cn.child_weights(af.r_min[nid][0], af.dr[nid][0], i_n)
                            fn[i_nb - 1, i_n - 1] = 0.5 * (w1 * f1 + w2 * f2)
                        else:
                            fn[i_nb - 1, i_n - 1] = 0.5 * (f1 + f2)
    return F


# --------------------------------------------------------------------- update
def add_divergence(y, F, dt, dr, r_min=None):
    """flux_update_densities' divergence of one box and one flux species: y
    (nc, nc) [j, i] the value after the source terms, F (2, nc + 1, nc + 1).
    r_min: the box's r_min(1) on a cylindrical tree (af_cyl_flux_factors on
    the r faces), None on a Cartesian one."""
    nc = y.shape[0]
    dtx, dty = dt / dr[0], dt / dr[1]
    Fx, Fy = F[0][0:nc, :], F[1][:, 0:nc]
    if r_min is None:
        return y + dtx * (Fx[:, 0:nc] - Fx[:, 1:nc + 1]) + dty * (Fy[0:nc, :] - Fy[1:nc + 1, :])
    rf1, rf2 = cn.flux_factors(r_min, dr[0], nc)
    return (y + dtx * (rf1[None, :] * Fx[:, 0:nc] - rf2[None, :] * Fx[:, 1:nc + 1]) +
            dty * (Fy[0:nc, :] - Fy[1:nc + 1, :]))

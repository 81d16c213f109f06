"""The species update with the flux-based source factor, stated in numpy
(test reference; fixes%source_factor = flux).

Written from the reference's text (add_source_terms and
compute_source_factor, src/m_fluid.f90:298-466 and 525-583; get_rates and
get_derivatives, src/m_chemistry.f90:565-688; flux_update_densities,
afivo/src/m_af_flux_schemes.f90:320-436), float64 operations in the order the
Fortran writes them, so comparisons can be bitwise. The electron face flux is
an input: the update reads it as flux_upwind_tree and af_consistent_fluxes
left it (tests take it from the C oracle, from tests/ions2d_numpy.py or from
the device).

Per interior cell of a leaf box:

    n    = max(n_e(s_deriv), 0)
    mu   = LT_get_col(td, mobility, field_Td) * N_inv
    fl   = 0.5 * NORM2([Fx(i) + Fx(i+1), Fy(j) + Fy(j+1) (, Fz(k) + Fz(k+1))])
    s    = (fl + 1e-9) / (1e-9 + n * mu * |E|);  min(1, s);  max(0, s)
    s    = 0 where n * min(dr)**3 < min_electrons (> 0)
    rate = rate * s for every ionization reaction, before the densities

NORM2 is the Fortran runtime's evaluation (afh.electrode.norm2: scaled by the
largest component), which scripts/make_srcfac_cases.py's stored factor
confirms bit for bit; sqrt(a*a + b*b + c*c) differs in the last bit for about
a third of the cells.

Arrays follow the device layout: cell data of a box (nc + 2,) * ndim indexed
[k, j, i] (i fastest), face data (ndim, (nc + 1,) * ndim) indexed [dim, k, j,
i]. Species are the plasma species in the fluid's order; with a variable gas
density the reactions index the gas species first (1 .. n_gas), as the driver
hands them to the library.
"""
import numpy as np

import cyl_numpy as cn
from afh import capi
from afh.electrode import norm2
from ions2d_numpy import lt_col

SMALL_FLUX = 1.0e-9
KB, EV = 1.3806503e-23, 1.6022e-19  # UC_boltzmann_const, UC_elec_volt


def centre_flux(F):
    """0.5 * NORM2 of the face sums of one box: F (ndim, (nc + 1,) * ndim)
    -> (nc,) * ndim."""
    nd = F.shape[0]
    nc = F.shape[1] - 1
    inner = [slice(0, nc)] * nd
    sums = []
    for d in range(nd):
        lo, hi = list(inner), list(inner)
        hi[nd - 1 - d] = slice(1, nc + 1)  # dimension d is axis nd - 1 - d
        sums.append(F[d][tuple(lo)] + F[d][tuple(hi)])
    return 0.5 * norm2(np.stack(sums, axis=-1))


def source_factor(ne, E, F, mu, dr, min_electrons=-1.0):
    """compute_source_factor and the threshold of add_source_terms: ne =
    max(n_e, 0) and E = |E| on the interior, F the box's electron face flux,
    mu the mobility (times N_inv) per cell, dr the box's spacings."""
    s = (centre_flux(F) + SMALL_FLUX) / (SMALL_FLUX + ne * mu * E)
    s = np.minimum(1.0, s)
    s = np.maximum(0.0, s)
    if min_electrons > 0:
        m = min(float(x) for x in dr)
        s = np.where(ne * (m * m * m) < min_electrons, 0.0, s)
    return s


def rate(r, chem, field, td=None, td_energy_col=0, Tg=300.0):
    """get_rates of one reaction (driver form) at the fields (Td)."""
    c0, c = r.get("rate_factor", 1.0), r.get("c", [])
    ty = r.get("rate_type", capi.RATE_TABULATED_FIELD)
    one = np.ones_like(field)
    if ty == capi.RATE_TABULATED_FIELD:
        return c0 * lt_col(chem, r["table_col"], field)
    if ty == capi.RATE_CONSTANT:
        return c0 * c[0] * one
    if ty == capi.RATE_LINEAR:
        return c0 * c[0] * (field - c[1])
    if ty == capi.RATE_EXP_V1:
        z = c[1] / (c[2] + field)
        return c0 * c[0] * np.exp(-(z * z))
    if ty == capi.RATE_EXP_V2:
        z = field / c[1]
        return c0 * c[0] * np.exp(-(z * z))
    if ty == capi.RATE_K1:
        Te = (2 * EV / (3 * KB)) * lt_col(td, td_energy_col, field)
        return c0 * c[0] * np.power(300 / Te, c[1])
    if ty == 13:  # AFH_RATE_K8
        return c0 * c[0] * np.power(300 / Tg, c[1]) * one
    raise NotImplementedError("rate type %d" % ty)


def update_box(prev, w_prev, der, E, F, dt, dr, reactions, chem, td, N, ionization=None,
               min_electrons=-1.0, e_index=0, last_step=True, dt_chemistry_nmin=-1.0,
               mask=None, photo=None, photo_s=0, Ng=None, gas_fractions=(), r_min=None,
               ions=(), td_energy_col=0, Tg=300.0):
    """One leaf box through flux_update_densities with add_source_terms.

    prev: [state][species] interior arrays; der: [species] interior arrays of
    state s_deriv; E: |E| on the interior; F: the electron face flux of the
    box; ionization: per-reaction flags, or None for no source factor; mask:
    interior booleans (True: updated) or None; photo: interior array added to
    the electrons and species slot photo_s; Ng: interior gas density (the
    reactions then index the gas species first); r_min: the box's r_min(1) on
    a cylindrical 2-D tree; ions: [(species slot, face flux)].
    Returns ([species] new interiors, the factor or None, the chemistry
    limit)."""
    ns = len(der)
    nd = F.shape[0]
    dens = [np.maximum(np.asarray(a, float), 0.0) for a in der]
    if Ng is None:
        N_inv = 1 / N
        field = 1e21 * N_inv * E
        all_dens = dens
    else:
        N_inv = 1 / Ng
        field = 1e21 * (E / Ng)
        all_dens = [np.maximum(f * Ng, 0.0) for f in gas_fractions] + dens
    nsrc = len(all_dens)
    derivs = [np.zeros_like(E) for _ in range(nsrc)]
    sfac = None
    src = mask is None or bool(np.any(mask))
    if ionization is not None:
        mu = lt_col(td, 1, field) * N_inv
        sfac = source_factor(dens[e_index], E, F, mu, dr, min_electrons)
    for n, r in enumerate(reactions):
        k = rate(r, chem, field, td, td_energy_col, Tg)
        if ionization is not None and ionization[n]:
            k = k * sfac
        prod = 1.0
        for ix in r["ix_in"]:
            prod = prod * all_dens[ix - 1]
        k = k * prod
        for ix in r["ix_in"]:
            derivs[ix - 1] = derivs[ix - 1] - k
        for ix, m in zip(r["ix_out"], r["mult_out"]):
            derivs[ix - 1] = derivs[ix - 1] + k * m
    lim = 1e100
    if last_step and src:
        eps = 1e-100
        for a, b in zip(all_dens, derivs):
            if dt_chemistry_nmin > 0:
                q = (a + dt_chemistry_nmin) / np.maximum(np.abs(b), eps)
            else:
                q = np.maximum(a, eps) / np.maximum(-b, eps)
            lim = min(lim, float(q.min()))
    pd = derivs[nsrc - ns:]
    if photo is not None:
        pd[e_index] = pd[e_index] + photo
        pd[photo_s] = pd[photo_s] + photo
    nc = E.shape[0]
    out = []
    for s in range(ns):
        y = 0.0
        for q, w in enumerate(w_prev):
            y = y + w * prev[q][s]
        base = y
        y = y + dt * pd[s]
        fluxes = [F] if s == e_index else [Fq for sl, Fq in ions if sl == s]
        for G in fluxes:
            if nd == 2:
                dtx, dty = dt / dr[0], dt / dr[1]
                Fx, Fy = G[0][0:nc, :], G[1][:, 0:nc]
                if r_min is None:
                    y = y + dtx * (Fx[:, 0:nc] - Fx[:, 1:nc + 1]) + \
                        dty * (Fy[0:nc, :] - Fy[1:nc + 1, :])
                else:
                    rf1, rf2 = cn.flux_factors(r_min, dr[0], nc)
                    y = y + dtx * (rf1[None, :] * Fx[:, 0:nc] - rf2[None, :] * Fx[:, 1:nc + 1]) + \
                        dty * (Fy[0:nc, :] - Fy[1:nc + 1, :])
            else:
                c = slice(0, nc)
                h = slice(1, nc + 1)
                y = y + (dt / dr[0]) * (G[0][c, c, c] - G[0][c, c, h]) + \
                    (dt / dr[1]) * (G[1][c, c, c] - G[1][c, h, c]) + \
                    (dt / dr[2]) * (G[2][c, c, c] - G[2][h, c, c])
        if mask is not None:
            y = np.where(mask, y, base)
        out.append(y)
    return out, (sfac if src else None), lim

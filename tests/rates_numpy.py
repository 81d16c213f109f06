"""The rate and J.E integrals of a species step, stated in numpy (test
reference; include/afivo_hip_rates.h).

Written from the reference's text: chemical_rates_box and sum_global_JdotE
(src/m_fluid.f90:665-731) with fc_inner_product (259-280) and
af_cyl_volume_cc (afivo/src/m_af_types.f90:1176-1182). The per-cell rates are
those of tests/srcfac_numpy.py (get_rates times the source factor times the
input densities, add_source_terms at m_fluid.f90:368-400).

Every cell of a leaf contributes one term per reaction (rate times the cell
volume) and one J.E term (inner product times the volume times
UC_elec_charge). The terms are summed with math.fsum, so the value the device
is held to is the exact sum of the restated terms, and the bound on the
difference follows from the terms alone:

    a sum of n terms in any order differs from the exact sum by at most
    (n - 1) u sum|x_i|, u = 2**-53; each term carries at most a few roundings
    of its own (the weight, product(dr), 1 ulp of pow / exp in the temperature
    rate forms):   bound = (n_cells + 8) * 2**-53 * sum|term|.

Arrays follow the device layout (tests/srcfac_numpy.py): cell data indexed
[k, j, i], face data [dim, k, j, i].
"""
import math

import numpy as np

import srcfac_numpy as sn
from ions2d_numpy import lt_col

ELEC_CHARGE = -1.6022e-19  # UC_elec_charge
TWO_PI = 2 * math.acos(-1.0)
U = 2.0 ** -53


def cell_rates(m, der, E, F, dr, factor=False, min_e=-1.0, Ng=None):
    """[reaction] the final rate per interior cell of one box: the rate
    coefficient, times the source factor for a flagged reaction (factor),
    times the input densities. m: a tests/state_srcfac.Model; der: [species]
    interiors of state s_deriv; E: |E|; F: the box's electron face flux."""
    dens = [np.maximum(np.asarray(a, float), 0.0) for a in der]
    if Ng is None:
        N_inv = 1 / m.N
        field = 1e21 * N_inv * E
        all_dens = dens
    else:
        N_inv = 1 / Ng
        field = 1e21 * (E / Ng)
        all_dens = [np.maximum(f * Ng, 0.0) for f in m.gas_fractions] + dens
    sfac = None
    if factor:
        mu = lt_col(m.td, 1, field) * N_inv
        sfac = sn.source_factor(dens[m.species_iv.index(m.i_electron)], E, F, mu, dr, min_e)
    out = []
    for n, r in enumerate(m.reactions):
        k = sn.rate(r, m.chem, field, m.td, m.td_energy_col, m.Tg)
        if factor and m.ionization[n]:
            k = k * sfac
        prod = 1.0
        for ix in r["ix_in"]:
            prod = prod * all_dens[ix - 1]
        out.append(k * prod)
    return out


def cell_volumes(dr, nc, ndim, r_min=None):
    """product(dr) per interior cell, or af_cyl_volume_cc(box, i) with r_min =
    the box's r_min(1) on a cylindrical tree."""
    v = float(dr[0]) * float(dr[1])
    if ndim == 3:
        v = v * float(dr[2])
    if r_min is None:
        return np.full((nc,) * ndim, v)
    i = np.arange(1, nc + 1)
    w = TWO_PI * (r_min + (i - 0.5) * dr[0]) * v
    return np.broadcast_to(w[None, :], (nc, nc)).copy()


def inner_product(Fa, Fb):
    """fc_inner_product of two face variables of one box, per interior cell:
    0.5 * sum over the low faces + 0.5 * (sum over the high faces)."""
    nd, nc = Fa.shape[0], Fa.shape[1] - 1
    inner = [slice(0, nc)] * nd
    lo_sum = hi_sum = None
    for d in range(nd):
        lo, hi = list(inner), list(inner)
        hi[nd - 1 - d] = slice(1, nc + 1)  # dimension d is axis nd - 1 - d
        pl = Fa[d][tuple(lo)] * Fb[d][tuple(lo)]
        ph = Fa[d][tuple(hi)] * Fb[d][tuple(hi)]
        lo_sum = pl if lo_sum is None else lo_sum + pl
        hi_sum = ph if hi_sum is None else hi_sum + ph
    return 0.5 * lo_sum + 0.5 * hi_sum


class Sums:
    """rates[n_reactions] and jdote: the exact sums of the terms; abs_rates,
    abs_jdote: the sums of their magnitudes; n_cells."""

    def __init__(self, rate_terms, je_terms, n_cells):
        self.rates = np.array([math.fsum(t) for t in rate_terms])
        self.abs_rates = np.array([math.fsum(np.abs(t)) for t in rate_terms])
        self.jdote = math.fsum(je_terms)
        self.abs_jdote = math.fsum(np.abs(je_terms))
        self.n_cells = n_cells

    def bounds(self):
        """(per reaction, J.E): (n_cells + 8) * 2**-53 * sum|term|."""
        k = (self.n_cells + 8) * U
        return k * self.abs_rates, k * self.abs_jdote


def tree_sums(m, dr, cc, F, Ef, s_deriv, boxes, factor=False, min_e=-1.0, lsf=None, Ng=None,
              r_min=None, cyl_weight=None, unmasked_only=False):
    """The sums over the leaf boxes `boxes`. m: a tests/state_srcfac.Model;
    dr {box: spacings} (or an AfTree, which also gives r_min); cc {iv:
    tree-wide array}; F, Ef: the tree-wide electron flux and face field; lsf:
    the update mask's level set -- a box without a cell lsf > 0 adds nothing,
    any other box all its cells; Ng: the tree-wide gas density or None.
    cyl_weight: True / False overrides m.cylindrical for the cell volume, and
    unmasked_only leaves the masked cells of every box out (both to show that
    the reference's choice matters: neither is what it does)."""
    if hasattr(dr, "dr"):
        dr, r_min = dr.dr, dr.r_min
    nd = m.ndim
    inner = (slice(1, -1),) * nd
    cyl = m.cylindrical if cyl_weight is None else cyl_weight
    rate_terms = [[] for _ in m.reactions]
    je_terms, n_cells = [], 0
    for b in boxes:
        if lsf is not None and not np.any(~(lsf[b - 1][inner] <= 0.0)):
            continue
        der = [cc[iv + s_deriv][b - 1][inner] for iv in m.species_iv]
        E = cc[m.i_efld][b - 1][inner]
        nc = E.shape[0]
        vol = cell_volumes(dr[b], nc, nd, r_min[b][0] if cyl else None)
        if unmasked_only and lsf is not None:
            vol = np.where(lsf[b - 1][inner] <= 0.0, 0.0, vol)
        rates = cell_rates(m, der, E, F[b - 1], dr[b], factor, min_e,
                           None if Ng is None else Ng[b - 1][inner])
        for n, k in enumerate(rates):
            rate_terms[n].append((k * vol).ravel())
        je_terms.append((inner_product(F[b - 1], Ef[b - 1]) * vol * ELEC_CHARGE).ravel())
        n_cells += nc ** nd
    cat = np.concatenate
    return Sums([cat(t) if t else np.zeros(0) for t in rate_terms],
                cat(je_terms) if je_terms else np.zeros(0), n_cells)

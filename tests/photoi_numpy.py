"""The Zheleznyak photoionization source in numpy (test infrastructure).

photoionization_rate_from_alpha (src/m_photoi.f90:232-270) with the table
location of LT_get_loc (m_lookup_table.f90), float64, every expression in the
Fortran's operand order, so a kernel that evaluates the same expressions
agrees bitwise:

    Td       = fld * 1e21 / gas_dens                       (SI_to_Townsend)
    frac     = (Td - x_min) * inv_fac
    frac <= 0      -> low = 1,     low_frac = 1
    frac >= n - 1  -> low = n - 1, low_frac = 0
    otherwise      -> low = ceil(frac), low_frac = low - frac
    col(Td)  = low_frac * y(low) + (1 - low_frac) * y(low + 1)
    tmp      = fld * mobility * alpha * n_e * coeff,  negative -> 0

with mobility = column 1 and alpha = column alpha_col of the transport table,
coeff = photoi_eta * quench_fac.
"""
import numpy as np


def lt_loc(x, x_min, inv_fac, n_points):
    """(low (1-based), low_frac) of LT_get_loc for array x."""
    x = np.asarray(x, np.float64)
    frac = (x - x_min) * inv_fac
    mid = np.ceil(frac)
    low = np.where(frac <= 0, 1.0, np.where(frac >= n_points - 1, float(n_points - 1), mid))
    lf = np.where(frac <= 0, 1.0, np.where(frac >= n_points - 1, 0.0, mid - frac))
    return low.astype(np.int64), lf


def lt_col(table, col, low, lf):
    """LT_get_col_at_loc: table (n_cols, n_points), col 1-based."""
    y = np.asarray(table[col - 1], np.float64)
    return lf * y[low - 1] + (1 - lf) * y[low]


def source(fld, n_e, gas_dens, x_min, inv_fac, table, alpha_col, coeff):
    """The source on cells with field strength fld and electron density n_e."""
    fld = np.asarray(fld, np.float64)
    Td = fld * 1e21 / gas_dens
    low, lf = lt_loc(Td, x_min, inv_fac, table.shape[1])
    alpha = lt_col(table, alpha_col, low, lf)
    mobility = lt_col(table, 1, low, lf)
    tmp = fld * mobility * alpha * n_e * coeff
    return np.where(tmp < 0, 0.0, tmp)

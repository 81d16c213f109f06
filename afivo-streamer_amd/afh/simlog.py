"""The text of the simulation log (output_log, src/m_output.f90:586-668) and
the merge of the field maxima (output_fld_maxima, 881-910): pure functions,
no device.
"""
import numpy as np

from . import electrode

# the header of m_output.f90:593-603, per NDIM
HEADER = {
    2: "it time dt v sum(n_e) sum(n_i) sum(charge) sum(J.E) max(E) x y max(n_e) x y "
       "max(E_r) x y min(E_r) voltage current_J.E current_displ ne_zmin ne_zmax "
       "max(Etip) x y wc_time n_cells min(dx) dt_cfl dt_diff dt_drt dt_chem highest(lvl)",
    3: "it time dt v sum(n_e) sum(n_i) sum(charge) sum(J.E) max(E) x y z max(n_e) x y z "
       "voltage current_J.E current_displ ne_zmin ne_zmax max(Etip) x y z wc_time "
       "n_cells min(dx) dt_cfl dt_diff dt_drt dt_chem highest(lvl)",
}
# n_reals of m_output.f90:617-623: the reals between `it` and n_cells
N_REALS = {2: 26, 3: 25}


def fortran_e(x, width=20, digits=8):
    """x as Fortran's E<width>.<digits>e3 edit descriptor writes it: a zero
    before the point, `digits` significant digits after it, a three-digit
    exponent, right-justified. '%.7e' has the same digits and rounding; the
    point moves one place and the exponent grows by one."""
    x = float(x)
    if not np.isfinite(x):
        s = "NaN" if np.isnan(x) else ("-Infinity" if x < 0 else "Infinity")
        return s.rjust(width)
    mant, exp = ("%.*e" % (digits - 1, x)).split("e")
    sign = "-" if mant.startswith("-") else ""
    d = mant.lstrip("-").replace(".", "")
    e = 0 if float(mant) == 0.0 else int(exp) + 1
    return ("%s0.%sE%s%03d" % (sign, d, "-" if e < 0 else "+", abs(e))).rjust(width)


def header_line(ndim):
    """The header as the reference leaves it in the file: the names, then the
    line end of its list-directed write of an empty string."""
    return HEADER[ndim] + " \n"


def format_row(ndim, row):
    """One row in (I6,<n>E20.8e3,I12,5E20.8e3,I3): it, the n_reals reals,
    n_cells, min(dx) and the four time-step limits, the highest level."""
    n = N_REALS[ndim]
    assert len(row) == n + 8, (len(row), n + 8)
    out = ["%6d" % int(row[0])]
    out += [fortran_e(x) for x in row[1:1 + n]]
    out.append("%12d" % int(row[1 + n]))
    out += [fortran_e(x) for x in row[2 + n:7 + n]]
    out.append("%3d" % int(row[7 + n]))
    return "".join(out)


def merge_maxima(coord_val, n_found, distance, threshold):
    """output_fld_maxima after analysis_get_maxima: n_found clipped to the
    stored rows, then from the end of the list every maximum closer than
    `distance` to an earlier one is merged into it (the larger value stays,
    the list's last row fills the gap), and the rows above the threshold are
    written. coord_val: (n, ndim + 1) rows of coordinates and value."""
    cv = np.array(coord_val, float)
    nd = cv.shape[1] - 1
    n_found = min(int(n_found), len(cv))
    for n in range(n_found, 0, -1):
        for i in range(1, n):
            if electrode.norm2((cv[i - 1, :nd] - cv[n - 1, :nd])[None])[0] < distance:
                if cv[i - 1, nd] < cv[n - 1, nd]:
                    cv[i - 1] = cv[n - 1]
                cv[n - 1] = cv[n_found - 1]
                n_found -= 1
                break
    cv = cv[:n_found]
    return cv[cv[:, nd] > threshold]

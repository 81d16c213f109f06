"""The reductions of include/afivo_hip_analysis.h and the rows built on them,
restated with numpy from the reference's Fortran (test infrastructure):

  reduce_fc       af_tree_max_fc / af_tree_min_fc with box_max_fc / box_min_fc
                  and af_reduction_loc (m_af_utils.f90:694-754, 803-952)
  zminmax         analysis_zmin_zmax_threshold (src/m_analysis.f90:81-149), as
                  written: a box's zmax entry uses its FIRST plane above
  max_region      analysis_max_var_region (src/m_analysis.f90:153-186)
  local_maxima    analysis_get_maxima (src/m_analysis.f90:23-78), in the fixed
                  order the libraries use: leaves in loop order, cells in
                  array order
  merge_maxima    the merge loop of output_fld_maxima (src/m_output.f90:881-902)
  log_columns     output_log's columns (src/m_output.f90:532-581, 632-666)

Arrays are the ones Tree.get_cc / get_fc return: cc[b - 1, (k,) j, i] with one
ghost layer, fc[b - 1, dim, (k,) j, i] over 1:nc+1. `leaves` is the list of
leaf ids in the reference's loop order (AfTree.leaves()); r_min and dr are
indexed by box id (AfTree.r_min, AfTree.dr, or dicts). Everything is float64
in the order the Fortran writes it; every result is a selection of stored
values or a cell-centre coordinate, so comparisons with the device are
bitwise.
"""
import numpy as np

from afh import electrode

HUGE = np.finfo(np.float64).max


def _loc(nd, b, q, shape):
    """af_loc_t as the libraries flatten it: (id, i, j, k), 1-based, k = 0 in
    2-D; q the C-order position in an array of `shape` ((k,) j, i)."""
    ix = np.unravel_index(int(q), shape)[::-1]
    return (int(b),) + tuple(int(x) + 1 for x in ix) + (0,) * (3 - nd)


def no_loc(nd):
    return (-1,) * (1 + nd) + (0,) * (3 - nd)


def _reduction_loc(leaves, box_fn, is_min, init, nd):
    """af_reduction_loc: a box replaces the running value when
    reduction(tmp, val) differs from val."""
    val, loc = init, no_loc(nd)
    for b in leaves:
        tmp, bloc = box_fn(b)
        new = min(tmp, val) if is_min else max(tmp, val)
        if abs(new - val) > 0:
            val, loc = tmp, bloc
    return float(val), loc


def reduce_fc(leaves, fc, nc, nd, dim, is_min):
    """dim 1-based. The range is 1:nc in every dimension but dim (1:nc+1)."""
    def box(b):
        sl = tuple(slice(0, nc + (1 if d == dim - 1 else 0)) for d in reversed(range(nd)))
        a = fc[b - 1, dim - 1][sl]
        q = np.argmin(a) if is_min else np.argmax(a)  # first in array order
        return a.ravel()[q], _loc(nd, b, q, a.shape)
    return _reduction_loc(leaves, box, is_min, (1 if is_min else -1) * (HUGE / 10), nd)


def zminmax(leaves, cc, r_min, dr, nc, nd, threshold, limits):
    out = [float(limits[0]), float(limits[1])]
    for b in leaves:
        a = cc[b - 1][(slice(1, -1),) * nd]  # a[n - 1]: plane n of the last dimension
        i = j = -1
        for n in range(1, nc + 1):
            if np.max(a[n - 1]) > threshold:
                if i == -1:
                    i = n
                j = n
        vec = [1e100, -1e100]
        if i != -1:
            vec[0] = r_min[b][nd - 1] + (i - 0.5) * dr[b][nd - 1]
        if j != -1:  # ix(NDIM) = i here too (m_analysis.f90:134)
            vec[1] = r_min[b][nd - 1] + (i - 0.5) * dr[b][nd - 1]
        out = [min(out[0], vec[0]), max(out[1], vec[1])]
    return float(out[0]), float(out[1])


def max_region(leaves, cc, r_min, dr, nc, nd, r0, r1):
    r0, r1 = np.asarray(r0, float)[:nd], np.asarray(r1, float)[:nd]

    def box(b):
        lo = np.asarray(r_min[b], float)[:nd]
        r_max = lo + nc * np.asarray(dr[b], float)[:nd]
        if np.any(lo > r1) or np.any(r_max < r0):
            return -1e100, no_loc(nd)
        a = cc[b - 1][(slice(1, -1),) * nd]
        q = np.argmax(a)
        return a.ravel()[q], _loc(nd, b, q, a.shape)
    return _reduction_loc(leaves, box, False, -1e100, nd)


def local_maxima(leaves, cc, r_min, dr, nc, nd, threshold):
    """Every maximum as a row (coordinates, value), leaves in loop order,
    cells in array order (i fastest)."""
    rows = []
    mid = (slice(1, -1),) * nd
    for b in leaves:
        a = cc[b - 1]
        val = a[mid]
        ge, gt = np.ones(val.shape, bool), np.zeros(val.shape, bool)
        for ax in range(nd):
            for sl in (slice(0, -2), slice(2, None)):
                nb = a[tuple(sl if d == ax else slice(1, -1) for d in range(nd))]
                ge &= val >= nb
                gt |= val > nb
        for ix in np.argwhere((val > threshold) & ge & gt):  # rows sorted (k,) j, i
            ijk = ix[::-1] + 1
            r = [r_min[b][d] + (ijk[d] - 0.5) * dr[b][d] for d in range(nd)]
            rows.append(r + [val[tuple(ix)]])
    return np.array(rows, float).reshape(len(rows), nd + 1)


def merge_maxima(coord_val, n_found, distance, threshold):
    """output_fld_maxima after the call: n_found clipped to the stored rows,
    maxima closer than `distance` merged from the end of the list, the rows
    above the threshold kept. coord_val: (n, nd + 1)."""
    cv = np.array(coord_val, float)
    nd = cv.shape[1] - 1
    n_found = min(int(n_found), len(cv))
    for n in range(n_found, 0, -1):
        for i in range(1, n):
            d = float(electrode.norm2((cv[i - 1, :nd] - cv[n - 1, :nd])[None])[0])
            if d < distance:
                if cv[i - 1, nd] < cv[n - 1, nd]:
                    cv[i - 1] = cv[n - 1]
                cv[n - 1] = cv[n_found - 1]
                n_found -= 1
                break
    cv = cv[:n_found]
    return cv[cv[:, nd] > threshold]


def r_loc(loc, r_min, dr, nd):
    """af_r_loc: r_min + (ix - 0.5) dr of the located box (a face location
    too)."""
    b = loc[0]
    return [float(r_min[b][d] + (loc[1 + d] - 0.5) * dr[b][d]) for d in range(nd)]


def log_columns(leaves, cc_e, cc_E, fc_E, r_min, dr, nc, nd, origin, length, threshold):
    """The columns of output_log that come from the new reductions and the
    located extrema, as a dict: max(E) and max(n_e) with their places, max /
    min E_r (2-D), ne_zmin / ne_zmax, max(Etip) and r_tip."""
    def cc_max(cc):
        def box(b):
            a = cc[b - 1][(slice(1, -1),) * nd]
            q = np.argmax(a)
            return a.ravel()[q], _loc(nd, b, q, a.shape)
        return _reduction_loc(leaves, box, False, -HUGE / 10, nd)

    out = {}
    mx, loc = cc_max(cc_E)
    out["max(E)"], out["r(E)"] = mx, r_loc(loc, r_min, dr, nd)
    mx, loc = cc_max(cc_e)
    out["max(n_e)"], out["r(n_e)"] = mx, r_loc(loc, r_min, dr, nd)
    if nd == 2:
        mx, loc = reduce_fc(leaves, fc_E, nc, nd, 1, False)
        out["max(E_r)"], out["r(E_r)"] = mx, r_loc(loc, r_min, dr, nd)
        out["min(E_r)"] = reduce_fc(leaves, fc_E, nc, nd, 1, True)[0]
    z = zminmax(leaves, cc_e, r_min, dr, nc, nd, threshold, [length[nd - 1], 0.0])
    out["ne_zmin"], out["ne_zmax"] = z
    r0 = np.array(origin, float)
    r1 = np.array(origin, float) + np.array(length, float)
    k = nd - 1
    if z[0] - origin[k] < origin[k] + length[k] - z[1]:
        r0[k] = z[1] - 0.02 * length[k]
        r1[k] = z[1] + 0.02 * length[k]
    else:
        r0[k] = z[0] - 0.02 * length[k]
        r1[k] = z[0] + 0.02 * length[k]
    mx, loc = max_region(leaves, cc_E, r_min, dr, nc, nd, r0, r1)
    out["max(Etip)"] = mx
    out["r(Etip)"] = r_loc(loc, r_min, dr, nd) if loc[0] > 0 else [0.0] * nd
    return out

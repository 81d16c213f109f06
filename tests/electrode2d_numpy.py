"""The 2-D electrode kernels' formulas in numpy (test infrastructure).

Each function states what one kernel of libafivo_hip_2d.so computes for a box
with a variable (level-set) stencil, in float64 and in the operand order of
the reference's NDIM == 2 code, so that the device results can be compared
bitwise. Box images are [j][i] arrays of (nc + 2)^2 cells (ghost cells
included); v is the box's stencil [j][i][5] over cells 1..nc in the order
(i,j), (i-1,j), (i+1,j), (i,j-1), (i,j+1) and b its bc_correction [j][i]
(or None), as afh.electrode.boxes_operators returns them.
"""
import numpy as np


def _nb(p):
    """phi at the cell and its four neighbours over the interior."""
    return (p[1:-1, 1:-1], p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1])


def apply_v(phi, v):
    """stencil_apply_357, variable branch (m_af_stencil.f90:433-441)."""
    c, xl, xh, yl, yh = _nb(phi)
    return v[..., 0] * c + v[..., 1] * xl + v[..., 2] * xh + v[..., 3] * yl + v[..., 4] * yh


def residual_v(phi, rhs, v, b):
    """residual_box: rhs - (L phi - bc_correction) over the interior
    (k2_residual<StVar>)."""
    a = apply_v(phi, v)
    if b is not None:
        a = a - b
    return rhs[1:-1, 1:-1] - a


def rhs_roundtrip(rhs, b, n=1):
    """The rhs after n half-sweeps: (rhs + bc_correction) - bc_correction on
    every interior cell each time (m_af_stencil.f90:838-841, 975-978)."""
    r = rhs.copy()
    if b is not None:
        for _ in range(n):
            r[1:-1, 1:-1] = (r[1:-1, 1:-1] + b) - b
    return r


def gsrb_v(phi, rhs, v, b, redblack):
    """stencil_gsrb_357, variable branch, in place on phi and rhs (k2_gsrb_v):
    the cells i = i0, i0 + 2, .. with i0 = 2 - iand(ieor(redblack, j), 1)."""
    nc = phi.shape[0] - 2
    r1 = rhs[1:-1, 1:-1] + b if b is not None else rhs[1:-1, 1:-1].copy()
    for j in range(1, nc + 1):
        i0 = 2 - ((redblack ^ j) & 1)
        for i in range(i0, nc + 1, 2):
            c = v[j - 1, i - 1]
            phi[j, i] = (r1[j - 1, i - 1] - c[1] * phi[j, i - 1] - c[2] * phi[j, i + 1] -
                         c[3] * phi[j - 1, i] - c[4] * phi[j + 1, i]) / c[0]
    if b is not None:
        rhs[1:-1, 1:-1] = r1 - b


def lpl_coef(dr, lam=0.0):
    """mg_box_lpl_stencil: c(2:5) = 1 / dr^2, c(1) = -sum(c(2:)) - lambda."""
    c = np.zeros(5)
    c[1] = c[2] = 1 / (dr[0] * dr[0])
    c[3] = c[4] = 1 / (dr[1] * dr[1])
    c[0] = -(((c[1] + c[2]) + c[3]) + c[4]) - lam
    return c


def apply_c(phi, c):
    """stencil_apply_357, constant branch."""
    p, xl, xh, yl, yh = _nb(phi)
    return c[0] * p + c[1] * xl + c[2] * xh + c[3] * yl + c[4] * yh


def gsrb_c(phi, rhs, c, redblack):
    """stencil_gsrb_357, constant branch, in place on phi (k2_gsrb)."""
    nc = phi.shape[0] - 2
    inv_c1 = 1 / c[0]
    for j in range(1, nc + 1):
        i0 = 2 - ((redblack ^ j) & 1)
        for i in range(i0, nc + 1, 2):
            phi[j, i] = (rhs[j, i] - c[1] * phi[j, i - 1] - c[2] * phi[j, i + 1] -
                         c[3] * phi[j - 1, i] - c[4] * phi[j + 1, i]) * inv_c1


def fill_sides(boxes, neighbors, bc):
    """af_gc_box's side ghost cells of a level without refinement boundaries,
    in place: boxes {id: image}, neighbors {id: (lowx, highx, lowy, highy)}
    (> 0: a box of the level, else a physical boundary), bc four (kind,
    value) with kind 'd' (Dirichlet: 2 value - first cell) or 'n' (Neumann
    with value 0: the first cell). Every value read is an interior cell."""
    new = {}
    for b, p in boxes.items():
        g = {}
        for nb in range(4):
            q = neighbors[b][nb]
            if q > 0:
                o = boxes[q]
                g[nb] = (o[1:-1, -2], o[1:-1, 1], o[-2, 1:-1], o[1, 1:-1])[nb].copy()
            else:
                first = (p[1:-1, 1], p[1:-1, -2], p[1, 1:-1], p[-2, 1:-1])[nb]
                kind, val = bc[nb]
                g[nb] = 2 * val - first if kind == "d" else first.copy()
        new[b] = g
    for b, p in boxes.items():
        p[1:-1, 0], p[1:-1, -1], p[0, 1:-1], p[-1, 1:-1] = (new[b][0], new[b][1], new[b][2],
                                                            new[b][3])


def rstr_fas_v(phi, rhs, v, b):
    """update_coarse for a child with a variable stencil (k2_rstr_fas<StVar>): the
    restricted residual and phi, (nc/2)^2 each: 0.25 * sum(cc(i_f:i_f+1,
    j_f:j_f+1)) in column-major section order."""
    res = residual_v(phi, rhs, v, b)
    p = phi[1:-1, 1:-1]

    def r4(a):
        return 0.25 * (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2])
    return r4(res), r4(p)


def parent_rhs_v(phi, rhs, tmp, v, b):
    """rhs = L phi + tmp (L phi - bc_correction on the interior, the old rhs
    on the ghost cells), tmp = phi over the whole block (k2_parent_rhs<StVar>)."""
    r = rhs.copy()
    a = apply_v(phi, v)
    if b is not None:
        a = a - b
    r[1:-1, 1:-1] = a
    return r + tmp, phi.copy()


def lpl_gradient(phi, dr, fac):
    """mg_box_lpl_gradient: fc [2][j][i] over faces 1..nc+1."""
    nc = phi.shape[0] - 2
    fc = np.zeros((2, nc + 1, nc + 1))
    fc[0, :nc, :] = (fac / dr[0]) * (phi[1:-1, 1:] - phi[1:-1, :-1])
    fc[1, :, :nc] = (fac / dr[1]) * (phi[1:, 1:-1] - phi[:-1, 1:-1])
    return fc


def lsf_gradient(phi, lsf, fc, ix, dd, bval, dr, fac):
    """mg_box_lpllsf_gradient, NDIM == 2 (m_af_multigrid.f90:2068-2087): the
    serial loop over the distance list, in place on fc [2][j][i]; a face two
    entries write keeps the later entry's value."""
    inv = (fac / dr[0], fac / dr[1])
    for n in range(len(ix)):
        i, j = int(ix[n][0]), int(ix[n][1])
        d = dd[n]
        if not lsf[j, i] >= 0:
            continue
        pc, bc = phi[j, i], bval[j - 1, i - 1]
        if d[0] < 1:
            fc[0, j - 1, i - 1] = inv[0] * (pc - bc) / d[0]
        if d[1] < 1:
            fc[0, j - 1, i] = inv[0] * (bc - pc) / d[1]
        if d[2] < 1:
            fc[1, j - 1, i - 1] = inv[1] * (pc - bc) / d[2]
        if d[3] < 1:
            fc[1, j, i - 1] = inv[1] * (bc - pc) / d[3]


def field_norm(fc):
    """mg_box_field_norm (2009-2014) over the interior."""
    nc = fc.shape[1] - 1
    sx = fc[0, :nc, :nc] + fc[0, :nc, 1:]
    sy = fc[1, :nc, :nc] + fc[1, 1:, :nc]
    return 0.5 * np.sqrt(sx * sx + sy * sy)


def electrode_species_bc(species, ne, ion, lsf, neumann_zero):
    """electrode_species_bc, NDIM == 2 (src/streamer.f90:578-636), in place:
    species a list of box images (the electrons and the first positive ion
    among them), every one zeroed where lsf < 0; with neumann_zero the
    electrons there get the mean over the neighbours with lsf > 0 (in the
    order i-1, i+1, j-1, j+1), copied to the ion."""
    nc = lsf.shape[0] - 2
    ne0 = ne.copy()  # (a cell with lsf < 0 never reads another such cell)
    for j in range(1, nc + 1):
        for i in range(1, nc + 1):
            if not lsf[j, i] < 0:
                continue
            for s in species:
                s[j, i] = 0.0
            if not neumann_zero:
                continue
            nb = [(j, i - 1), (j, i + 1), (j - 1, i), (j + 1, i)]
            cnt, sm = 0, 0.0
            for q in nb:
                if lsf[q] > 0:
                    cnt += 1
                    sm = sm + ne0[q]
            if cnt > 0:
                ne[j, i] = sm / cnt
                ion[j, i] = ne[j, i]


def update_mask(lsf):
    """set_box_mask (src/m_fluid.f90:469-483) over the interior: True where
    the cell is updated."""
    return ~(lsf[1:-1, 1:-1] <= 0.0)


def refine_electrode(flags, electrode_box, max_dx, electrode_dx, limited, forced, do_ref=1,
                     keep_ref=0):
    """refine_electrode_dx (src/m_refine.f90:261-265) on top of the box flags
    default_refinement gives without it: every cell of a box tagged
    mg_lsf_box with max_dx > electrode_dx asks for refinement. The rules after
    it: a refinement region only adds requests; in a box a refine_limits
    entry covers (`limited`), every request becomes af_keep_ref (282-289); a
    box with max_dx > refine_max_dx (`forced`) asks for refinement whatever
    came before (291-293); the refine_min_dx rule (294-296) is taken not to
    apply (the caller checks)."""
    out = np.array(flags).copy()
    hit = (np.asarray(electrode_box) != 0) & (np.asarray(max_dx) > electrode_dx)
    limited, forced = np.asarray(limited, bool), np.asarray(forced, bool)
    out[hit & ~limited] = do_ref
    out[hit & limited] = keep_ref
    out[forced] = do_ref
    return out

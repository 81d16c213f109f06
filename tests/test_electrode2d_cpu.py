"""Electrodes in the 2-D library: the host half (no GPU).

* afh.electrode in 2-D against its 3-D path, which tests/test_electrode_ops.py
  pins to the reference's own stencils (the rod8 fixture): the rod of
  programs/standard_2d/tests/test_2d_pos_electrode.cfg extruded along z,
  f3(x, y, z) = f2(x, y), has on every z-plane the 2-D problem's boundary
  distances, so the tagged boxes, ix, dd[:, :4], v[..., 1:5] and f_bc must be
  equal -- compared with tolerance 0.
* the four electrode fixtures (scripts/make_electrode2d_cases.py).
* tests/electrode2d_numpy.py, the statements the GPU tests compare with,
  against each other.
"""
import numpy as np
import pytest

import electrode2d_numpy as en
import golden
from afh import electrode

CASES = ["test_2d_pos_electrode", "test_2d_neg_electrode",
         "test_2d_pos_electrode_photoi", "test_2d_neg_electrode_photoi"]


class Extruded:
    """f3(x, y, z) = f2(x, y)."""

    def __init__(self, f2):
        self.f2, self.length_scale = f2, f2.length_scale

    def __call__(self, r):
        return self.f2(np.asarray(r, float)[..., :2])


def _rod():
    d = golden.load("rtest_test_2d_pos_electrode")
    L, o = np.asarray(d["domain_len"], float), np.asarray(d["domain_origin"], float)
    r0 = o + np.asarray(d["field_rod_r0"], float) * L
    r1 = o + np.asarray(d["field_rod_r1"], float) * L
    return electrode.RodLSF(r0, r1, float(d["field_rod_radius"][0])), L


def _boxes():
    """8-cell boxes at two levels around the rod (16 mm, 0 .. 4.8 mm, radius
    1 mm): level 1 (dr = 4 mm > radius: the search along the gradient) and
    level 5 (dr = 0.25 mm) boxes over the shaft, the tip and away from it."""
    f2, L = _rod()
    nc = 8
    out = [(np.zeros(2), L / nc)]
    dr5 = L / nc / 16
    for a in (6, 7, 8, 9):
        for b in (0, 1, 2, 3):
            out.append((np.array([a, b]) * nc * dr5, dr5))
    out.append((np.array([2, 9]) * nc * dr5, dr5))  # far from the rod
    return f2, nc, out


def test_boxes_operators_2d_equals_3d_plane():
    f2, nc, geo = _boxes()
    f3 = Extruded(f2)
    b2, b3 = [], []
    for r_min, dr in geo:
        lsf2 = f2(electrode.cell_centers(r_min, dr, nc))
        b2.append((lsf2, r_min, dr))
        rm3, dr3 = np.append(r_min, 3 * dr[0]), np.append(dr, dr[0])
        lsf3 = f3(electrode.cell_centers(rm3, dr3, nc))
        assert np.array_equal(lsf3[3], lsf2)
        b3.append((lsf3, rm3, dr3))
    o2 = electrode.boxes_operators(f2, b2, nc, 1.0)
    o3 = electrode.boxes_operators(f3, b3, nc, 1.0)
    assert [o is None for o in o2] == [o is None for o in o3]
    assert o2[0] is not None and o2[-1] is None
    assert sum(o is not None for o in o2) >= 6 and sum(o is None for o in o2) >= 2
    # the level-1 box took the search along the gradient line
    assert np.min(geo[0][1]) > f2.length_scale
    n_cmp = 0
    for a, b in zip(o2, o3):
        if a is None:
            continue
        v2, f2b, ix2, dd2 = a
        v3, f3b, ix3, dd3 = b
        assert v2.shape == (nc, nc, 5) and f2b.shape == (nc, nc)
        assert ix2.shape[1] == 2 and dd2.shape[1] == 4
        for k in range(nc):  # any z-plane
            sel = ix3[:, 2] == k + 1
            assert np.array_equal(ix3[sel][:, :2], ix2)
            assert np.array_equal(dd3[sel][:, :4], dd2)
            assert np.all(dd3[sel][:, 4:] == 1.0)
            assert np.array_equal(v3[k][..., 1:5], v2[..., 1:5])
            assert np.array_equal(f3b[k], f2b)
        # (the centre is -sum(v(2:)) before the boundary entries are zeroed:
        # the 3-D one has the two z terms more)
        assert np.all(v2[..., 0] < 0)
        n_cmp += len(ix2)
    assert n_cmp > 50


def test_3d_helpers_unchanged_shapes():
    """cell_centers / numerical_gradient keep their 3-D layout."""
    r = electrode.cell_centers(np.zeros(3), np.array([1.0, 2.0, 3.0]), 2)
    assert r.shape == (2, 2, 2, 3)
    assert np.array_equal(r[1, 0, 1], [1.5, 1.0, 4.5])
    r2 = electrode.cell_centers(np.zeros(2), np.array([1.0, 2.0]), 2, 0, 3)
    assert r2.shape == (4, 4, 2) and np.array_equal(r2[0, 3], [2.5, -1.0])


@pytest.mark.parametrize("name", CASES)
def test_electrode_fixtures(name):
    d = golden.load("rtest_" + name)
    assert len(d["coarse_grid_size_value"]) == 2
    assert len(d["field_rod_r0"]) == 2 and len(d["field_rod_r1"]) == 2
    assert int(d["use_electrode"][0]) == 1
    assert d["rtest_log"].shape == (11, 12)
    assert bool(int(d["photoi%enabled"][0])) == name.endswith("photoi")


def _rand_box(seed, nc=8):
    rng = np.random.default_rng(seed)
    ng = nc + 2
    v = rng.uniform(0.5, 2.0, (nc, nc, 5))
    v[..., 0] = -(((v[..., 1] + v[..., 2]) + v[..., 3]) + v[..., 4])
    return (rng.standard_normal((ng, ng)), rng.standard_normal((ng, ng)), v,
            rng.standard_normal((nc, nc)))


def test_numpy_statements_consistent():
    """A half sweep solves its cells' equations, leaves the others, and its
    rhs is the round trip; the restricted residual is the mean of
    residual_v; parent_rhs_v's interior is L phi - b + tmp."""
    phi, rhs, v, b = _rand_box(3)
    for rb in (1, 2):
        p, r = phi.copy(), rhs.copy()
        en.gsrb_v(p, r, v, b, rb)
        assert np.array_equal(r, en.rhs_roundtrip(rhs, b))
        j, i = np.meshgrid(np.arange(1, 9), np.arange(1, 9), indexing="ij")
        swept = ((i + j + rb) % 2) == 0
        assert np.array_equal(p[1:-1, 1:-1][~swept], phi[1:-1, 1:-1][~swept])
        res = en.residual_v(p, rhs, v, b)
        assert np.max(np.abs(res[swept])) < 1e-12 * np.max(np.abs(v))
        assert np.max(np.abs(res[~swept])) > 1e-3
    rr, rp = en.rstr_fas_v(phi, rhs, v, b)
    assert rr.shape == (4, 4)
    assert rr[1, 2] == 0.25 * sum([en.residual_v(phi, rhs, v, b)[2 + dj, 4 + di]
                                   for dj in (0, 1) for di in (0, 1)][k] for k in (0, 1, 2, 3))
    tmp = np.ones_like(phi)
    r2, t2 = en.parent_rhs_v(phi, rhs, tmp, v, b)
    assert np.array_equal(r2[1:-1, 1:-1], (en.apply_v(phi, v) - b) + 1.0)
    assert np.array_equal(r2[0], rhs[0] + 1.0) and np.array_equal(t2, phi)


def test_numpy_gradient_later_entry_wins():
    nc = 4
    rng = np.random.default_rng(1)
    phi = rng.standard_normal((nc + 2, nc + 2))
    lsf = np.ones((nc + 2, nc + 2))
    lsf[2, 3] = -1.0
    fc = en.lpl_gradient(phi, (0.5, 0.25), -1.0)
    base = fc.copy()
    # cells (2,2) and (3,2) share the x-face 3 of row 2; (3,2) has lsf < 0
    ix = np.array([[2, 2], [1, 2], [3, 2]])
    dd = np.array([[0.5, 1, 1, 1], [1, 0.25, 1, 1], [1, 1, 0.5, 0.5]])
    bval = np.full((nc, nc), 2.0)
    en.lsf_gradient(phi, lsf, fc, ix, dd, bval, (0.5, 0.25), -1.0)
    # face (i=2, j=2): written by entry 0 (low face) then entry 1 (high face)
    assert fc[0, 1, 1] == (-1.0 / 0.5) * (2.0 - phi[2, 1]) / 0.25
    changed = np.argwhere(fc != base)
    assert [tuple(c) for c in changed] == [(0, 1, 1)]
    assert en.field_norm(fc).shape == (nc, nc)

"""Cylindrical (af_cyl) coordinates in the 2-D library: everything that needs
no GPU -- the fixtures, the host tree, the numpy statement of the operators
(tests/cyl_numpy.py) checked against identities of the discretisation, the
Fortran interfaces and the exported symbols."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import cyl_numpy as cn
import golden
import state2d
from afh import capi
from afh.amr import AF_CYL, AfTree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(REPO, "afivo-streamer_amd", "fortran")
FLANG = shutil.which("amdflang") or "/opt/rocm/llvm/bin/amdflang"
EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("name,n_species", [("rtest_test_cyl", 3), ("rtest_test_cyl_chem", None)])
def test_cyl_fixtures_are_2d_and_cylindrical(name, n_species):
    d = golden.load(name)
    assert len(d["coarse_grid_size_value"]) == 2
    assert int(d["cylindrical"][0]) == 1
    assert list(d["coarse_grid_size_value"]) == [8, 8]
    assert d["rtest_log"].ndim == 2 and d["rtest_log"].shape[0] >= 2
    assert float(d["domain_origin"][0]) == 0.0
    if n_species is not None:
        assert int(d["n_species"][0]) == n_species
    # photoionization off, the models the 2-D library runs
    assert int(d["photoi%enabled"][0]) == 0


def test_state2d_tree_has_the_cylindrical_edge_cases():
    """The AMR tree of tests/state2d.py starts on the axis and has coarse-fine
    faces normal to r and normal to z."""
    c, af, _, _, _ = state2d.build_state("test_2d")
    used = [b for b in range(1, af.highest_id + 1) if af.in_use[b]]
    assert af.nc == 8 and af.highest_lvl >= 3
    assert any(af.r_min[b][0] == 0.0 for b in used)
    refb = {nb for b in used for nb in range(4) if af.neighbors[b][nb] == 0}
    assert refb & {0, 1}, "no coarse-fine face normal to r"
    assert refb & {2, 3}, "no coarse-fine face normal to z"


def test_total_volume_cylindrical_is_pi_r2_l():
    R, L = 3e-3, 7e-3
    af = AfTree(8, [R, L], [16, 32], coord=AF_CYL)
    af.refine_up_to_lvl(3)
    assert af.coord == AF_CYL
    v = af.total_volume()
    assert abs(v - np.pi * R * R * L) <= 8 * EPS * v
    r_mins = [af.r_min[b][0] for b in af.lvls[1]["ids"]]
    assert v == cn.total_volume(r_mins, af.nc * af.dr_base)
    with pytest.raises(ValueError):
        AfTree(8, [R, L], [16, 32], coord=AF_CYL, r_min=[-1e-3, 0.0])
    with pytest.raises(ValueError):
        AfTree(8, [R, L], [16, 32], coord=AF_CYL, periodic=(True, False))


@pytest.mark.parametrize("r_min", [0.0, 8 * 1.3e-4, 40 * 1.3e-4])
def test_operator_on_r_squared_is_4(r_min):
    """(1/r) d/dr (r d(r^2)/dr) = 4: the flux form gives it exactly at every
    radius, the axis cell included (its inner factor is exactly 0)."""
    nc, dr = 8, (1.3e-4, 0.9e-4)
    c = cn.lpl_coef(dr)
    i = np.arange(0, nc + 2)
    r = r_min + (i - 0.5) * dr[0]
    p = np.tile(r * r, (nc + 2, 1))
    out = cn.apply(p, c, r_min, dr[0])
    scale = np.abs(c[0]) * np.max(r * r)
    assert np.max(np.abs(out - 4.0)) <= 16 * EPS * scale
    f1, _ = cn.flux_factors(r_min, dr[0], nc)
    if r_min == 0.0:
        assert f1[0] == 0.0
        assert cn.cyl_coef(c, r_min, dr[0], nc)[1][0] == 0.0


def test_restriction_with_geometry_preserves_the_weighted_sum():
    rng = np.random.default_rng(7)
    nc = 8
    for p_r_min, p_dr in ((0.0, 2e-4), (16e-4, 2e-4)):
        dr_c = 0.5 * p_dr
        parent = np.zeros((nc + 2, nc + 2))
        fine_sum = 0.0
        for ix in ((1, 1), (2, 1), (1, 2), (2, 2)):
            child = rng.uniform(0.5, 2.0, (nc + 2, nc + 2))
            c_r_min = p_r_min + (ix[0] - 1) * dr_c * nc
            cn.restrict(child, parent, ix, p_r_min, p_dr, geometry=True)
            fine_sum += (dr_c * dr_c) * cn.sum_2pr_box(child, c_r_min, dr_c)
        coarse_sum = (p_dr * p_dr) * cn.sum_2pr_box(parent, p_r_min, p_dr)
        # nc^2 / 2 additions per partial sum: a few eps
        assert abs(coarse_sum - fine_sum) <= 8 * EPS * abs(fine_sum)
        # without geometry it is the plain mean and does not
        plain = np.zeros_like(parent)
        cn.restrict(child, plain, (2, 2), p_r_min, p_dr, geometry=False)
        f = child[1:-1, 1:-1]
        assert np.array_equal(plain[5:9, 5:9],
                              0.25 * (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2]))


def test_gsrb_half_sweep_solves_its_cells():
    """After a half sweep the residual vanishes (to rounding) on the cells it
    updated and only there."""
    rng = np.random.default_rng(3)
    nc, dr, r_min = 8, (1e-4, 1e-4), 0.0
    c = cn.lpl_coef(dr)
    p = rng.standard_normal((nc + 2, nc + 2))
    rhs = rng.standard_normal((nc + 2, nc + 2)) * abs(c[0])
    cn.gsrb_half(p, rhs, c, r_min, dr[0], 1)
    res = cn.residual(p, rhs, c, r_min, dr[0])
    jj, ii = np.meshgrid(np.arange(1, nc + 1), np.arange(1, nc + 1), indexing="ij")
    upd = ((ii + jj) & 1) == 1
    assert np.max(np.abs(res[upd])) <= 64 * EPS * abs(c[0]) * np.max(np.abs(p))
    assert np.min(np.abs(res[~upd])) > 1e-6 * abs(c[0])


def test_update_divergence_and_consistent_flux_shapes():
    nc, dr = 8, (2e-4, 1e-4)
    F = np.ones((2, nc + 1, nc + 1))
    # a uniform unit flux: the z term cancels, the r term is dt/dr (f1 - f2) = -dt / r
    out = cn.update_divergence(F, 1e-12, 0.0, dr)
    r = cn.radius_cc(0.0, dr[0], nc)
    assert np.allclose(out, np.tile(-1e-12 / r, (nc, 1)), rtol=1e-14, atol=0)
    w1, w2 = cn.child_weights(0.0, dr[0], np.arange(1, nc + 1))
    assert np.all(w1 + w2 == 2.0)
    assert cn.consistent_zface(3.0, 3.0, 0.0, dr[0], 2) == 3.0


@pytest.mark.skipif(not os.path.exists(FLANG), reason="amdflang not in the image")
def test_fortran_2d_module_compiles(tmp_path):
    """m_afivo_hip_2d.F90 and INTEGRATION.md's cylindrical snippet against
    m_afivo_hip (no GPU, no link)."""
    srcs = [os.path.join(FDIR, "m_afivo_hip.F90"), os.path.join(FDIR, "m_afivo_hip_2d.F90"),
            os.path.join(REPO, "tests", "fortran", "cyl_coord.F90")]
    for src in srcs:
        pre = tmp_path / (os.path.basename(src)[:-4] + ".f90")
        with open(pre, "w") as out:
            subprocess.run(["cpp", "-traditional-cpp", "-P", src], stdout=out, check=True)
        r = subprocess.run([FLANG, "-c", str(pre), "-o", str(pre) + ".o"], cwd=tmp_path,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_coord_symbols_exported_and_bound():
    lib = ctypes.CDLL(capi.HIP_LIB_2D)
    for n in capi.SIGNATURES_2D:
        assert hasattr(lib, "afh_" + n), n
    h = capi.hip_library_2d()
    assert h.has("tree_set_coord") and h.has("tree_get_coord")
    # the 2-D-only entry points stay out of the common ABI and its header
    assert not set(capi.SIGNATURES_2D) & set(capi.SIGNATURES)
    assert not {"afh_" + n for n in capi.SIGNATURES_2D} & set(capi.header_symbols())
    decl = open(os.path.join(REPO, "include", "afivo_hip_2d_cyl.h")).read()
    for n in capi.SIGNATURES_2D:
        assert "afh_" + n + "(" in decl
    assert (capi.COORD_XYZ, capi.COORD_CYL) == (1, 2)


def test_driver_accepts_cylindrical_only_in_2d_with_pfmg():
    from afh.driver import Simulation
    lib = capi.hip_library_2d()
    d = golden.load("rtest_test_cyl")
    with pytest.raises(ValueError, match="COARSE_PFMG"):
        Simulation(lib, d)
    sim = Simulation(lib, d, coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
    assert sim.cylindrical and sim.af.coord == AF_CYL

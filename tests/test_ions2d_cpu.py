"""Mobile ions in the 2-D library, the parts that need no GPU: the fixtures of
programs/standard_2d/tests/test_cyl_ion_motion{,_v2}.cfg, the driver's set-up
of their ion list, and the numpy statement's own edge cases
(tests/ions2d_numpy.py)."""
import numpy as np
import pytest

import golden
import ions2d_numpy as inp
from afh import capi
from afh.driver import Case, Simulation

PFMG = dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)
CASES = ["rtest_test_cyl_ion_motion", "rtest_test_cyl_ion_motion_v2"]
# input_data%mobile_ions of both .cfg files, in their order
CFG_IONS = ["N2_plus", "N4_plus", "O2_plus", "O4_plus", "O2_min", "O_min"]


@pytest.mark.parametrize("name", CASES)
def test_fixture(name):
    g = golden.load(name)
    c = Case(g)
    assert len(c.ia("coarse_grid_size_value")) == 2
    assert c.i("cylindrical") == 1
    assert c.i("n_mobile_ions") == 6
    species, itree = list(c.sa("species_list")), list(c.ia("species_itree"))
    fs = list(c.ia("flux_species"))
    assert fs[0] == c.ia("ivars")[1] and len(fs) == 7
    assert [species[itree.index(iv)] for iv in fs[1:]] == CFG_IONS
    assert list(c.sa("fc_names"))[2:] == CFG_IONS
    sign = list(c.ia("flux_species_charge_sign"))
    assert sign[0] == -1 and set(sign[1:]) == {-1, 1}
    assert sign[1:] == [1 if s.endswith("plus") else -1 for s in CFG_IONS]
    assert c.r("ion_se_yield") == 0
    assert len(c.ra("ion_mobilities")) == 6 and (c.ra("ion_mobilities") > 0).all()
    assert g["rtest_log"].shape == (11, 27)


@pytest.mark.parametrize("name", CASES)
def test_driver_sets_up_the_ions(name):
    sim = Simulation(capi.hip_library_2d(), golden.load(name), **PFMG)
    assert sim.ndim == 2 and sim.cylindrical
    assert len(sim.ions) == 6
    fv = [f for _, f, _ in sim.ions]
    assert len(set(fv)) == 6 and sim.f_flux not in fv and sim.f_field not in fv
    assert all(1 <= f <= sim.n_var_face for f in fv)
    plasma_names = [sim.species_list[n] for n in sim.plasma]
    assert [plasma_names[sp - 1] for sp, _, _ in sim.ions] == CFG_IONS
    assert all(sim.species_itree[sim.plasma[sp - 1]] != sim.i_electron for sp, _, _ in sim.ions)
    # ion_mobilities * N, the reference's scaling: mu = mobility / N * N_0
    assert all(m > 0 for _, _, m in sim.ions)


# ------------------------------------------------------- the numpy statement
NC = 4
TD = {"x_min": 0.0, "inv_fac": 1.0 / 50.0,
      "rows_cols": np.stack([np.linspace(2e24, 1e24, 11), np.linspace(1e24, 3e24, 11)], axis=1)}
N_INV = 1 / 2.5e25


def _state(seed, n_ions=2):
    rng = np.random.default_rng(seed)
    pads = 1e15 * (0.5 + rng.random((1 + n_ions, NC + 4, NC + 4)))
    E = 1e6 * (1 + rng.random((NC + 2, NC + 2)))
    Ef = 1e6 * rng.standard_normal((2, NC + 1, NC + 1))
    mob = 1e22 * (1 + rng.random(n_ions))
    return pads, E, Ef, np.array([1e-4, 2e-4]), mob


def test_zero_field_gives_zero_ion_flux():
    pads, E, Ef, dr, mob = _state(1)
    F, cfl, sigma, _ = inp.box_fluxes(pads, E, 0.0 * Ef, dr, TD, N_INV, mob, [-1, 1, -1])
    assert not F[1:].any()
    # (the electrons still diffuse)
    assert F[0][inp.face_valid(NC)].any() and (cfl > 0).all()
    assert all((s > 0).all() for s in sigma)


def test_charge_sign_mirrors_the_upwind_side():
    """u_f of a species with charge q in the field E equals u_f of charge -q
    in -E; the two fluxes are then equal too (q E is the same), and differ
    from the flux with the other upwind side."""
    pads, E, Ef, dr, mob = _state(2, n_ions=1)
    both = np.stack([pads[0], pads[1], pads[1]])
    mob2 = np.array([mob[0], mob[0]])
    Fa = inp.box_fluxes(both, E, Ef, dr, TD, N_INV, mob2, [-1, 1, -1])[0]
    Fb = inp.box_fluxes(both, E, -Ef, dr, TD, N_INV, mob2, [-1, 1, -1])[0]
    ok = inp.face_valid(NC)
    assert np.array_equal(Fa[1][ok], Fb[2][ok]) and np.array_equal(Fa[2][ok], Fb[1][ok])
    # same field, opposite charge: other upwind side, so not simply -F
    assert not np.array_equal(Fa[1][ok], -Fa[2][ok])
    lines = pads[1][2:-2, :]
    pos = Ef[0][0:NC, :] > 0
    up, um = inp.upwind_faces(lines, pos), inp.upwind_faces(lines, ~pos)
    assert np.array_equal(Fa[1][0][0:NC, :], (1.0 * (mob[0] * N_INV) * Ef[0][0:NC, :]) * up)
    assert np.array_equal(Fa[2][0][0:NC, :], (-1.0 * (mob[0] * N_INV) * Ef[0][0:NC, :]) * um)


def test_upwind_value_of_a_step():
    """A step between cells: the upwind side's value, unlimited."""
    line = np.array([[1.0, 1.0, 1.0, 1.0, 5.0, 5.0, 5.0, 5.0]])
    assert np.array_equal(inp.upwind_faces(line, np.ones((1, 5), bool))[0], [1, 1, 1, 5, 5])
    assert np.array_equal(inp.upwind_faces(line, np.zeros((1, 5), bool))[0], [1, 1, 5, 5, 5])


def test_sigma_is_the_per_face_sum():
    """Uniform field (one mobility), piecewise-constant densities: the
    electrons peak on one line, the ion on another, and a third line holds
    less of each but more of their sum. The folded maximum is that of the
    sum, neither the sum of the maxima nor any single term's."""
    E = np.full((NC + 2, NC + 2), 1e6)
    Ef = np.zeros((2, NC + 1, NC + 1))
    Ef[1] = 1e6  # along y only: x lines see no upwind jump
    mu_e = inp.lt_col(TD, 1, np.array(0.5 * (1e6 + 1e6) * 1e21 * N_INV)) * N_INV
    mob = np.array([mu_e / N_INV])  # the ion as mobile as the electrons
    pads = np.full((2, NC + 4, NC + 4), 1e15)
    pads[0][:, 3] = 3e15   # electrons: column i = 2
    pads[1][:, 5] = 3e15   # ion: column i = 4
    pads[:, :, 4] = 2.5e15  # both: column i = 3
    F, cfl, sigma, terms = inp.box_fluxes(pads, E, Ef, np.array([1e-4, 1e-4]), TD, N_INV, mob,
                                          [-1, 1])
    smax = max(s.max() for s in sigma)
    tmax = [max(t[n].max() for t in terms) for n in range(2)]
    assert smax == mu_e * 2.5e15 + (mob[0] * N_INV) * 2.5e15
    assert smax > max(tmax) and smax < tmax[0] + tmax[1]
    # the face of the maximum holds no species' own maximum
    sy = sigma[1]
    at = np.unravel_index(np.argmax(sy), sy.shape)
    assert all(terms[1][n][at] < tmax[n] for n in range(2))
    assert inp.limits(1.0, smax)[1] == inp.EPS0 / (inp.ELEM_CHARGE * smax)


def test_divergence_of_a_uniform_flux_vanishes():
    y = np.full((NC, NC), 3.0)
    F = np.ones((2, NC + 1, NC + 1))
    assert np.array_equal(inp.add_divergence(y, F, 0.1, [0.5, 0.25]), y)
    # cylindrical: the r term is F (rf1 - rf2) = -F dr / r
    got = inp.add_divergence(y, F, 0.1, [0.5, 0.25], r_min=0.0)
    r = 0.5 * (np.arange(NC) + 0.5)
    assert np.allclose(got, y - 0.1 * 1.0 / r[None, :], rtol=1e-14)

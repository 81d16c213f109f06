"""Photoionization in the 2-D library: everything that needs no GPU -- the
exported entry points, the three regression fixtures of programs/standard_2d
(scripts/make_photoi2d_cases.py), the driver's set-up on them, and the numpy
statement of the source (tests/photoi_numpy.py) against its own edge cases."""
import ctypes

import numpy as np
import pytest

import golden
import photoi_numpy as pn
from afh import capi
from afh.driver import Simulation

ENTRY = ("afh_photoi_set_src", "afh_photoi_helmh_compute")
# (fixture, cylindrical, rows x columns of the committed regression log)
CASES = [("rtest_test_2d_photoi", 0, (8, 12)),
         ("rtest_test_2d_photoi_chem", 0, (8, 27)),
         ("rtest_test_cyl_photoi_chem", 1, (7, 27))]
PFMG = dict(coarse_mode=capi.COARSE_PFMG, coarse_cycles=50, coarse_tol=1e-6)


def test_entry_points_declared_exported_and_bound():
    syms = capi.header_symbols("afivo_hip_2d.h")
    lib = ctypes.CDLL(capi.HIP_LIB_2D)
    for n in ENTRY:
        assert n in syms
        assert n in capi.header_symbols()  # part of the common ABI
        assert hasattr(lib, n)
    h = capi.hip_library_2d()
    assert h.has("photoi_set_src") and h.has("photoi_helmh_compute")


@pytest.mark.parametrize("name,cyl,shape", CASES)
def test_fixture(name, cyl, shape):
    d = golden.load(name)
    assert len(d["coarse_grid_size_value"]) == 2
    assert int(d["photoi%enabled"][0]) == 1
    assert str(d["photoi%method"][0]) == "helmholtz"
    assert str(d["photoi%source_type"][0]) == "Zheleznyak"
    assert str(d["photoi_helmh%author"][0]) == "Bourdon-3"
    assert int(d["cylindrical"][0]) == cyl
    assert d["rtest_log"].shape == shape
    assert len(d["rtest_columns"]) == shape[1]
    # the source as built needs a constant gas density, and no electrode
    assert int(d["gas_constant_density"][0]) == 1
    assert int(d["use_electrode"][0]) == 0


@pytest.mark.parametrize("name,cyl,shape", CASES)
def test_driver_sets_up_the_modes(name, cyl, shape):
    """Simulation.__init__ (no device call): three helmh_n variables, a valid
    photo_species, the Bourdon-3 modes scaled by the O2 pressure."""
    sim = Simulation(capi.hip_library_2d(), golden.load(name), **PFMG)
    assert sim.ndim == 2 and sim.photoi and bool(sim.cylindrical) == bool(cyl)
    assert len(sim.helm_iv) == 3 and len(set(sim.helm_iv)) == 3
    names = list(sim.cc_names)
    assert [names[iv - 1] for iv in sim.helm_iv] == ["helmh_1", "helmh_2", "helmh_3"]
    assert names[sim.i_photo - 1] == "photo"
    assert 1 <= sim.photo_species <= len(sim.plasma)
    # the ion the photoelectrons come with is positive
    assert sim.species_charge[sim.plasma[sim.photo_species - 1]] == 1
    assert len(sim.helm_lambdas) == 3 and all(l > 0 for l in sim.helm_lambdas)
    assert sim.photoi_coeff > 0
    assert sim.tree is None


def test_lt_loc_edges():
    """LT_get_loc: below the table, on a point, between points, at and above
    the last point."""
    x_min, inv_fac, n = 2.0, 4.0, 5  # points at 2, 2.25, ..., 3
    x = np.array([-1.0, 2.0, 2.1, 2.25, 2.3, 2.999, 3.0, 7.0])
    low, lf = pn.lt_loc(x, x_min, inv_fac, n)
    assert list(low) == [1, 1, 1, 1, 2, 4, 4, 4]
    assert lf[0] == 1.0 and lf[1] == 1.0 and lf[6] == 0.0 and lf[7] == 0.0
    assert lf[3] == 0.0  # on point 2: all weight on low + 1
    assert np.all((lf >= 0) & (lf <= 1))
    y = np.array([[10.0, 20.0, 30.0, 40.0, 50.0]])
    v = pn.lt_col(y, 1, low, lf)
    assert v[0] == 10.0 and v[3] == 20.0 and v[6] == 50.0 and v[7] == 50.0
    assert abs(v[2] - 14.0) < 1e-12


def test_source_clamps_and_scales():
    tab = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [5.0, 5.0, 5.0]])
    fld = np.array([0.0, 1.0, 2.0, 50.0])
    ne = np.array([1.0, 0.0, 2.0, 1.0])
    s = pn.source(fld, ne, 1e21, 0.0, 1.0, tab, 3, 0.5)
    # Td = fld; mobility 1, -, 3, 3 (clamped above the table); alpha 5
    assert list(s) == [0.0, 0.0, 2.0 * 3.0 * 5.0 * 2.0 * 0.5, 50.0 * 3.0 * 5.0 * 0.5]
    assert np.all(pn.source(fld, ne, 1e21, 0.0, 1.0, tab, 3, -0.5) == 0.0)

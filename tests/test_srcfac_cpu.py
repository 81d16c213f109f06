"""The flux-based source factor (fixes%source_factor = flux) without a GPU:
the entry point through every layer, tests/srcfac_numpy.py against the
reference's own step (tests/golden/srcfac_*.npz, scripts/
make_srcfac_cases.py), the fixtures themselves, and the driver's entries.

The numpy statement takes the electron face flux as an input. Here it comes
from the C oracle's flux_upwind_tree (3-D) and from tests/ions2d_numpy.py
(2-D), both held to the reference elsewhere. The factor is compared bitwise
(the NORM2 evaluation of the reference's Fortran runtime is reproduced); the
densities bitwise for test_3d and test_2d, whose rates call neither exp nor
pow, and to 1e-13 relative otherwise (tests/test_2d_replay.py's bar for
last-ulp libm differences), the count of values that are not bitwise printed.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import state_srcfac as ss
from afh import capi
from afh.driver import Simulation

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(REPO, "afivo-streamer_amd", "fortran")
FLANG = shutil.which("amdflang") or "/opt/rocm/llvm/bin/amdflang"
NAME = "afh_fluid_set_source_factor"
CASES = [(m, v) for m in ss.MODELS for v in ss.VARIANTS]


# ------------------------------------------------------------------ the ABI
def test_both_libraries_export_the_symbol():
    for path in (capi.HIP_LIB, capi.HIP_LIB_2D):
        assert hasattr(ctypes.CDLL(path), NAME), path


def test_header_declares_it_outside_the_common_abi():
    assert capi.header_symbols("afivo_hip_srcfac.h") == [NAME]
    assert NAME not in capi.header_symbols("afivo_hip.h")
    assert NAME not in capi.header_symbols("afivo_hip_2d.h")
    src = open(os.path.join(REPO, "include", "afivo_hip_srcfac.h")).read()
    assert "#define AFH_SRCFAC_NONE 0" in src and "#define AFH_SRCFAC_FLUX 1" in src
    assert (capi.SRCFAC_NONE, capi.SRCFAC_FLUX) == (0, 1)


def test_binding_for_the_hip_libraries_only():
    assert list(capi.SIGNATURES_SRCFAC) == ["fluid_set_source_factor"]
    assert not set(capi.SIGNATURES_SRCFAC) & set(capi.SIGNATURES)
    assert capi.hip_library().has("fluid_set_source_factor")
    assert capi.hip_library_2d().has("fluid_set_source_factor")
    assert not capi.oracle_library().has("fluid_set_source_factor")
    # (the common ABI the libraries report is unchanged)
    assert "afh_fluid_set_source_factor" not in capi.hip_library().symbols()


@pytest.mark.skipif(not os.path.exists(FLANG), reason="amdflang not in the image")
def test_fortran_module_and_snippet_compile(tmp_path):
    """m_afivo_hip_srcfac.F90 and INTEGRATION.md's snippet against
    m_afivo_hip (no GPU, no link)."""
    srcs = [os.path.join(FDIR, "m_afivo_hip.F90"), os.path.join(FDIR, "m_afivo_hip_srcfac.F90"),
            os.path.join(REPO, "tests", "fortran", "source_factor.F90")]
    for src in srcs:
        pre = tmp_path / (os.path.basename(src)[:-4] + ".f90")
        with open(pre, "w") as out:
            subprocess.run(["cpp", "-traditional-cpp", "-P", src], stdout=out, check=True)
        r = subprocess.run([FLANG, "-c", str(pre), "-o", str(pre) + ".o"], cwd=tmp_path,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# ------------------------------------------------------------- the fixtures
@pytest.fixture(scope="module")
def states():
    """{model: the state of tests/state_srcfac.build_state}, built once."""
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = ss.build_state(model)
        return cache[model]
    return get


@pytest.mark.parametrize("model,variant", CASES)
def test_fixture_belongs_to_the_state(states, model, variant):
    c, af, _, _, _, _ = states(model)
    fx = ss.load(model, variant)
    keep = ss.kept_leaves(model, af, len(c.ia("all_densities")))
    assert fx["leaves"].tolist() == keep
    assert set(keep) <= set(af.leaves()) and len({af.lvl[b] for b in keep}) >= 2
    nd = ss.MODELS[model][0]
    for k in (1, 2):
        assert fx["dens_%d" % k].shape == (len(c.ia("all_densities")), len(keep)) + (af.nc,) * nd
        assert fx["srcfac_%d" % k].shape == fx["off_e_%d" % k].shape == fx["dens_%d" % k].shape[1:]


@pytest.mark.parametrize("model", list(ss.MODELS))
def test_fixtures_are_not_vacuous(model):
    """Conditions, not measurements: the factor changes the electrons of at
    least 20 % of the cells by more than 1e-10 relative, the threshold at
    least 5 % more, and the stored factor has cells at 1, cells at 0 (with
    the threshold, which is what sets them) and at least 10 % in between."""
    flux, mn = ss.load(model, "flux"), ss.load(model, "min")
    for k in (1, 2):
        off = flux["off_e_%d" % k]
        assert np.array_equal(off, mn["off_e_%d" % k])
        ch_f = np.abs(flux["dens_%d" % k][0] / off - 1) > 1e-10
        ch_m = np.abs(mn["dens_%d" % k][0] / off - 1) > 1e-10
        assert ch_f.mean() >= 0.20, ch_f.mean()
        assert (ch_m & ~ch_f).mean() >= 0.05, (ch_m & ~ch_f).mean()
        for fx in (flux, mn):
            s = fx["srcfac_%d" % k]
            assert s.min() >= 0.0 and s.max() == 1.0
            assert ((s > 0) & (s < 1)).mean() >= 0.10
        assert (mn["srcfac_%d" % k] == 0).any()
        # the threshold only clears cells: elsewhere the two factors agree
        on = mn["srcfac_%d" % k] != 0
        assert np.array_equal(mn["srcfac_%d" % k][on], flux["srcfac_%d" % k][on])


def test_ionization_reactions_are_a_strict_subset_in_the_chemistry_model(states):
    for model, n_ion in (("test_3d", 1), ("test_3d_chem", 3)):
        ion = ss.ionization(states(model)[0])
        assert sum(ion) == n_ion and 0 < sum(ion) < len(ion)


# ------------------------------------------------- numpy against the fixtures
@pytest.fixture(scope="module")
def fluxes(states):
    """{(model, stage): (Simulation, the electron face flux of the state)}:
    the C oracle's flux_upwind_tree in 3-D, tests/ions2d_numpy.py in 2-D."""
    cache = {}

    def get(model, k):
        if (model, k) in cache:
            return cache[model, k]
        c, af, cc, fc, _, d = states(model)
        s_deriv = ss.stages(model)[k][0]
        if ss.MODELS[model][0] == 3:
            sim = Simulation(capi.oracle_library(), d)
            sim.af = af
            sim._bind(sim._create_tree())
            for iv, a in cc.items():
                sim.tree.put_cc(iv, a)
            for ivf, a in fc.items():
                sim.tree.put_fc(ivf, a)
            sim.fluid.flux_upwind_tree(s_deriv)
            F = sim.tree.get_fc(sim.f_flux)
            sim.tree.close()
        else:
            sim = Simulation(capi.hip_library_2d(), d)
            F = ss.flux_2d_numpy(sim, af, cc, fc, s_deriv)
        cache[model, k] = (sim, F)
        return cache[model, k]
    return get


@pytest.mark.parametrize("model,variant", CASES)
def test_numpy_equals_the_reference(states, fluxes, monkeypatch, model, variant):
    monkeypatch.setenv("AFH_FACES_FROM_PHI", "0")  # the stored face field, as the reference
    c, af, cc, fc, dt0, _ = states(model)
    fx = ss.load(model, variant)
    keep = fx["leaves"].tolist()
    n_diff, worst = 0, 0.0
    for k, stage in enumerate(ss.stages(model)):
        sim, F = fluxes(model, k)
        res = ss.numpy_step(sim, af, cc, F, stage, ss.stage_dt(model, k, dt0), keep,
                            min_e=ss.VARIANTS[variant])
        s = np.stack([res[b][1] for b in keep])
        assert np.array_equal(s, fx["srcfac_%d" % (k + 1)]), (k, int((s != fx["srcfac_%d" % (k + 1)]).sum()))
        for q in range(len(sim.plasma)):
            y = np.stack([res[b][0][q] for b in keep])
            r = fx["dens_%d" % (k + 1)][q]
            n_diff += int((y != r).sum())
            worst = max(worst, float(np.abs(y / r - 1).max()))
    print("%s %s: %d densities not bitwise, max rel %.3g" % (model, variant, n_diff, worst))
    assert worst <= 1e-13
    if model in ("test_3d", "test_2d"):
        assert n_diff == 0


def test_plain_norm_is_not_the_reference_norm(states, fluxes, monkeypatch):
    """sqrt(a a + b b + c c) in place of the runtime's NORM2 misses the stored
    factor in the last bit of some cells: the evaluation matters."""
    import srcfac_numpy as sn
    monkeypatch.setattr(sn, "norm2", lambda v: np.sqrt(np.sum(v * v, axis=-1)))
    c, af, cc, fc, dt0, _ = states("test_3d")
    fx = ss.load("test_3d", "flux")
    keep = fx["leaves"].tolist()
    sim, F = fluxes("test_3d", 0)
    res = ss.numpy_step(sim, af, cc, F, ss.stages("test_3d")[0], dt0, keep)
    s = np.stack([res[b][1] for b in keep])
    assert not np.array_equal(s, fx["srcfac_1"])
    assert np.abs(s / fx["srcfac_1"] - 1).max() < 1e-15


# ------------------------------------------------------------------ driver
def _case(model="test_3d"):
    return dict(ss.golden.load(ss.MODELS[model][1]))


def test_driver_reads_the_entries():
    lib = capi.hip_library()
    sim = Simulation(lib, _case())
    assert sim.source_factor == capi.SRCFAC_NONE and sim.i_srcfac == 0
    d = ss.case_with_factor(_case(), "min")
    sim = Simulation(lib, d)
    assert sim.source_factor == capi.SRCFAC_FLUX
    assert sim.source_min_electrons == 5e4
    assert sim.cc_names[sim.i_srcfac - 1] == "srcfac" and sim.i_srcfac == sim.n_var_cell
    assert sim.ionization == [True, False]
    d = ss.case_with_factor(_case(), "flux", write=False)
    sim = Simulation(lib, d)
    assert sim.source_factor == capi.SRCFAC_FLUX and sim.i_srcfac == 0
    d["source_factor"] = np.array(["none"])
    assert Simulation(lib, d).source_factor == capi.SRCFAC_NONE
    assert Simulation(capi.hip_library_2d(),
                      ss.case_with_factor(_case("test_2d"), "flux")).i_srcfac > 0


def test_driver_refuses_an_unknown_factor():
    d = _case()
    d["source_factor"] = np.array(["original_flux"])
    with pytest.raises(ValueError, match="none, flux"):
        Simulation(capi.hip_library(), d)


def test_driver_needs_the_srcfac_variable_to_write_it():
    d = ss.case_with_factor(_case(), "flux")
    d["cc_names"] = np.array([n for n in d["cc_names"] if n != "srcfac"])
    with pytest.raises(ValueError, match="srcfac"):
        Simulation(capi.hip_library(), d)


def test_driver_refuses_a_library_without_the_entry_point():
    with pytest.raises(NotImplementedError, match="source_factor"):
        Simulation(capi.oracle_library(), ss.case_with_factor(_case(), "flux"))
    # (a case that does not ask for the factor still runs on it)
    assert Simulation(capi.oracle_library(), _case()).source_factor == capi.SRCFAC_NONE

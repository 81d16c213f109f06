"""The rate and J.E sums (include/afivo_hip_rates.h) without a GPU: the entry
points through every layer, the driver's refusal on a library without them,
and the restart record.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden
from afh import capi
from afh.datfile import DatTree, parse_sim_data, sim_data_bytes
from afh.driver import Simulation

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(REPO, "afivo-streamer_amd", "fortran")
FLANG = shutil.which("amdflang") or "/opt/rocm/llvm/bin/amdflang"
NAMES = ["afh_fluid_set_rate_sums", "afh_fluid_fetch_rate_sums"]


# ------------------------------------------------------------------ the ABI
def test_both_libraries_export_the_symbols():
    for path in (capi.HIP_LIB, capi.HIP_LIB_2D):
        for name in NAMES:
            assert hasattr(ctypes.CDLL(path), name), (path, name)


def test_header_declares_them_outside_the_common_abi():
    assert sorted(capi.header_symbols("afivo_hip_rates.h")) == sorted(NAMES)
    for name in NAMES:
        assert name not in capi.header_symbols("afivo_hip.h")
        assert name not in capi.header_symbols("afivo_hip_2d.h")
        assert name not in capi.header_symbols("afivo_hip_srcfac.h")


def test_binding_for_the_hip_libraries_only():
    assert sorted(capi.SIGNATURES_RATES) == sorted(n[len("afh_"):] for n in NAMES)
    assert not set(capi.SIGNATURES_RATES) & set(capi.SIGNATURES)
    for n in capi.SIGNATURES_RATES:
        assert capi.hip_library().has(n) and capi.hip_library_2d().has(n)
        assert not capi.oracle_library().has(n)
        # (the common ABI the libraries report is unchanged)
        assert "afh_" + n not in capi.hip_library().symbols()
        assert "afh_" + n not in capi.hip_library_2d().symbols()


@pytest.mark.skipif(not os.path.exists(FLANG), reason="amdflang not in the image")
def test_fortran_module_compiles(tmp_path):
    """m_afivo_hip_rates.F90 against m_afivo_hip (no GPU, no link), and its
    interfaces name the two entry points."""
    src = open(os.path.join(FDIR, "m_afivo_hip_rates.F90")).read()
    for name in NAMES:
        assert 'afh_pfx//"%s"' % name[len("afh_"):] in src
    for base in ("m_afivo_hip.F90", "m_afivo_hip_rates.F90"):
        pre = tmp_path / (base[:-4] + ".f90")
        with open(pre, "w") as out:
            subprocess.run(["cpp", "-traditional-cpp", "-P", os.path.join(FDIR, base)],
                           stdout=out, check=True)
        r = subprocess.run([FLANG, "-c", str(pre), "-o", str(pre) + ".o"], cwd=tmp_path,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# --------------------------------------------------------------- the driver
def test_driver_refuses_a_library_without_the_sums():
    with pytest.raises(NotImplementedError, match="afivo_hip_rates.h"):
        Simulation(capi.oracle_library(), golden.load("rtest_test_3d"), global_rates=True)


def test_driver_default_is_off_and_reads_the_update_interval():
    d = dict(golden.load("rtest_test_2d"))
    sim = Simulation(capi.oracle_library(), d)
    assert not sim.rate_sums and sim.current_update_per_steps == 1000 * 1000
    assert np.all(sim.global_rates == 0) and sim.global_JdotE == 0.0
    with pytest.raises(RuntimeError, match="global_rates"):
        sim.diagnostics()
    d["current_update_per_steps"] = np.array([3])
    assert Simulation(capi.oracle_library(), d).current_update_per_steps == 3


def test_default_run_writes_the_record_with_zeros(tmp_path):
    """Without global_rates the .dat record is the one of a run that never
    had the sums: zeros in both fields, the bytes those of sim_data_bytes with
    zeros."""
    sim = Simulation(capi.oracle_library(), golden.load("rtest_test_3d"))
    sim.start()
    sim.step()
    sim.write_dat(str(tmp_path / "run"))
    t = DatTree.read(tmp_path / "run.dat")
    n = len(sim.reactions)
    d = parse_sim_data(t.other, n)
    assert np.all(d["global_rates"] == 0.0) and d["global_JdotE"] == 0.0
    assert t.other == sim_data_bytes(sim.it, sim.output_cnt, sim.time, sim.global_time,
                                     sim.photoi_prev_time, sim.global_dt, np.zeros(n), 0.0,
                                     sim.frac_rejected)
    sim.tree.close()


def test_record_round_trips_nonzero_rates():
    rates = np.array([3.25e9, 0.0, 1.5e-3, 7.0e12])
    raw = sim_data_bytes(17, 3, 1.5e-9, 1.5e-9, 1.25e-9, 2e-12, rates, 4.75e-7, 0.0199)
    d = parse_sim_data(raw, len(rates))
    assert np.array_equal(d["global_rates"], rates) and d["global_JdotE"] == 4.75e-7
    assert d["it"] == 17 and d["fraction_steps_rejected"] == 0.0199
    assert sim_data_bytes(d["it"], d["output_cnt"], d["time"], d["global_time"],
                          d["photoi_prev_time"], d["global_dt"], d["global_rates"],
                          d["global_JdotE"], d["fraction_steps_rejected"]) == raw

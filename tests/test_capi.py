"""CPU-side checks of the C ABI: the product library builds for gfx950, loads,
and exports every symbol include/afivo_hip.h declares (no compute calls)."""
import ctypes

import pytest

from afh import capi


def test_header_declares_api():
    syms = capi.header_symbols()
    assert "afh_mg_fas_vcycle" in syms and "afh_flux_upwind_tree" in syms
    assert len(syms) >= 24


def test_hip_library_exports_every_header_symbol():
    lib = ctypes.CDLL(capi.HIP_LIB)
    missing = [s for s in capi.header_symbols() if not hasattr(lib, s)]
    assert not missing, missing


def test_binding_covers_header():
    bound = {"afh_" + n for n in capi.SIGNATURES}
    assert set(capi.header_symbols()) == bound


def test_oracle_exports_same_api():
    lib = ctypes.CDLL(capi.ORACLE_LIB)
    missing = [s.replace("afh_", "afo_") for s in capi.header_symbols()
               if not hasattr(lib, s.replace("afh_", "afo_"))]
    assert not missing, missing


@pytest.mark.parametrize("which", ["3d", "2d"])
def test_bad_argument_sets_the_error_text(which):
    """The error plumbing both libraries share: a null handle returns
    AFH_ERR_ARG (-1) and afh_last_error() gives the call's text, the next
    failing call replaces it. No GPU: the handles are refused before any
    device call. (afh_profile_read's text differs between the libraries.)"""
    lib = ctypes.CDLL(capi.HIP_LIB if which == "3d" else capi.HIP_LIB_2D)
    lib.afh_last_error.restype = ctypes.c_char_p
    fn = lib.afh_fluid_set_source_factor
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double,
                   ctypes.c_int32]
    assert fn(None, 0, None, 0.0, 0) == -1
    assert lib.afh_last_error() == b"afh_fluid_set_source_factor: null"
    out = ctypes.c_double()
    lib.afh_tree_sum_cc.restype = ctypes.c_int32
    lib.afh_tree_sum_cc.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.c_void_p]
    assert lib.afh_tree_sum_cc(None, 1, 1, ctypes.byref(out)) == -1
    assert lib.afh_last_error() == b"afh_tree_sum_cc: null tree"
    lib.afh_profile_read.restype = ctypes.c_int32
    lib.afh_profile_read.argtypes = [ctypes.c_void_p] * 4
    assert lib.afh_profile_read(None, None, None, None) == -1
    assert lib.afh_last_error() == (b"null argument" if which == "3d"
                                    else b"afh_profile_read: null argument")


def test_no_device_is_an_error_not_a_fallback():
    """Without a GPU the product must fail loudly (no CPU fallback)."""
    import numpy as np
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from afh.model import Tree
    from afh.tree import uniform_tree
    topo = uniform_tree(4, (4, 4, 4), (1e-3, 1e-3, 1e-3), 2)
    with pytest.raises(capi.AfhError):
        Tree(capi.hip_library(), topo, 14, 2)

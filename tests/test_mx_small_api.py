"""The opt-in MX pipeline for mid-size forwards (glc_engine_set_mx_small_forwards) and the 128 tile of the MX GEMM (csrc/gemm128x.hip): what
can be checked without a GPU — the symbols, their declarations, the Python wrappers, and the kernel instantiations the product library ships."""
import ctypes
import os
import re

from test_build import SO, _kernel_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("glc_engine_set_mx_small_forwards", "glc_debug_last_forward_mx128")


def test_library_exports_the_symbols_and_the_bindings_know_them():
    from gliclass.c_amd import _lib
    L = ctypes.CDLL(SO)
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in _lib.HIP_SYMBOLS, s
    hip = _lib.hip()
    assert hip.glc_engine_set_mx_small_forwards(None, 1) == -1 and b"null engine" in hip.glc_last_error()
    assert hip.glc_debug_last_forward_mx128(None) == -1


def test_header_declares_the_switch_the_query_and_the_kernel_id():
    code = open(os.path.join(ROOT, "include", "gliclass_hip.h")).read()
    assert re.search(r"\bint\s+glc_engine_set_mx_small_forwards\s*\(\s*glc_engine\s*\*\s*e\s*,\s*int\s+mode\s*\)\s*;", code)
    assert re.search(r"\bint\s+glc_debug_last_forward_mx128\s*\(\s*const\s+glc_engine\s*\*\s*e\s*\)\s*;", code)
    assert re.search(r"\bGLC_GEMM_RUN_AUTO\s*=\s*4\b", code) and re.search(r"\bGLC_GEMM_RUN_MX128\s*=\s*5\b", code)
    assert "GLICLASS_MX_SMALL" in code


def test_engine_class_has_both_methods():
    from gliclass.c_amd.engine import Engine
    assert callable(getattr(Engine, "set_mx_small_forwards", None)) and callable(getattr(Engine, "last_mx128", None))


def test_library_ships_exactly_the_128_tile_builds_the_launcher_reaches():
    """EPI_BIAS (0), EPI_GELU (1), EPI_RESID (2), EPI_QKV (3) and the transposed EPI_QKV build of the V third: nothing else"""
    ks = [k for k in _kernel_names() if "gemm128x_kernel<" in k]
    got = sorted(re.search(r"gemm128x_kernel<([^>]*)>", k).group(1).replace(" ", "") for k in ks)
    assert got == ["0,false", "1,false", "2,false", "3,false", "3,true"], ks

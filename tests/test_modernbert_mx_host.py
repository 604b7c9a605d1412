"""CPU: the public switch of ModernBERT's opt-in MX pipeline exists in the C header and in the ctypes table, and the entry answers a
null engine with -1 and a message without touching a GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_in_the_header_and_documented():
    src = open(os.path.join(ROOT, "include", "gliclass_hip.h")).read()
    assert re.search(r"^int glc_engine_enable_mx\(glc_engine\* e\);", src, re.M)
    assert "GLICLASS_MX_MODERNBERT=1" in src
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "GLICLASS_MX_MODERNBERT" in doc


def test_entry_is_in_the_ctypes_table_and_the_engine_class():
    from gliclass.c_amd import _lib
    from gliclass.c_amd.engine import Engine
    assert "glc_engine_enable_mx" in _lib.HIP_SYMBOLS
    assert callable(getattr(Engine, "enable_mx"))
    L = _lib.hip()
    assert all(hasattr(L, s) for s in _lib.HIP_SYMBOLS)


def test_null_engine_is_refused_cleanly():
    from gliclass.c_amd import _lib
    L = _lib.hip()
    assert L.glc_engine_enable_mx(None) == -1
    assert b"enable_mx: null engine" in L.glc_last_error()


def test_the_mx_gemm_admits_the_geglu_epilogue_on_the_eight_wave_tile_only():
    """the launcher's table: EPI_GEGLU reaches gemm256x_kernel, never the one-wave gemm256w_kernel (tests/test_build.py pins its four builds)"""
    src = open(os.path.join(ROOT, "gliclass", "c_amd", "csrc", "gemm256x.hip")).read()
    assert "launch_x<EPI_GEGLU, false>" in src
    w128 = src[src.index("if constexpr (!VMODE && (EPI == EPI_BIAS"):]
    assert "EPI_GEGLU" not in w128[:w128.index("{")]

"""CPU (no GPU): the captured-graph replay switch and its two reports exist at every layer — declared in include/gliclass_hip.h, exported
by libgliclass_hip.so, bound in _lib.py and offered by Engine — and answer a null engine as the header says."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("glc_engine_set_graph_replay", "glc_debug_last_forward_graph", "glc_debug_graph_cache_size")


@pytest.fixture(scope="module")
def hip():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "gliclass", "c_amd"), "-j4", "all"], stdout=subprocess.DEVNULL)
    from gliclass.c_amd import _lib
    return _lib.hip()


def test_header_declares_the_switch_and_the_reports():
    src = open(os.path.join(ROOT, "include", "gliclass_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+glc_engine_set_graph_replay\s*\(\s*glc_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", code)
    assert re.search(r"\bint\s+glc_debug_last_forward_graph\s*\(\s*const\s+glc_engine\s*\*\s*e\s*\)\s*;", code)
    assert re.search(r"\bint\s+glc_debug_graph_cache_size\s*\(\s*const\s+glc_engine\s*\*\s*e\s*\)\s*;", code)
    assert "GLICLASS_GRAPH_REPLAY" in src


def test_library_exports_the_symbols(hip):
    from gliclass.c_amd import _lib
    for s in SYMBOLS:
        assert s in _lib.HIP_SYMBOLS, s
        assert hasattr(hip, s), s


def test_engine_has_the_methods():
    from gliclass.c_amd.engine import Engine
    for m in ("set_graph_replay", "last_graph", "graph_cache_size"):
        assert callable(getattr(Engine, m, None)), m


def test_null_engine(hip):
    assert hip.glc_engine_set_graph_replay(None, 1) == -1
    assert b"null engine" in hip.glc_last_error()
    assert hip.glc_debug_last_forward_graph(None) == -1
    assert hip.glc_debug_graph_cache_size(None) == -1

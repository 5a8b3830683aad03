"""CPU side of the multiplicative level combination (fedd_schwarz_set_level_combination): the entries are exported and
wrapped, the setting is a property of the context that needs no device, and the facade that calls it still compiles."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_combination_entries_are_exported(fedd_lib):
    L = ctypes.CDLL(fedd_lib.LIB_PATH)
    for name in ("fedd_schwarz_set_level_combination", "fedd_schwarz_get_level_combination"):
        assert hasattr(L, name), name
        assert name in fedd_lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    assert int(re.search(r"#define FEDD_LEVELS_ADDITIVE (\d+)", hdr).group(1)) == fedd_lib.LEVELS_ADDITIVE == 0
    assert int(re.search(r"#define FEDD_LEVELS_MULTIPLICATIVE (\d+)", hdr).group(1)) == fedd_lib.LEVELS_MULTIPLICATIVE == 1


def test_level_combination_is_a_context_setting(fedd_lib):
    """set before any setup (as fedd_schwarz_set_coarse may be), read back, unknown values refused; no device needed"""
    c = fedd_lib.Context(device=-1)
    try:
        assert c.schwarz_get_level_combination() == fedd_lib.LEVELS_ADDITIVE
        c.schwarz_set_level_combination(fedd_lib.LEVELS_MULTIPLICATIVE)
        assert c.schwarz_get_level_combination() == fedd_lib.LEVELS_MULTIPLICATIVE
        with pytest.raises(fedd_lib.FeddError, match="fedd_schwarz_set_level_combination"):
            c.schwarz_set_level_combination(2)
        assert c.schwarz_get_level_combination() == fedd_lib.LEVELS_MULTIPLICATIVE
        c.schwarz_set_level_combination(fedd_lib.LEVELS_ADDITIVE)
        assert c.schwarz_get_level_combination() == fedd_lib.LEVELS_ADDITIVE
    finally:
        c.close()


def test_facade_sets_the_level_combination_and_compiles():
    src = open(os.path.join(ROOT, "feddlib_amd", "host", "feddlib", "fedd_facade.hpp")).read()
    assert "fedd_schwarz_set_level_combination(ctx" in src
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    host = os.path.join(ROOT, "feddlib_amd", "host")
    drv = os.path.join(ROOT, "examples", "drivers", "laplace_main.cpp")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", host, drv], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

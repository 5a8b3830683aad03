"""CPU side of preconditioned CG and the symmetric Schwarz apply: the entries are exported, declared and wrapped, the two
options exist, and a host-only context is told that the solve needs a GPU."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fedd_cg", "fedd_cg_x0", "fedd_cg_info", "fedd_schwarz_full_info")


def test_cg_entries_are_exported_declared_and_wrapped(fedd_lib):
    L = ctypes.CDLL(fedd_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in fedd_lib.SIGNATURES, name
        assert "int %s(fedd_ctx* ctx" % name in hdr, name
    for wrapper in ("cg", "cg_x0", "cg_info", "schwarz_full_info"):
        assert callable(getattr(fedd_lib.Context, wrapper)), wrapper
    # the signatures of fedd_gmres / fedd_gmres_x0 without `restart`
    for a, b in (("fedd_cg", "fedd_gmres"), ("fedd_cg_x0", "fedd_gmres_x0")):
        g = list(fedd_lib.SIGNATURES[b])
        assert fedd_lib.SIGNATURES[a] == g[:5] + g[6:]


def test_cg_options_exist(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        c.set_option("apply_gather", 1)
        c.set_option("apply_gather", 0)
        for kind in (0, 1, 2):
            c.set_option("apply_full_kind", kind)
        with pytest.raises(fedd_lib.FeddError, match="apply_full_kind"):
            c.set_option("apply_full_kind", 3)
        c.set_option("apply_full_kind", 0)
        assert c.cg_info() == {"replacements": 0, "breakdown": 0}
    finally:
        c.close()


def test_cg_needs_a_gpu_context(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        b = np.ones(4)
        x = np.zeros(4)
        its, rel = ctypes.c_int(), ctypes.c_double()
        for fn in (c._L.fedd_cg, c._L.fedd_cg_x0):
            rc = fn(c._h, b.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                    1e-8, 10, 0, ctypes.byref(its), ctypes.byref(rel))
            assert rc != 0
            assert "needs a GPU context" in c._L.fedd_last_error().decode()
    finally:
        c.close()


def test_facade_names_the_cg_entries():
    src = open(os.path.join(ROOT, "feddlib_amd", "host", "feddlib", "fedd_facade.hpp")).read()
    for s in ("fedd_cg(ctx", "fedd_cg_x0(ctx", '"Block CG"', '"Pseudo Block CG"', "is not built (Block GMRES, Block CG, Pseudo Block CG are)"):
        assert s in src, s

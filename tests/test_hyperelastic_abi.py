"""The hyperelastic entries at the ABI level, without a GPU: the symbols in header, library and binding, and the loud failure on a
host-only context."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_in_header_library_and_binding(fedd_lib):
    hdr = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    L = ctypes.CDLL(fedd_lib.LIB_PATH)
    for name in ("fedd_assemble_hyperelastic", "fedd_hyperelastic_force_get"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in fedd_lib.SIGNATURES
    for name, value in (("FEDD_HYPER_NEOHOOKE", fedd_lib.HYPER_NEOHOOKE), ("FEDD_HYPER_MOONEY_RIVLIN", fedd_lib.HYPER_MOONEY_RIVLIN),
                        ("FEDD_HYPER_STVK", fedd_lib.HYPER_STVK)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, hdr).group(1)) == value
    for name, value in (("FEDD_HYPER_TANGENT", fedd_lib.HYPER_TANGENT), ("FEDD_HYPER_FORCE", fedd_lib.HYPER_FORCE)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == value
    assert hasattr(fedd_lib.Context, "assemble_hyperelastic") and hasattr(fedd_lib.Context, "hyperelastic_force_get")


def test_calls_fail_loudly_without_a_device(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
            c.assemble_hyperelastic(fedd_lib.HYPER_NEOHOOKE, [3.0e6, 0.4])
        buf = (ctypes.c_double * 3)()
        L = fedd_lib.lib()
        assert L.fedd_hyperelastic_force_get(c._h, ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))) != 0
        assert "needs a GPU context" in L.fedd_last_error().decode()
    finally:
        c.close()

"""ALE convection, host side of the ABI: the symbols of the header section "ALE convection" are exported and bound, and they
fail loudly on a host-only context.  tests/test_gpu_ale.py runs them."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fedd_mesh_velocity_set", "fedd_mesh_velocity_diff", "fedd_mesh_velocity_get", "fedd_assemble_advection_ale")


def test_symbols_in_header_library_and_binding(fedd_lib):
    hdr = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    L = ctypes.CDLL(fedd_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in fedd_lib.SIGNATURES
    for name, value in (("FEDD_ALE_P", fedd_lib.ALE_P), ("FEDD_ALE_FIXEDPOINT", fedd_lib.ALE_FIXEDPOINT),
                        ("FEDD_ALE_NEWTON", fedd_lib.ALE_NEWTON)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, hdr).group(1)) == value
    for name in ("mesh_velocity_set", "mesh_velocity_diff", "mesh_velocity", "assemble_advection_ale"):
        assert hasattr(fedd_lib.Context, name), name
    # the entries cite the reference lines they replace
    for cite in ("FE_def.hpp:3044-3255", "FSI_def.hpp:460-462", "NavierStokes_def.hpp:245-278", "FE_def.hpp:3064-3065"):
        assert cite in hdr, cite
    # the moving-mesh section no longer lists this as left out, and keeps the mesh velocity across a move
    assert "mesh velocity and ALE convection" not in hdr
    assert re.search(r"A move KEEPS.*fedd_mesh_velocity_set.*A move DROPS", hdr, re.S)


def test_calls_fail_loudly_without_a_device(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        for call in (lambda: c.mesh_velocity_set(np.zeros(6)), lambda: c.mesh_velocity_set(None),
                     lambda: c.mesh_velocity_diff(np.zeros(6), np.zeros(6), 0.1), lambda: c.mesh_velocity(),
                     lambda: c.assemble_advection_ale(fedd_lib.ALE_P, 1.0, -1, 4),
                     lambda: c.assemble_advection_ale(fedd_lib.ALE_NEWTON, 1.0, -1, 4)):
            with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
                call()
    finally:
        c.close()

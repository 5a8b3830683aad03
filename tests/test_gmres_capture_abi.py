"""CPU side of the s-step block capture: the three entries are exported, declared and wrapped, capi checks its arguments
before it calls, and contexts that cannot capture say why."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fedd_gmres_capture_arm", "fedd_gmres_capture_info", "fedd_gmres_capture_get")


def test_capture_entries_are_exported_declared_and_wrapped(fedd_lib):
    L = ctypes.CDLL(fedd_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in fedd_lib.SIGNATURES, name
        assert "int %s(fedd_ctx* ctx" % name in hdr, name
        assert callable(getattr(fedd_lib.Context, name[len("fedd_"):])), name
    for piece in fedd_lib.Context.CAPTURE_PIECES:
        assert '"%s"' % piece in hdr, piece


def test_capture_argument_checks(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        assert c.gmres_capture_info() == dict(captured=0, n=0, ldv=0, k=0, sa_req=0, S=0, m=0, fused=0)
        with pytest.raises(ValueError, match="no piece is named 'W3'"):
            c.gmres_capture_get("W3")
        with pytest.raises(ValueError, match="integer"):
            c.gmres_capture_arm(1.5)
        with pytest.raises(fedd_lib.FeddError, match="nothing captured"):
            c.gmres_capture_get("P1")
        with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
            c.gmres_capture_arm(0)
        c.gmres_capture_arm(-1)                     # disarming needs nothing
        out = np.zeros(1)
        rc = c._L.fedd_gmres_capture_get(c._h, b"nope", out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1)
        assert rc != 0 and "no piece is named 'nope'" in c._L.fedd_last_error().decode()
        rc = c._L.fedd_gmres_capture_get(c._h, b"P1", None, 0)
        assert rc != 0 and "null argument" in c._L.fedd_last_error().decode()
    finally:
        c.close()


def test_capture_is_refused_on_several_ranks(fedd_lib):
    c = fedd_lib.Context(device=-1, rank=1, nranks=2, nccl_id=None)
    try:
        with pytest.raises(fedd_lib.FeddError, match="fedd_gmres_capture_arm: one rank only"):
            c.gmres_capture_arm(0)
    finally:
        c.close()

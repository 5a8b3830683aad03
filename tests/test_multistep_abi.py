"""BDF history, C ABI (include/fedd_hip.h "BDF time stepping", feddlib_amd/csrc/timestep.hip): the five symbols are declared,
exported and bound; on a host-only context every compute entry fails with "needs a GPU context"; `order` and `n_use` are
refused before anything else, so those errors are checked here without a device; matrix slots 5 and 6 exist, slot 7 does not."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("fedd_multistep_begin", "fedd_multistep_advance", "fedd_multistep_set", "fedd_multistep_get", "fedd_multistep_info")


def test_new_symbols_in_header_library_and_binding(fedd_lib):
    hdr = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    L = ctypes.CDLL(fedd_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in fedd_lib.SIGNATURES, name
        assert hasattr(fedd_lib.Context, name[len("fedd_"):]), name
    # the entries cite the reference lines they replace, and say where they differ from them
    for cite in ("DAESolverInTime_def.hpp:1209-1333", "TimeSteppingTools.cpp:493-515", "TimeProblem_def.hpp:833-849", ":417-438",
                 "applied ONCE"):
        assert cite in hdr, cite
    # the history kernel has a timing class of its own, named in the binding
    n = int(re.search(r"FEDD_T_COUNT\s*=\s*(\d+)", hdr).group(1))
    assert len(fedd_lib.TIMER_NAMES) == n
    assert fedd_lib.TIMER_NAMES[int(re.search(r"FEDD_T_MULTISTEP\s*=\s*(\d+)", hdr).group(1))] == "multistep_state"


def test_compute_entries_need_a_gpu_context(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        c.mesh_set_dict(fedd_lib.structured_mesh(3, 1, 2))
        z = np.zeros(108)
        one = np.ones(1)
        f64 = fedd_lib._f64p
        calls = [lambda: c._L.fedd_multistep_begin(c._h, 2),
                 lambda: c._L.fedd_multistep_advance(c._h, 5, 1, fedd_lib._p(one, f64)),
                 lambda: c._L.fedd_multistep_set(c._h, 0, fedd_lib._p(z, f64)),
                 lambda: c._L.fedd_multistep_get(c._h, 0, fedd_lib._p(z, f64))]
        for k, call in enumerate(calls):
            assert call() != 0, "call %d succeeded on a host-only context" % k
            assert "needs a GPU context" in fedd_lib.lib().fedd_last_error().decode(), k
        with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
            c.multistep_begin(1)
        with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
            c.multistep_advance(5, [1.0])
        assert c.multistep_info() == (0, 0)             # the query needs no device: no history
    finally:
        c.close()


@pytest.mark.parametrize("order", [0, 3, -1])
def test_begin_refuses_other_orders(fedd_lib, order):
    c = fedd_lib.Context(device=-1)
    try:
        with pytest.raises(fedd_lib.FeddError, match=r"order must be 1 or 2 \(got %d\)" % order):
            c.multistep_begin(order)
    finally:
        c.close()


def test_advance_refuses_n_use_zero(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        with pytest.raises(fedd_lib.FeddError, match="n_use must be at least 1"):
            c.multistep_advance(5, [])
        one = np.ones(1)
        assert c._L.fedd_multistep_advance(c._h, 5, -2, fedd_lib._p(one, fedd_lib._f64p)) != 0
        assert "n_use must be at least 1 (got -2)" in fedd_lib.lib().fedd_last_error().decode()
    finally:
        c.close()


def test_slots_five_and_six_exist_and_seven_does_not(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        assert c.matrix_combine_current(5, 1.0, 0, 1.0) is False
        assert c.matrix_combine_current(5, 1.0, 6, 1.0) is False
        assert c.matrix_combine_current(6, 1.0, 5, 1.0) is False
        for m, a in ((7, 0), (0, 7), (-1, 0)):
            with pytest.raises(fedd_lib.FeddError, match="out of range"):
                c.matrix_combine_current(m, 1.0, a, 1.0)
    finally:
        c.close()

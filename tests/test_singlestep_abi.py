"""Single-step time stepping, C ABI (include/fedd_hip.h "Single-step time stepping", feddlib_amd/csrc/singlestep.hip): every new
entry is declared, exported and bound; on a host-only context each fails with "needs a GPU context", except fedd_stage_info; the
header's section carries the normative order that tests/test_gpu_singlestep.py restates."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("fedd_stage_begin", "fedd_stage_push", "fedd_stage_rhs", "fedd_block_merge_scaled", "fedd_stage_error", "fedd_stage_get",
       "fedd_stage_info")


def header():
    return open(os.path.join(ROOT, "include", "fedd_hip.h")).read()


def test_new_symbols_in_header_library_and_binding(fedd_lib):
    hdr = header()
    L = ctypes.CDLL(fedd_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in fedd_lib.SIGNATURES, name
    for meth in ("stage_begin", "stage_push", "stage_rhs", "stage_error", "stage_get", "stage_info", "block_merge_scaled"):
        assert hasattr(fedd_lib.Context, meth), meth
    assert (fedd_lib.STAGE_ERR_EUCLIDEAN, fedd_lib.STAGE_ERR_L2) == (0, 1)
    assert re.search(r"FEDD_STAGE_ERR_EUCLIDEAN\s*=\s*0", hdr) and re.search(r"FEDD_STAGE_ERR_L2\s*=\s*1", hdr)
    for cite in ("DAESolverInTime_def.hpp:384-516", "TimeSteppingTools.cpp:309-487", "BlockMatrix_def.hpp:371-392"):
        assert cite in hdr + open(os.path.join(ROOT, "feddlib_amd", "csrc", "singlestep.hip")).read(), cite
    from feddlib_amd import build
    assert "singlestep.hip" in build.SOURCES
    # the stages are not slots
    assert re.search(r"constexpr int MAX_AUX = 7;", open(os.path.join(ROOT, "feddlib_amd", "csrc", "fedd_internal.hpp")).read())


def test_calls_need_a_gpu_context(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        c.mesh_set_dict(fedd_lib.structured_mesh(2, 1, 2))
        z = np.zeros(64)
        e = ctypes.c_double()
        p = lambda a: fedd_lib._p(a, fedd_lib._f64p)
        calls = [lambda: c.stage_begin(2),
                 lambda: c.stage_push(4),
                 lambda: c.stage_rhs(5, 2, [-0.1], [0.0]),
                 lambda: c.block_merge_scaled(4, 2, 0.5, 1, -1),
                 lambda: c.stage_error(fedd_lib.STAGE_ERR_EUCLIDEAN, 5, 0, -1),
                 lambda: c._L.fedd_stage_error(c._h, fedd_lib.STAGE_ERR_L2, 5, 0, 0, ctypes.byref(e)),
                 lambda: c._L.fedd_stage_get(c._h, 0, p(z), p(z))]
        for k, call in enumerate(calls):
            rc = None
            try:
                rc = call()
            except fedd_lib.FeddError as err:
                assert "needs a GPU context" in str(err), (k, str(err))
                continue
            assert rc not in (None, 0), "call %d succeeded on a host-only context" % k
            assert "needs a GPU context" in fedd_lib.lib().fedd_last_error().decode(), k
    finally:
        c.close()


def test_info_is_a_query_that_needs_no_device(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        assert c.stage_info() == (0, 0, 0, 0)
        try:
            c.stage_get(0)
        except fedd_lib.FeddError as err:
            assert "stage 0 of 0" in str(err)
        else:
            raise AssertionError("stage_get without a stage succeeded")
    finally:
        c.close()


def test_header_states_the_normative_order_and_the_memory():
    hdr = header()
    blk = hdr[hdr.index("Single-step time stepping for nonlinear block problems"):hdr.index("int fedd_stage_info(")]
    flat = re.sub(r"[\s*]+", " ", blk)
    assert "NORMATIVE" in flat
    i0 = flat.index("t = rowsum(M[slot_m], u_0)")
    i1 = flat.index("mv = coeff_f[j] rowsum(F_j, u_j)")
    i2 = flat.index("mv = mv + (coeff_bt[j] rowsum(B^T[slot_bt], p_j))")
    i3 = flat.index("t = t + mv")
    i4 = flat.index("rhs[n_m .. n) = 0.0")
    assert i0 < i1 < i2 < i3 < i4
    assert "8 nnz(FULL velocity pattern) + 8 n bytes" in flat
    assert "NOT matrix slots" in flat
    assert "0.0 (B^T p_j)" in flat and "equals skipping the term" in flat
    assert "s_bt == 1.0 gives the bits of fedd_block_merge" in flat
    assert "no floating-point atomics" in flat

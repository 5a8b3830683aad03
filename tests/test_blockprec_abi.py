"""Block preconditioners, C ABI (include/fedd_hip.h "Block preconditioners", feddlib_amd/csrc/blockprec.hip): the four symbols
are declared, exported and bound, and the errors that need no device name their cause -- a NULL child, more than one rank,
child meshes of other sizes, an unmerged parent; fedd_matrix_import between host-only contexts needs a GPU context."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("fedd_matrix_import", "fedd_block_prec_attach", "fedd_block_prec_detach", "fedd_block_prec_info")


def test_new_symbols_in_header_library_and_binding(fedd_lib):
    hdr = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    L = ctypes.CDLL(fedd_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in fedd_lib.SIGNATURES, name
        assert hasattr(fedd_lib.Context, name[len("fedd_"):]), name
    for k, v in (("FEDD_BLOCKPREC_DIAGONAL", fedd_lib.BLOCKPREC_DIAGONAL), ("FEDD_BLOCKPREC_TRIANGULAR", fedd_lib.BLOCKPREC_TRIANGULAR)):
        assert int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) == v
    # the header cites what it replaces and states the apply
    for cite in ("PrecBlock2x2_def.hpp:114-164", "Preconditioner_def.hpp:979-1062", "NORMATIVE", "z_p = schur_scale * s",
                 "setLocalRowZero"):
        assert cite in hdr, cite
    n = int(re.search(r"FEDD_T_COUNT\s*=\s*(\d+)", hdr).group(1))
    assert len(fedd_lib.TIMER_NAMES) == n
    assert fedd_lib.TIMER_NAMES[int(re.search(r"FEDD_T_BLOCKPREC_BT\s*=\s*(\d+)", hdr).group(1))] == "blockprec_bt"


@pytest.fixture()
def three(fedd_lib):
    cs = [fedd_lib.Context(device=-1) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


def test_attach_errors_name_their_cause_without_a_device(fedd_lib, three):
    p, v, s = three
    with pytest.raises(fedd_lib.FeddError, match="null child: the velocity context is NULL"):
        p.block_prec_attach(fedd_lib.BLOCKPREC_DIAGONAL, None, s)
    with pytest.raises(fedd_lib.FeddError, match="null child: the Schur complement context is NULL"):
        p.block_prec_attach(fedd_lib.BLOCKPREC_DIAGONAL, v, None)
    with pytest.raises(fedd_lib.FeddError, match=r"kind 7 \(FEDD_BLOCKPREC_DIAGONAL = 1, FEDD_BLOCKPREC_TRIANGULAR = 2\)"):
        p.block_prec_attach(7, v, s)
    # an unmerged parent (nothing can be merged without a device)
    with pytest.raises(fedd_lib.FeddError, match="unmerged parent.*fedd_block_merge first"):
        p.block_prec_attach(fedd_lib.BLOCKPREC_TRIANGULAR, v, s, -1.0, 2)
    with pytest.raises(fedd_lib.FeddError, match="matrix slot 9 out of range"):
        p.block_prec_attach(fedd_lib.BLOCKPREC_TRIANGULAR, v, s, -1.0, 9)
    with pytest.raises(fedd_lib.FeddError, match="schur_scale must be a nonzero number"):
        p.block_prec_attach(fedd_lib.BLOCKPREC_DIAGONAL, v, s, 0.0)
    with pytest.raises(fedd_lib.FeddError, match="three different contexts"):
        p.block_prec_attach(fedd_lib.BLOCKPREC_DIAGONAL, v, v)
    assert p.block_prec_info() == {"kind": 0, "schur_scale": 1.0, "slot_bt": -1, "applies": 0}
    p.block_prec_detach()       # nothing attached: no error


def test_attach_refuses_child_meshes_of_other_sizes(fedd_lib, three):
    p, v, s = three
    p.mesh_set_dict(fedd_lib.structured_mesh(3, 1, 3))      # 64 nodes
    v.mesh_set_dict(fedd_lib.structured_mesh(3, 1, 2))      # 27
    s.mesh_set_dict(fedd_lib.structured_mesh(3, 1, 2))
    with pytest.raises(fedd_lib.FeddError, match="wrong sizes: the velocity child's mesh has 27 owned nodes, the parent's 64"):
        p.block_prec_attach(fedd_lib.BLOCKPREC_DIAGONAL, v, s)
    v.mesh_set_dict(fedd_lib.structured_mesh(3, 1, 3))
    s.mesh_set_dict(fedd_lib.structured_mesh(3, 1, 4))      # 125: more pressure than velocity nodes
    with pytest.raises(fedd_lib.FeddError, match="wrong sizes: the Schur complement child's mesh has 125 owned nodes, more than the parent's 64"):
        p.block_prec_attach(fedd_lib.BLOCKPREC_DIAGONAL, v, s)


def test_more_than_one_rank_is_refused(fedd_lib):
    L = fedd_lib.lib()
    hs = []
    try:
        for rank, nranks in ((0, 1), (0, 2), (0, 1)):
            h = ctypes.c_void_p()
            assert L.fedd_ctx_create(ctypes.byref(h), -1, None, rank, nranks) == 0
            hs.append(h)
        p, v2, s = hs
        assert L.fedd_block_prec_attach(p, 1, v2, s, -1.0, -1) != 0
        assert "one rank only (contexts with 1, 2 and 1 ranks were given)" in L.fedd_last_error().decode()
        assert L.fedd_block_prec_attach(v2, 1, p, s, -1.0, -1) != 0
        assert "one rank only (contexts with 2, 1 and 1 ranks were given)" in L.fedd_last_error().decode()
        assert L.fedd_matrix_import(p, v2, 0) != 0
        assert "fedd_matrix_import: one rank only" in L.fedd_last_error().decode()
    finally:
        for h in hs:
            L.fedd_ctx_destroy(h)


def test_matrix_import_needs_a_gpu_context(fedd_lib, three):
    p, v, s = three
    v.mesh_set_dict(fedd_lib.structured_mesh(3, 1, 2))
    with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
        v.matrix_import(p, 0)
    L = fedd_lib.lib()
    assert L.fedd_matrix_import(v._h, None, 0) != 0 and "null context" in L.fedd_last_error().decode()
    assert L.fedd_matrix_import(v._h, v._h, 0) != 0 and "same context" in L.fedd_last_error().decode()


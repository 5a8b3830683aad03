"""CPU side of the moving mesh (fedd_mesh_move): the entry points exist, a host-only context is refused with the words every
device call uses, a fresh context has moved nothing, and the header lists what a move keeps and what it drops."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fedd_mesh_move", "fedd_mesh_move_info", "fedd_mesh_coords_get")


def _header():
    return open(os.path.join(ROOT, "include", "fedd_hip.h")).read()


def test_the_three_symbols_exist(fedd_lib):
    txt = _header()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name + " is not declared in include/fedd_hip.h"
        assert name in fedd_lib.SIGNATURES
        assert hasattr(fedd_lib.lib(), name)
    for meth in ("mesh_move", "mesh_move_info", "mesh_coords"):
        assert hasattr(fedd_lib.Context, meth)


def test_timers_of_the_two_kernels(fedd_lib):
    txt = _header()
    assert fedd_lib.TIMER_NAMES[int(re.search(r"FEDD_T_MESH_MOVE\s*=\s*(\d+)", txt).group(1))] == "mesh_move"
    assert fedd_lib.TIMER_NAMES[int(re.search(r"FEDD_T_MOVE_CHECK\s*=\s*(\d+)", txt).group(1))] == "move_check"


def test_host_only_context_needs_a_gpu_context(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        m = fedd_lib.structured_mesh(2, 1, 2)
        c.mesh_set_dict(m)      # numbering only
        with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
            c.mesh_move(np.zeros_like(m["xyz"]))
        with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
            c.mesh_move(None)
        with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
            c.mesh_coords()
        assert c.mesh_move_info()["n_moves"] == 0
    finally:
        c.close()


def test_fresh_context_has_moved_nothing(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        info = c.mesh_move_info()
        assert (info["n_moves"], info["geometry_id"]) == (0, 0)
        assert info["min_det_ratio"] == 1.0
    finally:
        c.close()


def test_header_names_the_kept_and_the_dropped(fedd_lib):
    txt = _header()
    start = txt.index("Moving mesh")
    sec = txt[start:txt.index("int fedd_mesh_move(", start)]
    keeps, drops = sec.index("A move KEEPS"), sec.index("A move DROPS")
    assert keeps < drops
    kept, dropped = sec[keeps:drops], sec[drops:]
    for word in ("adjacency", "tile structures", "tile shapes", "patterns", "stored slots", "gather lists", "scratch",
                 "surface set", "Dirichlet flag tables", "halo plan", "time-stepping histories"):
        assert word in kept, "the kept list does not name: " + word
    for word in ("box lattice", "box structure", "coarse lattice", "classification", "per-element geometry",
                 "fedd_matrix_combine_current answers 0"):
        assert word in dropped, "the dropped list does not name: " + word
    for word in ("NOT cumulative", "NULL restores", "NOTHING is committed", "more than one rank", "ALE convection",
                 "interface distances"):
        assert word in sec, "the section does not say: " + word

"""CPU side of the interface distances and the scaled vector Laplacian: the entry points exist, a host-only context is refused
with the words every device call uses, the info query answers on a fresh context, and the header states the operation order."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fedd_interface_distance", "fedd_interface_distance_points", "fedd_interface_distance_set",
         "fedd_interface_distance_get", "fedd_interface_distance_info", "fedd_laplace_scale_get")


def _header():
    return open(os.path.join(ROOT, "include", "fedd_hip.h")).read()


def test_the_symbols_exist(fedd_lib):
    txt = _header()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name + " is not declared in include/fedd_hip.h"
        assert name in fedd_lib.SIGNATURES
        assert hasattr(fedd_lib.lib(), name)
    for meth in ("interface_distance", "interface_distance_points", "interface_distance_set", "interface_distances",
                 "interface_distance_info", "laplace_scale"):
        assert hasattr(fedd_lib.Context, meth)
    assert re.search(r"FEDD_FORM_LAPLACE_XDIM\s*=\s*7\b", txt) and fedd_lib.FORM_LAPLACE_XDIM == 7
    assert fedd_lib.TIMER_NAMES[int(re.search(r"FEDD_T_INTERFACE_DIST\s*=\s*(\d+)", txt).group(1))] == "interface_distance"
    assert len(fedd_lib.TIMER_NAMES) == int(re.search(r"FEDD_T_COUNT\s*=\s*(\d+)", txt).group(1))
    from feddlib_amd import build
    assert "interface_distance.hip" in build.SOURCES


def test_host_only_context_needs_a_gpu_context(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        m = fedd_lib.structured_mesh(2, 1, 2)
        c.mesh_set_dict(m)      # numbering only
        c.dofs = 2
        calls = [lambda: c.interface_distance([2]),
                 lambda: c.interface_distance_points(np.zeros((3, 2))),
                 lambda: c.interface_distance_set(np.zeros(m["xyz"].shape[0])),
                 lambda: c.interface_distance_set(None),
                 lambda: c.interface_distances(),
                 lambda: c.laplace_scale(),
                 lambda: c.assemble(fedd_lib.FORM_LAPLACE_XDIM, [0.03, 1000.0])]
        for k, call in enumerate(calls):
            with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
                call()
        assert c.interface_distance_info()["have"] is False
    finally:
        c.close()


def test_info_answers_on_a_fresh_context(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        info = c.interface_distance_info()
        assert info["have"] is False and info["n_interface"] == 0
        t = info["tile_points"]
        assert t >= 64 and t % 64 == 0 and 3 * 8 * t <= 64 * 1024    # a whole number of waves; the 3D tile fits the default LDS limit
        # every output may be NULL
        assert c._L.fedd_interface_distance_info(c._h, None, None, None) == 0
    finally:
        c.close()


def test_header_states_the_operation_order_and_the_lifetime():
    txt = _header()
    start = txt.index("Interface distances and the scaled vector Laplacian")
    sec = re.sub(r"[\s*]+", " ", txt[start:txt.index("int fedd_interface_distance(", start)])
    for cite in ("Domain_def.hpp:568-648", "MeshInterface_def.hpp:473-491", "FE_def.hpp:2225-2402", "Geometry_def.hpp:24-34",
                 "FE_def.hpp:2273-2278, 2343-2349"):
        assert cite in sec, cite
    for word in ("NORMATIVE", "min(1000.0", "ascending k", "no fused multiply-add", "monotone", "independent of the order",
                 "n_interface = 0", "IN FORCE", "fedd_mesh_move KEEPS", "releases them", "(d_0 + d_1 + d_2) / 3.0",
                 "(d_0 + d_1 + d_2 + d_3) / 4.0", "FIRST dim + 1 nodes", "mean < distance (strict)", "NO doSetZeros",
                 "no floating-point atomic", "names fedd_interface_distance"):
        assert word in sec, word
    mv = txt[txt.index("Moving mesh"):txt.index("int fedd_mesh_move(")]
    kept = mv[mv.index("A move KEEPS"):mv.index("A move DROPS")]
    assert "interface distances" in kept

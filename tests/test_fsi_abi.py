"""The FSI coupling entries of include/fedd_hip.h on host-only contexts: symbols and signatures, the "needs a GPU context"
errors, and the argument errors that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fedd_interface_match", "fedd_interface_match_sizes", "fedd_interface_match_get", "fedd_interface_match_info",
         "fedd_fsi_merge", "fedd_fsi_interface_rhs", "fedd_fsi_info", "fedd_fsi_prec_attach", "fedd_fsi_prec_detach",
         "fedd_fsi_prec_info"]


def test_symbols_and_signatures(fedd_lib):
    hdr = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(fedd_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in fedd_lib.SIGNATURES
        decl = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % n, code)
        assert decl, n
        assert len(decl.group(1).split(",")) == len(fedd_lib.SIGNATURES[n]), n
    for t, name in (("FEDD_T_FSI_MATCH", "fsi_match"), ("FEDD_T_FSI_MERGE", "fsi_merge"), ("FEDD_T_FSI_APPLY", "fsi_apply")):
        assert fedd_lib.TIMER_NAMES[int(re.search(r"%s\s*=\s*(\d+)" % t, hdr).group(1))] == name
    assert len(fedd_lib.TIMER_NAMES) == int(re.search(r"FEDD_T_COUNT\s*=\s*(\d+)", hdr).group(1))
    for m in ("interface_match", "interface_match_table", "interface_match_info", "fsi_merge", "fsi_interface_rhs", "fsi_info",
              "fsi_prec_attach", "fsi_prec_detach", "fsi_prec_info"):
        assert callable(getattr(fedd_lib.Context, m))


@pytest.fixture()
def hosts(fedd_lib):
    cs = [fedd_lib.Context(device=-1) for _ in range(3)]
    m = fedd_lib.structured_mesh(2, 1, 2)
    cs[0].mesh_set_dict(m)
    cs[1].mesh_set_dict(m)
    yield cs
    for c in cs:
        c.close()


def test_host_only_contexts_need_a_gpu(fedd_lib, hosts):
    f, s, cpl = hosts
    with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
        f.interface_match(s, [2])
    with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
        cpl.fsi_merge(f, s, 0.1)
    with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
        cpl.fsi_prec_attach(f, s)
    with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
        _rhs = np.zeros(4)
        fedd_lib._chk(cpl._L.fedd_fsi_interface_rhs(cpl._h, fedd_lib._p(_rhs, fedd_lib._f64p)))


def test_argument_errors_without_a_device(fedd_lib, hosts):
    f, s, cpl = hosts
    with pytest.raises(fedd_lib.FeddError, match="same context"):
        f.interface_match(f, [2])
    with pytest.raises(fedd_lib.FeddError, match="null context"):
        f.interface_match(None, [2])
    with pytest.raises(fedd_lib.FeddError, match="empty interface"):
        f.interface_match(s, np.zeros(0, dtype=np.int32))
    with pytest.raises(fedd_lib.FeddError, match="dt must be positive"):
        cpl.fsi_merge(f, s, 0.0)
    with pytest.raises(fedd_lib.FeddError, match="dt must be positive"):
        cpl.fsi_merge(f, s, -1.0)
    with pytest.raises(fedd_lib.FeddError, match="three different contexts"):
        cpl.fsi_merge(f, f, 0.1)
    with pytest.raises(fedd_lib.FeddError, match="null context"):
        cpl.fsi_merge(None, s, 0.1)
    with pytest.raises(fedd_lib.FeddError, match="null child: the fluid"):
        cpl.fsi_prec_attach(None, s)
    with pytest.raises(fedd_lib.FeddError, match="null child: the structure"):
        cpl.fsi_prec_attach(f, None)
    with pytest.raises(fedd_lib.FeddError, match="no matched interface"):
        f.interface_match_table()
    with pytest.raises(fedd_lib.FeddError, match="does not hold a coupled system"):
        cpl.fsi_info()
    with pytest.raises(fedd_lib.FeddError, match="null pointer"):
        fedd_lib._chk(cpl._L.fedd_fsi_interface_rhs(cpl._h, None))
    # the queries that need no device
    assert f.interface_match_info() == {"have": False, "n_pairs": 0, "max_pair_distance": 0.0, "tile_points": 1024}
    assert cpl.fsi_prec_info() == {"attached": False, "applies": 0}
    cpl.fsi_prec_detach()       # nothing attached: not an error


def test_more_than_one_rank_is_refused(fedd_lib):
    a = fedd_lib.Context(device=-1, rank=0, nranks=2)
    b = fedd_lib.Context(device=-1)
    c = fedd_lib.Context(device=-1)
    try:
        with pytest.raises(fedd_lib.FeddError, match="one rank only"):
            a.interface_match(b, [2])
        with pytest.raises(fedd_lib.FeddError, match="one rank only"):
            c.fsi_merge(a, b, 0.1)
        with pytest.raises(fedd_lib.FeddError, match="one rank only"):
            c.fsi_prec_attach(a, b)
    finally:
        for x in (a, b, c):
            x.close()

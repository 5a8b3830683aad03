"""fedd_interface_match (include/fedd_hip.h "FSI coupling", feddlib_amd/csrc/fsi.hip) against tests/fsi_ref.py: the table id
for id (integer equality), its lifetime, and its errors.

Shapes: 2D P2 on 4 x 4 cells (9 interface nodes); the same interface split into two flags, in both orders; 3D P1 on 32^3 cells,
whose face has 33^2 = 1089 nodes and so straddles the rank kernel's LDS tile of 1024 points.  "Contexts on different devices"
needs two GPUs and is not run here; more than one rank and host-only contexts are in tests/test_fsi_abi.py."""
import numpy as np
import pytest

import fsi_pair
import fsi_ref
from fsi_pair import FLAG

pytestmark = pytest.mark.gpu


def contexts(lib, mf, ms):
    f, s = lib.Context(device=0), lib.Context(device=0)
    f.mesh_set_dict(mf)
    s.mesh_set_dict(ms)
    return f, s


def check_table(lib, mf, ms, flags):
    f, s = contexts(lib, mf, ms)
    try:
        n = f.interface_match(s, flags)
        got = f.interface_match_table()
        ref = fsi_pair.reference_table(mf, ms, flags)
        assert n == ref[0].shape[0]
        for a, b in zip(got, ref):
            assert np.array_equal(a, b)
        for a, b in zip(s.interface_match_table(), ref):      # both contexts hold the same table
            assert np.array_equal(a, b)
        info = f.interface_match_info()
        assert info["have"] and info["n_pairs"] == n and info["max_pair_distance"] == 0.0
        return got
    finally:
        f.close()
        s.close()


def test_p2_square(fedd_lib):
    mf, ms = fsi_pair.pair(fedd_lib.structured_mesh_p2(2, 1, 4))
    i_f, _, ptr = check_table(fedd_lib, mf, ms, [FLAG])
    assert i_f.shape[0] == 9 and list(ptr) == [0, 9]


@pytest.mark.parametrize("flags", [[FLAG, FLAG + 1], [FLAG + 1, FLAG]])
def test_two_flags_in_both_orders(fedd_lib, flags):
    mf, ms = fsi_pair.pair(fedd_lib.structured_mesh_p2(2, 1, 4))
    for m in (mf, ms):
        x = fsi_ref.unique_coords(m)
        m["flag_uni"][(m["flag_uni"] == FLAG) & (x[:, 1] > 0.6)] = FLAG + 1
    _, _, ptr = check_table(fedd_lib, mf, ms, flags)
    assert sorted(np.diff(ptr).tolist()) == [4, 5]      # y = 0.625 ... 1 | y = 0 ... 0.5


def test_cube_face_straddles_the_lds_tile(fedd_lib):
    mf, ms = fsi_pair.pair(fedd_lib.structured_mesh(3, 1, 32))
    h = fedd_lib.Context(device=-1)
    tile = h.interface_match_info()["tile_points"]
    h.close()
    i_f, _, _ = check_table(fedd_lib, mf, ms, [FLAG])
    assert i_f.shape[0] == 33 * 33 and tile < i_f.shape[0] < 2 * tile


def test_permuted_structure_gives_the_same_pairs(fedd_lib):
    mf, ms = fsi_pair.pair(fedd_lib.structured_mesh_p2(2, 1, 4))
    perm = np.random.default_rng(5).permutation(ms["gid_uni"].shape[0])
    mp = dict(ms)
    mp["gid_uni"] = ms["gid_uni"][perm]
    mp["flag_uni"] = ms["flag_uni"][perm]
    f, s = contexts(fedd_lib, mf, ms)
    g, t = contexts(fedd_lib, mf, mp)
    try:
        f.interface_match(s, [FLAG])
        g.interface_match(t, [FLAG])
        a_f, a_s, _ = f.interface_match_table()
        b_f, b_s, _ = g.interface_match_table()
        assert np.array_equal(a_f, b_f)
        assert np.array_equal(ms["gid_uni"][a_s], mp["gid_uni"][b_s]) and not np.array_equal(a_s, b_s)
    finally:
        for c in (f, s, g, t):
            c.close()


def test_lifetime(fedd_lib):
    mf, ms = fsi_pair.pair(fedd_lib.structured_mesh_p2(2, 1, 4))
    f, s = contexts(fedd_lib, mf, ms)
    cpl = fedd_lib.Context(device=0)
    try:
        f.interface_match(s, [FLAG])
        before = f.interface_match_table()
        # a move keeps the table, and a second match still pairs at the REFERENCE coordinates
        d = np.zeros_like(mf["xyz"])
        d[:, 1] = 0.05 * mf["xyz"][:, 0] * (1.0 - mf["xyz"][:, 1]) * mf["xyz"][:, 1]
        f.mesh_move(d)
        assert f.interface_match_info()["have"]
        for a, b in zip(f.interface_match_table(), before):
            assert np.array_equal(a, b)
        f.interface_match(s, [FLAG])
        assert f.interface_match_info()["max_pair_distance"] == 0.0
        for a, b in zip(f.interface_match_table(), before):
            assert np.array_equal(a, b)
        # mesh_set on either side drops it on both
        s.mesh_set_dict(ms)
        assert not f.interface_match_info()["have"] and not s.interface_match_info()["have"]
        with pytest.raises(fedd_lib.FeddError, match="no matched interface"):
            f.interface_match_table()
        with pytest.raises(fedd_lib.FeddError, match="no matched interface between exactly these two contexts"):
            cpl.fsi_merge(f, s, 0.1)
    finally:
        for c in (cpl, f, s):
            c.close()


def test_errors_name_their_cause(fedd_lib):
    mf, ms = fsi_pair.pair(fedd_lib.structured_mesh_p2(2, 1, 4))
    xs = fsi_ref.unique_coords(ms)
    # one more structure node on the flag
    extra = dict(ms)
    extra["flag_uni"] = ms["flag_uni"].copy()
    extra["flag_uni"][np.nonzero(xs[:, 0] > 1.9)[0][0]] = FLAG
    f, s = contexts(fedd_lib, mf, extra)
    try:
        with pytest.raises(fedd_lib.FeddError, match="different number of nodes.*flag %d has 9 fluid and 10 structure" % FLAG):
            f.interface_match(s, [FLAG])
        assert not f.interface_match_info()["have"]
        with pytest.raises(fedd_lib.FeddError, match="empty interface"):
            f.interface_match(s, [99])
    finally:
        f.close()
        s.close()
    # two structure nodes of the interface at the same place
    twin = dict(ms)
    twin["xyz"] = ms["xyz"].copy()
    on = np.nonzero(ms["flag_uni"] == FLAG)[0]
    rep = {int(g): i for i, g in enumerate(ms["gid_rep"])}
    twin["xyz"][rep[int(ms["gid_uni"][on[3]])]] = twin["xyz"][rep[int(ms["gid_uni"][on[5]])]]
    f, s = contexts(fedd_lib, mf, twin)
    try:
        with pytest.raises(fedd_lib.FeddError, match="structure nodes %d and %d .*identical coordinates" % (on[3], on[5])):
            f.interface_match(s, [FLAG])
    finally:
        f.close()
        s.close()
    # a context without a mesh, meshes of different dimension
    f, s = contexts(fedd_lib, mf, ms)
    e = fedd_lib.Context(device=0)
    try:
        with pytest.raises(fedd_lib.FeddError, match="the structure carries no mesh"):
            f.interface_match(e, [FLAG])
        e.mesh_set_dict(fedd_lib.structured_mesh(3, 1, 2))
        with pytest.raises(fedd_lib.FeddError, match="different dimension"):
            f.interface_match(e, [FLAG])
    finally:
        for c in (e, f, s):
            c.close()

"""fedd_interface_distance* on the GPU: the distances are, bit for bit, those of the numpy restatement of the reference loop
(tests/interface_ref.py) -- the kernel rounds every product and every sum on its own, takes the minimum of the squared distances
and one correctly rounded root, which is the minimum of the roots.

Meshes, the smallest that reach each shape: structured 2D P1 / P2 with 5 x 4 cells, structured 3D P1 / P2 with 3 x 3 x 2 cells,
one distorted lattice (seeded jitter of the interior nodes), one and two flags; point sets of 1, tile, tile + 1 and
2 tile + 3 points (the LDS tile of fedd_interface_distance_info) against a mesh of 30 nodes (less than one workgroup) and one of
342 nodes (two workgroups, the second partly filled)."""
import numpy as np
import pytest

import interface_ref as ir
import stress_ref as sr

pytestmark = pytest.mark.gpu

_meshes = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mesh(lib, case):
    if case not in _meshes:
        if case == "square_p1":
            m = lib.structured_mesh(2, 1, [5, 4])
        elif case == "square_p2":
            m = lib.structured_mesh_p2(2, 1, [5, 4])
        elif case == "cube_p1":
            m = lib.structured_mesh(3, 1, [3, 3, 2])
        elif case == "cube_p2":
            m = lib.structured_mesh_p2(3, 1, [3, 3, 2])
        elif case == "distorted":
            m = sr.jitter(lib.structured_mesh(3, 1, 3), amplitude=0.25, seed=5)
        elif case == "square_18":       # 19 x 18 = 342 nodes: no multiple of the block size, two workgroups
            m = lib.structured_mesh(2, 1, [18, 17])
        _meshes[case] = m
    return _meshes[case]


@pytest.fixture(scope="module")
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("case", ["square_p1", "square_p2", "cube_p1", "cube_p2", "distorted"])
@pytest.mark.parametrize("flags", [(2,), (2, 3)])
def test_flags_variant_is_the_restatement_bit_for_bit(fedd_lib, ctx, case, flags):
    m = mesh(fedd_lib, case)
    ctx.mesh_set_dict(m)
    n = ctx.interface_distance(list(flags))
    side = ir.interface_nodes(m, flags)
    assert n == side.shape[0] > 0
    d = ctx.interface_distances()
    assert np.array_equal(bits(d), bits(ir.distances_to_flags(m, flags)))
    assert np.all(d[side] == 0.0)                       # an interface node has distance 0.0
    assert np.all(d[np.setdiff1d(np.arange(d.shape[0]), side)] > 0.0)
    info = ctx.interface_distance_info()
    assert info["have"] and info["n_interface"] == n
    if case == "square_p1" and flags == (2,):
        assert np.array_equal(bits(d), bits(m["xyz"][:, 0]))        # the known answer: the distance to the side x = 0 is x


@pytest.mark.parametrize("case", ["square_p1", "square_18", "distorted"])
def test_points_variant_straddles_the_tile(fedd_lib, ctx, case):
    m = mesh(fedd_lib, case)
    dim = m["dim"]
    ctx.mesh_set_dict(m)
    T = ctx.interface_distance_info()["tile_points"]
    rng = np.random.default_rng(17)
    for n_pts in (1, T, T + 1, 2 * T + 3):
        pts = rng.uniform(-0.25, 1.25, (n_pts, dim))
        pts[n_pts - 1] = m["xyz"][7] + 1e-3            # the last point of the last (partly filled) tile is the nearest of node 7
        ctx.interface_distance_points(pts)
        d = ctx.interface_distances()
        ref = ir.distances(m["xyz"], pts)
        assert np.array_equal(bits(d), bits(ref)), n_pts
        assert ctx.interface_distance_info()["n_interface"] == n_pts
        # a permutation of the points gives the same bits
        ctx.interface_distance_points(pts[rng.permutation(n_pts)])
        assert np.array_equal(bits(ctx.interface_distances()), bits(d)), n_pts


def test_far_points_and_no_points_give_the_cap(fedd_lib, ctx):
    m = mesh(fedd_lib, "cube_p1")
    ctx.mesh_set_dict(m)
    n = m["xyz"].shape[0]
    ctx.interface_distance_points(np.array([[5000.0, 0.0, 0.0], [0.0, -3000.0, 10.0]]))
    assert np.array_equal(ctx.interface_distances(), np.full(n, 1000.0))
    ctx.interface_distance_points(np.zeros((0, 3)))
    assert np.array_equal(ctx.interface_distances(), np.full(n, 1000.0))
    assert ctx.interface_distance_info() == {"have": True, "n_interface": 0, "tile_points": ctx.interface_distance_info()["tile_points"]}
    assert ctx.interface_distance([77]) == 0            # no node carries the flag: not an error
    assert np.array_equal(ctx.interface_distances(), np.full(n, 1000.0))
    assert ctx.interface_distance([]) == 0
    # one point inside the cap among far ones
    pts = np.array([[5000.0, 0.0, 0.0], [300.0, 400.0, 0.0]])
    ctx.interface_distance_points(pts)
    assert np.array_equal(bits(ctx.interface_distances()), bits(ir.distances(m["xyz"], pts)))


def test_set_get_round_trip_and_release(fedd_lib, ctx):
    m = mesh(fedd_lib, "square_p2")
    ctx.mesh_set_dict(m)
    v = np.random.default_rng(2).uniform(0.0, 2000.0, m["xyz"].shape[0])
    v[3], v[4] = -0.0, np.nextafter(1.0, 2.0)
    ctx.interface_distance_set(v)
    assert np.array_equal(bits(ctx.interface_distances()), bits(v))     # stored as given: no cap, no rounding
    assert ctx.interface_distance_info()["n_interface"] == 0
    ctx.interface_distance_set(None)
    assert not ctx.interface_distance_info()["have"]
    with pytest.raises(fedd_lib.FeddError, match="no distances"):
        ctx.interface_distances()


def test_distances_survive_a_move_and_go_with_the_mesh(fedd_lib, ctx):
    m = mesh(fedd_lib, "cube_p1")
    ctx.mesh_set_dict(m)
    ctx.interface_distance([2])
    d0 = ctx.interface_distances()
    x = m["xyz"]
    disp = 0.05 * np.stack([np.sin(np.pi * x[:, 0]) * x[:, 1], 0.0 * x[:, 0], np.sin(np.pi * x[:, 2])], axis=1)
    ctx.mesh_move(disp)
    assert ctx.interface_distance_info()["have"]
    assert np.array_equal(bits(ctx.interface_distances()), bits(d0))            # kept: the reference never recomputes them
    # a call after the move takes the coordinates in force
    ctx.interface_distance([2])
    assert np.array_equal(bits(ctx.interface_distances()), bits(ir.distances_to_flags(m, 2, xyz=x + disp)))
    ctx.mesh_set_dict(m)
    assert not ctx.interface_distance_info()["have"]
    with pytest.raises(fedd_lib.FeddError, match="no distances"):
        ctx.interface_distances()


def test_errors(fedd_lib):
    c = fedd_lib.Context(device=0)
    try:
        with pytest.raises(fedd_lib.FeddError, match="fedd_mesh_set first"):
            c.interface_distance([2])
        with pytest.raises(fedd_lib.FeddError, match="fedd_mesh_set first"):
            c.interface_distance_points(np.zeros((1, 1)))
        with pytest.raises(fedd_lib.FeddError, match="fedd_mesh_set first"):
            c.interface_distance_set(np.zeros(1))
        m = mesh(fedd_lib, "square_p1")
        c.mesh_set_dict(m)
        with pytest.raises(fedd_lib.FeddError, match="no distances"):
            c.interface_distances()
        z = np.zeros(4)
        assert c._L.fedd_interface_distance_points(c._h, -1, fedd_lib._p(z, fedd_lib._f64p)) != 0
        assert "negative number of points" in fedd_lib.lib().fedd_last_error().decode()
        fl = np.zeros(1, dtype=np.int32)
        assert c._L.fedd_interface_distance(c._h, -2, fedd_lib._p(fl, fedd_lib._i32p), None) != 0
        assert "negative number of flags" in fedd_lib.lib().fedd_last_error().decode()
        assert c._L.fedd_interface_distance_points(c._h, 3, None) != 0
        assert "null point array" in fedd_lib.lib().fedd_last_error().decode()
        assert not c.interface_distance_info()["have"]          # a refused call leaves nothing behind
    finally:
        c.close()
    # more than one rank (host-callback transport, no communicator needed for the check)
    c2 = fedd_lib.Context(device=0, rank=0, nranks=2)
    try:
        c2.mesh_set_dict(mesh(fedd_lib, "square_p1"))
        with pytest.raises(fedd_lib.FeddError, match="one rank only"):
            c2.interface_distance([2])
        with pytest.raises(fedd_lib.FeddError, match="one rank only"):
            c2.interface_distance_points(np.zeros((1, 2)))
        with pytest.raises(fedd_lib.FeddError, match="one rank only"):
            c2.interface_distance_set(np.zeros(mesh(fedd_lib, "square_p1")["xyz"].shape[0]))
    finally:
        c2.close()

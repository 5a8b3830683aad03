"""Structured P2 generator (fedd_mesh_structured_p2_build, fedd_mesh_p2_vertices_first), CPU side: bit equality with the numpy
restatement of the reference's P2 branches (structured_p2_ref.py) on every rank of the smallest decompositions that have
interior, face, edge and corner ranks, and properties that do not depend on the restatement."""
import itertools
import math

import numpy as np
import pytest

import fedd_oracle as fo
import structured_p2_ref as ref

CASES = [(2, 1, 3), (2, 2, 2), (2, 3, 2), (3, 1, 2), (3, 2, 2), (3, 1, 3)]
EDGE_SLOT_2D = {(0, 1): 3, (1, 2): 4, (0, 2): 5}
EDGE_SLOT_3D = {(0, 1): 4, (1, 2): 5, (0, 2): 6, (0, 3): 7, (1, 3): 8, (2, 3): 9}


def edge_slots(dim):
    return EDGE_SLOT_3D if dim == 3 else EDGE_SLOT_2D


@pytest.fixture(scope="module")
def meshes(fedd_lib):
    """every rank's mesh of every case, built once"""
    return {(dim, N, M): [fedd_lib.structured_mesh_p2(dim, N, M, rank) for rank in range(N ** dim)] for dim, N, M in CASES}


@pytest.mark.parametrize("dim,N,M", CASES)
def test_generator_matches_reference_restatement(meshes, dim, N, M):
    for rank, m in enumerate(meshes[(dim, N, M)]):
        r = ref.build(dim, N, M, rank)
        np.testing.assert_array_equal(m["conn"], r["conn"])
        assert m["xyz"].tobytes() == r["xyz"].tobytes(), "coordinates differ in some bit on rank %d" % rank
        np.testing.assert_array_equal(m["gid_rep"], r["gid_rep"])
        np.testing.assert_array_equal(m["gid_uni"], r["gid_uni"])
        np.testing.assert_array_equal(m["flag_rep"], r["flag_rep"])
        np.testing.assert_array_equal(m["flag_uni"], r["flag_uni"])
        np.testing.assert_array_equal(m["owner_rep"], r["owner"])
        np.testing.assert_array_equal(m["elem_flag"], r["eflag"])


@pytest.mark.parametrize("dim,N,M", [(2, 2, 2), (3, 2, 2)])
def test_flags_option_0_keeps_the_generator_flag(fedd_lib, dim, N, M):
    for rank in range(N ** dim):
        m = fedd_lib.structured_mesh_p2(dim, N, M, rank, flags_option=0)
        r = ref.build(dim, N, M, rank, flags_option=0)
        np.testing.assert_array_equal(m["flag_rep"], r["flag_rep"])
        np.testing.assert_array_equal(m["flag_uni"], r["flag_uni"])
        on_side = ((m["xyz"] == 0.0) | (m["xyz"] == 1.0)).any(axis=1)
        np.testing.assert_array_equal(m["flag_rep"], on_side.astype(np.int32))


@pytest.mark.parametrize("dim,N,M", CASES)
def test_mid_nodes_are_edge_midpoints(meshes, dim, N, M):
    for m in meshes[(dim, N, M)]:
        X, conn = m["xyz"], m["conn"]
        for (a, b), s in edge_slots(dim).items():
            mid = 0.5 * (X[conn[:, a]] + X[conn[:, b]])
            assert X[conn[:, s]].tobytes() == mid.tobytes(), "slot %d is not the midpoint of (%d, %d) bit for bit" % (s, a, b)


@pytest.mark.parametrize("dim,N,M", CASES)
def test_elements_are_nondegenerate_and_fill_the_domain(meshes, dim, N, M):
    vols = []
    for m in meshes[(dim, N, M)]:
        X = m["xyz"][m["conn"][:, :dim + 1]]
        B = np.transpose(X[:, 1:, :] - X[:, :1, :], (0, 2, 1))
        det = np.abs(np.linalg.det(B))
        assert (det > 0).all()
        vols.extend((det / math.factorial(dim)).tolist())
    assert abs(math.fsum(vols) - 1.0) <= 1e-14


@pytest.mark.parametrize("dim,N,M", CASES)
def test_faces_conform(meshes, dim, N, M):
    """Global view through the gids: an interior face is shared by exactly two elements, which see the same mid nodes on it;
    a face on a side of the domain is held by exactly one element."""
    slots = edge_slots(dim)
    faces = {}
    coord = {}
    for m in meshes[(dim, N, M)]:
        g = m["gid_rep"][m["conn"]]
        for gi, x in zip(m["gid_rep"], m["xyz"]):
            coord[int(gi)] = x
        for skip in range(dim + 1):
            vs = [v for v in range(dim + 1) if v != skip]
            mids = [slots[p] for p in itertools.combinations(vs, 2)]
            for row in g:
                key = tuple(sorted(int(row[v]) for v in vs))
                faces.setdefault(key, []).append(tuple(sorted(int(row[s]) for s in mids)))
    n_bnd = 0
    for key, held in faces.items():
        X = np.array([coord[v] for v in key])
        on_side = bool(((X == 0.0).all(axis=0) | (X == 1.0).all(axis=0)).any())
        if on_side:
            assert len(held) == 1, "boundary face %s is held by %d elements" % (key, len(held))
            n_bnd += 1
        else:
            assert len(held) == 2, "interior face %s is held by %d elements" % (key, len(held))
            assert held[0] == held[1], "the two elements at face %s see different mid nodes" % (key,)
    cells = N * M
    assert n_bnd == (4 * cells if dim == 2 else 6 * 2 * cells * cells)


@pytest.mark.parametrize("dim,N,M", CASES)
def test_unique_maps_partition_the_lattice(meshes, dim, N, M):
    n1 = 2 * N * M + 1
    count = np.zeros(n1 ** dim, dtype=np.int64)
    for rank, m in enumerate(meshes[(dim, N, M)]):
        count[m["gid_uni"]] += 1
        np.testing.assert_array_equal(m["gid_uni"], m["gid_rep"][m["owner_rep"] == rank])
        assert m["n_global"] == n1 ** dim
    assert (count == 1).all()


@pytest.mark.parametrize("dim,N,M", CASES)
def test_vertices_are_the_p1_mesh_and_perm_puts_them_first(fedd_lib, meshes, dim, N, M):
    """FE::assemblyDivAndDivT walks the velocity and pressure element lists in step: the vertices of P2 element T are the
    nodes of P1 element T under (r,s,t) -> (2r,2s,2t)."""
    p2m = 2 * M + 1
    for rank, m in enumerate(meshes[(dim, N, M)]):
        p1 = fedd_lib.structured_mesh(dim, N, M, rank)
        c1 = p1["conn"].astype(np.int64)
        r, s, t = c1 % (M + 1), (c1 // (M + 1)) % (M + 1), c1 // (M + 1) ** 2
        np.testing.assert_array_equal(m["conn"][:, :dim + 1], 2 * r + p2m * (2 * s + p2m * 2 * t))
        perm, n_p1 = m["perm"], m["n_p1"]
        assert n_p1 == p1["xyz"].shape[0]
        np.testing.assert_array_equal(np.sort(perm), np.arange(m["xyz"].shape[0]))
        assert m["xyz"][perm[:n_p1]].tobytes() == p1["xyz"].tobytes()
        np.testing.assert_array_equal(perm[n_p1:], np.sort(perm[n_p1:]))       # the rest keep their reference order
        # the renumbered mesh is the same mesh
        v = fedd_lib.structured_mesh_p2(dim, N, M, rank, vertices_first=True)
        assert v["xyz"].tobytes() == m["xyz"][perm].tobytes()
        assert v["xyz"][v["conn"]].tobytes() == m["xyz"][m["conn"]].tobytes()
        np.testing.assert_array_equal(v["conn"][:, :dim + 1], p1["conn"])
        np.testing.assert_array_equal(v["gid_rep"][v["conn"]], m["gid_rep"][m["conn"]])
        np.testing.assert_array_equal(v["gid_uni"], v["gid_rep"][v["owner_rep"] == rank])
        flag_of = dict(zip(m["gid_uni"].tolist(), m["flag_uni"].tolist()))
        assert [flag_of[g] for g in v["gid_uni"].tolist()] == v["flag_uni"].tolist()


@pytest.mark.parametrize("dim,N,M", [(2, 1, 3), (3, 1, 2), (2, 2, 2)])
@pytest.mark.parametrize("vertices_first", [False, True])
def test_p2_surfaces(fedd_lib, dim, N, M, vertices_first):
    for rank in range(N ** dim):
        m = fedd_lib.structured_mesh_p2(dim, N, M, rank, vertices_first=vertices_first)
        s1, f1 = fedd_lib.structured_surfaces(dim, N, M, rank)
        s2, f2 = fedd_lib.structured_surfaces(dim, N, M, rank, p2=True, vertices_first=vertices_first)
        np.testing.assert_array_equal(f1, f2)
        p1 = fedd_lib.structured_mesh(dim, N, M, rank)
        X = m["xyz"]
        assert X[s2[:, :dim]].tobytes() == p1["xyz"][s1].tobytes()
        pairs = [(0, 1)] if dim == 2 else [(0, 1), (1, 2), (0, 2)]       # the slot order of fedd_mesh_p2_surfaces
        for k, (a, b) in enumerate(pairs):
            assert X[s2[:, dim + k]].tobytes() == (0.5 * (X[s2[:, a]] + X[s2[:, b]])).tobytes()
        # every surface element is a face of a volume element
        nodes = [set(row.tolist()) for row in m["conn"]]
        for row in s2:
            assert any(set(row.tolist()) <= e for e in nodes)


def test_structured_p2_generator_errors(fedd_lib):
    with pytest.raises(fedd_lib.FeddError, match="H/h"):
        fedd_lib.structured_mesh_p2(3, 1, 0)
    with pytest.raises(fedd_lib.FeddError, match="rank"):
        fedd_lib.structured_mesh_p2(3, 2, 2, rank=8)
    with pytest.raises(fedd_lib.FeddError, match="rank"):
        fedd_lib.structured_mesh_p2(2, 2, 2, rank=-1)
    with pytest.raises(fedd_lib.FeddError, match="dimension"):
        fedd_lib.structured_mesh_p2(1, 1, 2)
    with pytest.raises(fedd_lib.FeddError, match="flags option 7"):
        fedd_lib.structured_mesh_p2(2, 1, 2, flags_option=7)
    with pytest.raises(fedd_lib.FeddError, match="ghost"):
        fedd_lib.structured_surfaces(2, 1, 2, ghosts=True, p2=True)


@pytest.mark.parametrize("dim,M", [(2, 3), (3, 2)])
@pytest.mark.parametrize("vertices_first", [False, True])
def test_oracle_p2_laplace_on_the_lattice(fedd_lib, dim, M, vertices_first):
    """The oracle's P2 Laplace form on the new mesh: constants are in the kernel and u = x^2, which P2 holds exactly, has the
    energy int |grad u|^2 = int 4 x^2 = 4/3.  Bounds: a row of K has at most ~30 (2D) / ~70 (3D) entries of size O(1), so a row
    sum and the quadratic form carry a few hundred eps of rounding; 1e-13 is ~450 eps."""
    m = fedd_lib.structured_mesh_p2(dim, 1, M, vertices_first=vertices_first)
    om = fo.Mesh(dim=dim, fe="P2", conn=m["conn"], xyz=m["xyz"], gid_rep=m["gid_rep"], flag_rep=m["flag_rep"],
                 gid_uni=m["gid_uni"], flag_uni=m["flag_uni"], xyz_uni=None, n_global=m["n_global"])
    K = fo.assembly_laplace(om)
    assert abs(K @ np.ones(K.shape[0])).max() <= 1e-13
    u = np.zeros(K.shape[0])
    u[m["gid_rep"]] = m["xyz"][:, 0] ** 2
    assert abs(u @ (K @ u) - 4.0 / 3.0) <= 1e-13

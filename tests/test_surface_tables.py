"""Host side of the surface load vector (no GPU): the 1-D quadrature rules and line bases, the integrated basis
functions of the boundary elements, the boundary faces of a mesh, the structured surface elements with their flags
and the P2 surface elements."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_line_quadrature_integrates_monomials(fedd_lib, degree):
    pts, w = fedd_lib.fe_quadrature(1, degree)
    assert pts.shape == (w.shape[0], 1) and ((pts > 0) & (pts < 1)).all()
    for k in range(max(degree, 1) + 1):                       # int_0^1 x^k = 1 / (k + 1)
        err = abs(w @ pts[:, 0] ** k - 1.0 / (k + 1))
        assert err <= 4e-16, "degree %d, x^%d: %g" % (degree, k, err)


def test_line_quadrature_rejects_higher_degrees(fedd_lib):
    with pytest.raises(fedd_lib.FeddError, match="up to degree 3"):
        fedd_lib.fe_quadrature(1, 4)


@pytest.mark.parametrize("nen,nodes", [(2, [0.0, 1.0]), (3, [0.0, 1.0, 0.5])])
def test_line_bases_partition_of_unity_and_nodal(fedd_lib, nen, nodes):
    phi, dphi = fedd_lib.fe_basis(1, nen, 3)
    pts, _ = fedd_lib.fe_quadrature(1, 3)
    assert np.abs(phi.sum(axis=1) - 1.0).max() <= 4e-16 and np.abs(dphi.sum(axis=1)).max() <= 2e-15
    # nodal: the Lagrange polynomials on the nodes (end, end, mid), evaluated at the quadrature points
    for i, xi in enumerate(nodes):
        lag = np.ones(pts.shape[0])
        for j, xj in enumerate(nodes):
            if j != i:
                lag *= (pts[:, 0] - xj) / (xi - xj)
        assert np.abs(phi[:, i] - lag).max() <= 4e-16, (nen, i)


@pytest.mark.parametrize("sdim,nsn,expect", [(1, 2, [1 / 2, 1 / 2]), (1, 3, [1 / 6, 1 / 6, 2 / 3]),
                                             (2, 3, [1 / 6, 1 / 6, 1 / 6]), (2, 6, [0, 0, 0, 1 / 6, 1 / 6, 1 / 6])])
def test_integrated_basis_of_the_boundary_elements(fedd_lib, sdim, nsn, expect):
    """sum_q w_q phi_q,i at the degree of the surface form, determineDegree(dim - 1, FEType, Std): P1 -> 1, P2 -> 2"""
    degree = 2 if nsn in (3, 6) and (sdim, nsn) != (2, 3) else 1
    for extra in range(0, 2):
        _, w = fedd_lib.fe_quadrature(sdim, degree + extra)
        phi, _ = fedd_lib.fe_basis(sdim, nsn, degree + extra)
        err = np.abs(w @ phi - np.array(expect)).max()
        assert err <= 1e-15, "sum_q w_q phi_q,i off by %g" % err


def face_set(a):
    return set(map(tuple, np.sort(np.asarray(a), axis=1)))


@pytest.mark.parametrize("name,dim", [("tetrahedron.mesh", 3), ("square.mesh", 2), ("DFG3DCylinder_1k.mesh", 3)])
def test_boundary_faces_are_the_files_surface_entities(fedd_lib, name, dim):
    m = fedd_lib.read_mesh(os.path.join(GOLD, name), dim)
    faces = fedd_lib.boundary_faces(dim, m["conn"], m["xyz"].shape[0])
    assert (np.diff(faces, axis=1) > 0).all()                 # ascending vertex ids
    assert len(face_set(faces)) == faces.shape[0] == m["surf"].shape[0]
    assert face_set(faces) == face_set(m["surf"])


def side_of(xyz_face):
    """(direction, 0 | 1) of the unit-cube side all rows of xyz_face lie on"""
    hits = [(d, v) for d in range(xyz_face.shape[1]) for v in (0, 1) if (np.abs(xyz_face[:, d] - v) < 1e-12).all()]
    assert len(hits) == 1, xyz_face
    return hits[0]


@pytest.mark.parametrize("dim,M,count", [(3, 3, 6 * 2 * 9), (2, 5, 4 * 5)])
def test_structured_surfaces_one_block(fedd_lib, dim, M, count):
    m = fedd_lib.structured_mesh(dim, 1, M)
    faces = fedd_lib.boundary_faces(dim, m["conn"], m["xyz"].shape[0])
    assert faces.shape[0] == count
    surf, sflag = fedd_lib.structured_surfaces(dim, 1, M)
    assert face_set(surf) == face_set(faces) and surf.shape[0] == count
    per_flag = {f: int((sflag == f).sum()) for f in np.unique(sflag)}
    per_side = count // (2 * dim)
    assert per_flag == {1: (2 * dim - 2) * per_side, 2: per_side, 3: per_side}
    for s, f in zip(surf, sflag):
        d, v = side_of(m["xyz"][s])
        assert f == (1 if d > 0 else (3 if v else 2))
    # ... which is the flag of the nodes strictly inside that side
    for i, x in enumerate(m["xyz"]):
        on = [(d, v) for d in range(dim) for v in (0, 1) if abs(x[d] - v) < 1e-12]
        if len(on) == 1:
            assert m["flag_rep"][i] == (1 if on[0][0] > 0 else (3 if on[0][1] else 2))
    surf0, sflag0 = fedd_lib.structured_surfaces(dim, 1, M, flags_option=0)
    assert (surf0 == surf).all() and (sflag0 == 1).all()


@pytest.mark.parametrize("dim,dec,cells,layers", [(3, (2, 1, 1), [2, 4, 4], 1), (3, (2, 1, 1), [2, 4, 4], 4),
                                                  (2, (2, 2), [3, 3], 1), (3, (1, 2, 2), [3, 2, 2], 2)])
def test_structured_surfaces_of_rank_meshes(fedd_lib, dim, dec, cells, layers):
    """every rank lists exactly the faces of its local mesh (ghost elements included) that lie on the global boundary, with the
    flags of the one-block mesh"""
    glob = fedd_lib.structured_mesh(dim, [1] * dim, [d * c for d, c in zip(dec, cells)])
    gs, gf = fedd_lib.structured_surfaces(dim, [1] * dim, [d * c for d, c in zip(dec, cells)])
    gflag = {tuple(sorted(glob["gid_rep"][s])): f for s, f in zip(gs, gf)}
    for rank in range(int(np.prod(dec))):
        m = fedd_lib.structured_mesh(dim, dec, cells, rank, ghosts=layers)
        surf, sflag = fedd_lib.structured_surfaces(dim, dec, cells, rank, ghosts=layers)
        assert (np.diff(surf, axis=1) > 0).all()
        local_faces = face_set(m["gid_rep"][fedd_lib.boundary_faces(dim, m["conn"], m["xyz"].shape[0])])
        expect = {k for k in local_faces if k in gflag}
        got = {tuple(sorted(m["gid_rep"][s])): f for s, f in zip(surf, sflag)}
        assert len(got) == surf.shape[0] and set(got) == expect
        assert all(gflag[k] == f for k, f in got.items())


@pytest.mark.parametrize("name,dim", [("square.mesh", 2), ("DFG3DCylinder_1k.mesh", 3)])
def test_p2_surface_mid_nodes(fedd_lib, name, dim):
    m = fedd_lib.read_mesh(os.path.join(GOLD, name), dim)
    m2 = fedd_lib.p2_of_p1(m, volume_id=0)
    s2 = fedd_lib.p2_surfaces(m)
    assert (s2[:, :dim] == m["surf"]).all() and (s2[:, dim:] >= m["xyz"].shape[0]).all()
    pairs = [(0, 1)] if dim == 2 else [(0, 1), (1, 2), (0, 2)]
    for k, (a, b) in enumerate(pairs):
        mid = 0.5 * (m2["xyz"][s2[:, a]] + m2["xyz"][s2[:, b]])
        assert np.abs(m2["xyz"][s2[:, dim + k]] - mid).max() <= 1e-15
    # the mid nodes are nodes of an element that holds the surface element
    elems = [set(e) for e in m2["conn"]]
    for s in s2[:: max(1, s2.shape[0] // 25)]:
        assert any(set(s) <= e for e in elems)

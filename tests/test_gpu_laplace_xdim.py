"""fedd_assemble(FEDD_FORM_LAPLACE_XDIM) on the GPU against the numpy restatement of FE::assemblyLaplaceXDim
(tests/interface_ref.py): parity to 1e-10 of a row's largest magnitude (the project's bar), the element coefficients bit for
bit, exact linearity in a power-of-two coefficient, reduction to the vector Laplacian, reproducibility, the moved mesh, and a
solve on the assembled matrix.

Four distorted meshes (seeded jitter of the interior nodes; the P2 mid nodes stay on their straight edges), the smallest with
more than one element per node and more than one workgroup's worth of elements per wave trip:
  2D P1 / P2: 4 x 4 cells, 3D P1 / P2: 3 x 3 x 3 and 2 x 2 x 2 cells.
The interface is the side x = 0 (flag 2); distance 0.4 scales some but not all elements, which the tests assert."""
import numpy as np
import pytest
import scipy.sparse as sp

import interface_ref as ir
import stress_ref as sr

pytestmark = pytest.mark.gpu

RTOL = 1e-10
CASES = {"tri_p1": (2, "p1", 4), "tri_p2": (2, "p2", 4), "tet_p1": (3, "p1", 3), "tet_p2": (3, "p2", 2)}
DIST, COEF = 0.4, 37.5
_meshes, _ref = {}, {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mesh(lib, case):
    if case not in _meshes:
        dim, fe, M = CASES[case]
        m = sr.jitter(lib.structured_mesh(dim, 1, M), amplitude=0.2, seed=23)
        _meshes[case] = lib.p2_of_p1(m, volume_id=0) if fe == "p2" else m
    return _meshes[case]


def reference(lib, case):
    """(distances, coefficients, matrix) of the restatement, computed once per mesh"""
    if case not in _ref:
        m = mesh(lib, case)
        d = ir.distances_to_flags(m, 2)
        f = ir.coefficients(m, d, DIST, COEF)
        assert 0 < np.count_nonzero(f == COEF) < f.shape[0]
        _ref[case] = (d, f, ir.assemble(m, f))
    return _ref[case]


def csr_global(ctx, n):
    rowptr, col, val, gid = ctx.csr_get()
    nr = rowptr.shape[0] - 1
    rows = np.repeat(np.arange(nr), np.diff(rowptr))
    A = sp.csr_matrix((val, (gid[:nr][rows], gid[col])), shape=(n, n))
    A.sort_indices()
    return A


def row_error(A, B):
    A = A.tocsr(); B = B.tocsr()
    A.sort_indices(); B.sort_indices()
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    scale = np.maximum(np.abs(B).max(axis=1).toarray().ravel(), 1e-3 * abs(B).max())
    return float((np.abs(A.data - B.data) / scale[np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))]).max())


def values(ctx):
    return ctx.csr_get()[2].copy()


@pytest.fixture(scope="module")
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def prepare(lib, ctx, case, with_distances=True):
    m = mesh(lib, case)
    ctx.mesh_set_dict(m)
    ctx.pattern_build(m["dim"], lib.BLOCK_DIAG)
    if with_distances:
        ctx.interface_distance([2])
    return m


@pytest.mark.parametrize("case", list(CASES))
def test_parity_coefficients_symmetry_and_reproducibility(fedd_lib, ctx, case):
    m = prepare(fedd_lib, ctx, case)
    d, f, K = reference(fedd_lib, case)
    assert np.array_equal(bits(ctx.interface_distances()), bits(d))
    ctx.assemble(fedd_lib.FORM_LAPLACE_XDIM, [DIST, COEF])
    assert np.array_equal(bits(ctx.laplace_scale()), bits(f))
    A = csr_global(ctx, K.shape[0])
    err = row_error(A, K)
    print("%s: largest error relative to the row maximum %.3e" % (case, err))
    assert err <= RTOL
    assert abs(A - A.T).max() <= 1e-13 * abs(A).max()
    v1 = values(ctx)
    ctx.assemble(fedd_lib.FORM_LAPLACE_XDIM, [DIST, COEF])
    assert np.array_equal(bits(values(ctx)), bits(v1))             # two calls agree bit for bit


@pytest.mark.parametrize("case", list(CASES))
def test_exact_linearity_and_reduction_to_the_vector_laplacian(fedd_lib, ctx, case):
    m = prepare(fedd_lib, ctx, case)
    ctx.assemble(fedd_lib.FORM_LAPLACE_XDIM, [2000.0, 1024.0])      # every mean is at most 1000 < 2000: every element scaled
    assert np.all(ctx.laplace_scale() == 1024.0)
    big = values(ctx)
    ctx.assemble(fedd_lib.FORM_LAPLACE_XDIM, [0.0, 1024.0])         # no mean is below 0: f = 1 everywhere
    assert np.all(ctx.laplace_scale() == 1.0)
    one = values(ctx)
    assert np.array_equal(bits(big), bits(1024.0 * one))            # a power of two scales every product and sum exactly
    A1 = csr_global(ctx, m["dim"] * m["n_global"])
    ctx.set_option("asm_zero_eps", 0.0)
    ctx.assemble(fedd_lib.FORM_LAPLACE_VEC)
    L = csr_global(ctx, m["dim"] * m["n_global"])
    err = row_error(A1, L)
    print("%s: f = 1 against FORM_LAPLACE_VEC %.3e" % (case, err))
    assert err <= RTOL


def test_mean_equal_distance_is_not_scaled_and_mid_edge_nodes_do_not_enter(fedd_lib, ctx):
    m = prepare(fedd_lib, ctx, "tri_p2", with_distances=False)
    n, dim = m["xyz"].shape[0], 2
    vertex = np.zeros(n, dtype=bool)
    vertex[np.unique(m["conn"][:, :dim + 1])] = True
    # every vertex 0.75, so every mean is (0.75 + 0.75 + 0.75) / 3.0 = 0.75 exactly; the mid-edge nodes alone are close
    dist = np.where(vertex, 0.75, 1e-6)
    e0 = m["conn"][0, :dim + 1]
    dist[e0] = [0.5, 0.5, 0.5]                                       # ... but element 0 (and what shares its vertices) lies below
    ctx.interface_distance_set(dist)
    ctx.assemble(fedd_lib.FORM_LAPLACE_XDIM, [0.75, 9.0])
    f = ctx.laplace_scale()
    ref = ir.coefficients(m, dist, 0.75, 9.0)
    assert np.array_equal(bits(f), bits(ref))
    means = ir.element_means(m, dist)
    at = means == 0.75
    assert at.any() and np.all(f[at] == 1.0)                        # strict <
    assert f[0] == 9.0 and 0 < np.count_nonzero(f == 9.0) < f.shape[0]
    assert row_error(csr_global(ctx, dim * m["n_global"]), ir.assemble(m, ref)) <= RTOL
    # the same in 3D: (0.75 * 4) / 4.0
    m3 = prepare(fedd_lib, ctx, "tet_p2", with_distances=False)
    v3 = np.zeros(m3["xyz"].shape[0], dtype=bool)
    v3[np.unique(m3["conn"][:, :4])] = True
    d3 = np.where(v3, 0.75, 1e-6)
    ctx.interface_distance_set(d3)
    ctx.assemble(fedd_lib.FORM_LAPLACE_XDIM, [0.75, 9.0])
    assert np.all(ctx.laplace_scale() == 1.0)
    ctx.assemble(fedd_lib.FORM_LAPLACE_XDIM, [np.nextafter(0.75, 1.0), 9.0])
    assert np.all(ctx.laplace_scale() == 9.0)


@pytest.mark.parametrize("case", ["tet_p1", "tri_p2"])
def test_moved_context_with_kept_distances_is_a_fresh_context_on_the_moved_coordinates(fedd_lib, ctx, case):
    m = prepare(fedd_lib, ctx, case)
    x = m["xyz"]
    dim = m["dim"]
    bubble = np.prod(np.sin(np.pi * x), axis=1)
    disp = 0.05 / CASES[case][2] * np.stack([bubble * np.cos(2.1 * x[:, (k + 1) % dim] + 0.7 * k) for k in range(dim)], axis=1)
    d0 = ctx.interface_distances()
    ctx.mesh_move(disp)
    ctx.pattern_build(dim, fedd_lib.BLOCK_DIAG)
    ctx.assemble(fedd_lib.FORM_LAPLACE_XDIM, [DIST, COEF])
    moved, f_moved = values(ctx), ctx.laplace_scale()
    fresh = fedd_lib.Context(device=0)
    try:
        m2 = dict(m)
        m2["xyz"] = x + disp                            # the single addition of Mesh::moveMesh
        fresh.mesh_set_dict(m2)
        fresh.pattern_build(dim, fedd_lib.BLOCK_DIAG)
        fresh.interface_distance_set(d0)
        fresh.assemble(fedd_lib.FORM_LAPLACE_XDIM, [DIST, COEF])
        assert np.array_equal(bits(f_moved), bits(fresh.laplace_scale()))
        assert np.array_equal(bits(moved), bits(values(fresh)))
    finally:
        fresh.close()
    assert np.array_equal(bits(f_moved), bits(reference(fedd_lib, case)[1]))    # the coefficients did not move with the mesh


def test_extension_problem_solves_to_the_solver_tolerance(fedd_lib, ctx):
    """Dirichlet rows, Schwarz setup and GMRES on the scaled matrix: the interface (flag 2) is displaced, the rest of the boundary
    held.  Right-preconditioned GMRES minimises the true residual, so the residual recomputed on the host from the read-back matrix
    is the reported one up to rounding: it is held to 10 x rtol."""
    m = prepare(fedd_lib, ctx, "tet_p1")
    dim = 3
    ctx.assemble(fedd_lib.FORM_LAPLACE_XDIM, [DIST, COEF])
    ctx.assemble_rhs([0.0, 0.0, 0.0])
    ctx.dirichlet([1, 2, 3], [0.0, 0.0, 0.0, 0.02, 0.01, -0.01, 0.0, 0.0, 0.0])
    ctx.schwarz_set_target(27, 1.0)
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    rtol = 1e-9
    x, its, rel = ctx.gmres(None, rtol=rtol, max_it=300, restart=100, use_prec=True)
    assert rel <= rtol and 0 < its < 300
    rowptr, col, val, gid = ctx.csr_get()
    A = sp.csr_matrix((val, col, rowptr))
    b = ctx.rhs_get()
    assert np.linalg.norm(A @ x - b) <= 10.0 * rtol * np.linalg.norm(b)
    # the interface moved by what was prescribed, the held boundary not at all
    flag = np.asarray(m["flag_uni"])
    X = x.reshape(-1, dim)
    # (a unit row holds |x_i - g_i| = |r_i|, so the residual bound above bounds these too)
    bound = 10.0 * rtol * np.linalg.norm(b)
    assert np.abs(X[flag == 2] - np.array([0.02, 0.01, -0.01])).max() <= bound
    assert np.abs(X[(flag == 1) | (flag == 3)]).max() <= bound
    assert np.abs(X[flag == 0]).max() > 0.0


def test_errors(fedd_lib):
    c = fedd_lib.Context(device=0)
    try:
        m = mesh(fedd_lib, "tri_p1")
        c.mesh_set_dict(m)
        c.pattern_build(2, fedd_lib.BLOCK_DIAG)
        with pytest.raises(fedd_lib.FeddError, match="fedd_interface_distance"):
            c.assemble(fedd_lib.FORM_LAPLACE_XDIM, [DIST, COEF])
        with pytest.raises(fedd_lib.FeddError, match="no fedd_assemble"):
            c.laplace_scale()
        c.interface_distance([2])
        with pytest.raises(fedd_lib.FeddError, match="distance, coefficient"):
            c.assemble(fedd_lib.FORM_LAPLACE_XDIM, None)
        c.pattern_build(2, fedd_lib.BLOCK_FULL)
        with pytest.raises(fedd_lib.FeddError, match="DIAG pattern"):
            c.assemble(fedd_lib.FORM_LAPLACE_XDIM, [DIST, COEF])
        c.pattern_build(1, fedd_lib.BLOCK_SCALAR)
        with pytest.raises(fedd_lib.FeddError, match="DIAG pattern"):
            c.assemble(fedd_lib.FORM_LAPLACE_XDIM, [DIST, COEF])
        assert c.interface_distance_info()["have"]      # the refused calls dropped nothing
    finally:
        c.close()
    two = fedd_lib.Context(device=0, rank=0, nranks=2)
    try:
        two.mesh_set_dict(mesh(fedd_lib, "tri_p1"))
        with pytest.raises(fedd_lib.FeddError, match="one rank"):
            two.assemble(fedd_lib.FORM_LAPLACE_XDIM, [DIST, COEF])
    finally:
        two.close()

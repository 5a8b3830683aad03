"""Structured P2 lattices (fedd_mesh_structured_p2_build) through the device layer at the ABI level: the P2 forms and a solve
against the oracle on the same mesh, Stokes and Navier-Stokes on the vertices-first numbering (pressure dof k = P1 lattice node
k), and the lattice memoisation of the SpMV and of the Schwarz setup on P2 rows, which are several times longer than P1 rows."""
import numpy as np
import pytest
import scipy.sparse as sp

import fedd_oracle as fo
from test_gpu_navier_stokes import NavierStokesABI
from test_gpu_parity import assert_matrix_close, csr_global, oracle_mesh
from test_navier_stokes_abi import Restatement

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def device_numbering(m):
    """the one-rank mesh dict with local = global ids: what the merged-system calls index by"""
    n = m["xyz"].shape[0]
    assert m["gid_uni"].shape[0] == n
    return dict(m, gid_rep=np.arange(n, dtype=np.int64), gid_uni=np.arange(n, dtype=np.int64), flag_uni=m["flag_rep"].copy())


def stokes_meshes(lib, dim, M):
    mv = lib.structured_mesh_p2(dim, 1, M, vertices_first=True)
    # one rank: the unique flags in the new order are the repeated ones
    np.testing.assert_array_equal(mv["flag_uni"], mv["flag_rep"])
    m1 = lib.structured_mesh(dim, 1, M)
    assert mv["n_p1"] == m1["xyz"].shape[0] and mv["xyz"][:mv["n_p1"]].tobytes() == m1["xyz"].tobytes()
    return m1, device_numbering(mv)


def stokes_bc(mv, profile=lambda y: 4.0 * y * (1.0 - y)):
    """the reference's structured Stokes test (feddlib/problems/tests/stokes/main.cpp): no-slip on flag 1, inflow on flag 2 --
    4 y (1 - y) in 2D, 16 y (1 - y) z (1 - z) in 3D --, flag 3 natural"""
    dim, X, flag = mv["dim"], mv["xyz"], mv["flag_uni"]
    nodes = np.nonzero(np.isin(flag, (1, 2)))[0]
    vals = np.zeros((nodes.shape[0], dim))
    infl = flag[nodes] == 2
    y = X[nodes, 1]
    prof = profile(y)
    if dim == 3:
        prof = prof * profile(X[nodes, 2])
    vals[infl, 0] = prof[infl]
    rows = (dim * nodes[:, None] + np.arange(dim)[None, :]).ravel()
    return nodes, vals, rows


@pytest.mark.parametrize("dim,M", [(2, 4), (3, 3)])
def test_p2_forms_and_solve_match_the_oracle(fedd_lib, ctx, dim, M):
    m = fedd_lib.structured_mesh_p2(dim, 1, M)
    om = oracle_mesh(m)
    n = om.n_global
    ctx.mesh_set_dict(m)
    nnz = ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    ctx.assemble(fedd_lib.FORM_LAPLACE)
    K = fo.assembly_laplace(om)
    assert nnz == K.nnz
    assert_matrix_close(csr_global(ctx, n)[0], K)
    ctx.assemble(fedd_lib.FORM_MASS)
    assert_matrix_close(csr_global(ctx, n)[0], fo.assembly_mass(om, "Scalar"))
    ctx.pattern_build(dim, fedd_lib.BLOCK_DIAG)
    ctx.assemble(fedd_lib.FORM_LAPLACE_VEC)
    assert_matrix_close(csr_global(ctx, dim * n)[0], fo.assembly_laplace_vecfield(om))
    mu, nu = 2.0e6, 0.4
    E = mu * 2.0 * (1.0 + nu)
    lam = nu * E / ((1.0 + nu) * (1.0 - 2.0 * nu))
    ctx.pattern_build(dim, fedd_lib.BLOCK_FULL)
    ctx.assemble(fedd_lib.FORM_LINELAS, [lam, mu])
    assert_matrix_close(csr_global(ctx, dim * n)[0], fo.assembly_linelas(om, lam, mu))
    # the Laplace problem of the reference's laplace test: f = 1, zero Dirichlet values on flags 1, 2, 3
    ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    ctx.assemble(fedd_lib.FORM_LAPLACE)
    ctx.assemble_rhs([1.0])
    ctx.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    A_bc, rhs_bc, _, _, _ = fo.laplace_problem(om, bc_flags=(1, 2, 3))
    assert_matrix_close(csr_global(ctx, n)[0], A_bc)
    ctx.schwarz_set_target(8, 1.0)
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    x, its, rel = ctx.gmres(None, rtol=1e-13, max_it=500, restart=200, use_prec=True)
    xd = fo.direct_solve(A_bc, rhs_bc)
    print("P2 Laplace %dD M=%d: %d iterations, relres %.2e" % (dim, M, its, rel))
    np.testing.assert_allclose(x, xd, rtol=0, atol=1e-10 * np.abs(xd).max())


@pytest.mark.parametrize("dim,M", [(2, 4), (3, 2)])
def test_stokes_on_the_vertices_first_lattice(fedd_lib, dim, M):
    """A, B, B^T and the merged system against the oracle's blocks; monolithic Schwarz + GMRES, and GMRES with the Triangular
    block preconditioner, against a sparse direct solve of the merged system."""
    lib = fedd_lib
    m1, mv = stokes_meshes(lib, dim, M)
    omv, omp = oracle_mesh(mv), oracle_mesh(m1)
    n_p, nv = m1["xyz"].shape[0], mv["xyz"].shape[0]
    nA, n = dim * nv, dim * nv + n_p
    nodes, vals, rows = stokes_bc(mv)
    p, v, s = lib.Context(device=0), lib.Context(device=0), lib.Context(device=0)
    try:
        p.mesh_set_dict(mv)
        p.pattern_build(dim, lib.BLOCK_DIAG)
        p.assemble(lib.FORM_LAPLACE_VEC)
        p.matrix_store(0)
        p.assemble_div(n_p, 1, 2)
        p.matrix_scale(1, -1.0)
        p.matrix_scale(2, -1.0)
        Ao, BTo, Bo = fo.stokes_blocks(omv, omp, 1.0)
        assert_matrix_close(p.matrix_get(0), Ao)
        assert_matrix_close(p.matrix_get(1), Bo)
        assert_matrix_close(p.matrix_get(2), BTo)
        p.block_merge(0, 2, 1, -1)
        Mo = fo.block_merge(Ao, BTo, Bo)
        rowptr, col, val, gid = p.csr_get()
        assert rowptr.shape[0] - 1 == n
        assert_matrix_close(sp.csr_matrix((val, col, rowptr), shape=(n, n)), Mo)
        p.rhs_set(np.zeros(n))
        p.dirichlet_rows(rows, vals.ravel())
        is_dir = np.zeros(n, dtype=bool)
        is_dir[rows] = True
        g = np.zeros(n)
        g[rows] = vals.ravel()
        M_bc, rhs_bc = fo.set_dirichlet(Mo, np.zeros(n), is_dir, g)
        rowptr, col, val, gid = p.csr_get()
        assert_matrix_close(sp.csr_matrix((val, col, rowptr), shape=(n, n)), M_bc)
        xd = fo.direct_solve(M_bc, rhs_bc)
        assert np.abs(xd[:nA]).max() > 0.5        # the inflow drives a flow
        p.schwarz_setup(overlap=1, combine=lib.COMBINE_RESTRICTED)
        x, its, rel = p.gmres(None, rtol=1e-12, max_it=1500, restart=300, use_prec=True)
        print("Stokes %dD M=%d, monolithic Schwarz: %d iterations, relres %.2e, error %.2e"
              % (dim, M, its, rel, np.abs(x - xd).max() / np.abs(xd).max()))
        assert rel <= 1e-12
        np.testing.assert_allclose(x, xd, rtol=0, atol=1e-10 * np.abs(xd).max())
        # Triangular block preconditioner: velocity child on block (0,0) with the Dirichlet rows, Schur child on M_p
        v.mesh_set_dict(mv)
        v.matrix_import(p, 0)
        v.dirichlet_nodes(nodes, vals)
        v.schwarz_setup(1 if dim == 2 else 0, lib.COMBINE_RESTRICTED)
        s.mesh_set_dict(m1)
        s.pattern_build(1, lib.BLOCK_SCALAR)
        s.assemble(lib.FORM_MASS)
        s.schwarz_setup(1, lib.COMBINE_RESTRICTED)
        p.block_prec_attach(lib.BLOCKPREC_TRIANGULAR, v, s, -1.0, 2)
        try:
            x, its, rel = p.gmres(None, rtol=1e-12, max_it=1500, restart=300, use_prec=True)
        finally:
            p.block_prec_detach()
        print("Stokes %dD M=%d, Triangular: %d iterations, relres %.2e, error %.2e"
              % (dim, M, its, rel, np.abs(x - xd).max() / np.abs(xd).max()))
        assert rel <= 1e-12
        np.testing.assert_allclose(x, xd, rtol=0, atol=1e-10 * np.abs(xd).max())
    finally:
        for c in (p, v, s):
            c.close()


def check_spmv_report(info, n_rows, nnz):
    """fedd_spmv_patterns / fedd_spmv_classes / fedd_spmv_col_bytes against fedd_spmv_info and each other"""
    assert info["nnz_pattern"] == nnz and 0 < info["nnz_streamed"] <= nnz, info
    assert (info["column_patterns"] >= 1) == (info["column_index_bytes"] == 0), info
    if info["column_patterns"] == 0:
        assert info["rows_with_explicit_columns"] == n_rows and info["column_index_bytes"] in (2, 4), info
    else:
        assert 0 <= info["rows_with_explicit_columns"] <= n_rows, info
    if info["row_classes"] == 0:
        assert info["rows_in_classes"] == 0 and info["nnz_streamed_outside_classes"] == info["nnz_streamed"], info
    else:
        assert 0 < info["rows_in_classes"] <= n_rows and 0 <= info["nnz_streamed_outside_classes"] <= info["nnz_streamed"], info


def test_spmv_memoisation_on_a_p2_lattice(fedd_lib, ctx):
    """41^3 = 68 921 rows, just over the 65 536-row gate of the row classes.  What the class and pattern stages find on P2 rows
    is printed, not asserted (declining them is a valid outcome); every stream gives the bits of the per-entry kernel, and at
    drop tolerance 0 the bits of the parity CSR."""
    m = fedd_lib.structured_mesh_p2(3, 1, 20)
    assert m["xyz"].shape[0] == 41 ** 3 > 65536
    ctx.mesh_set_dict(m)
    ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    ctx.assemble(fedd_lib.FORM_LAPLACE)
    ctx.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    n, _, nnz = ctx.csr_sizes()
    x = np.random.default_rng(41).standard_normal(n)
    y_public = ctx.spmv(x)                          # the parity CSR
    try:
        ctx.set_option("spmv_exact_public", 0)      # fedd_spmv = the solver's stream from here on
        ctx.set_option("spmv_classes", 0)
        ctx.set_option("spmv_pattern", 0)
        ctx.set_option("spmv_nt", 0)
        y0 = ctx.spmv(x)
        check_spmv_report(ctx.spmv_info(), n, nnz)
        for classes, pattern in ((1, 1), (1, 2), (0, 2)):
            ctx.set_option("spmv_classes", classes)
            ctx.set_option("spmv_pattern", pattern)
            y = ctx.spmv(x)
            info = ctx.spmv_info()
            print("P2 lattice, spmv_classes %d spmv_pattern %d: %s" % (classes, pattern, info))
            if info["row_classes"] == 0 and info["column_patterns"] == 0:
                print("  the class and pattern stages declined the P2 rows: the window kernel ran")
            check_spmv_report(info, n, nnz)
            assert np.array_equal(y, y0), (classes, pattern)
        ctx.set_option("spmv_drop_tol", 0.0)        # the same entries as the parity CSR but its exact zeros
        for classes, pattern in ((0, 0), (1, 1), (1, 2)):
            ctx.set_option("spmv_classes", classes)
            ctx.set_option("spmv_pattern", pattern)
            assert np.array_equal(ctx.spmv(x), y_public), (classes, pattern)
            check_spmv_report(ctx.spmv_info(), n, nnz)
    finally:
        ctx.set_option("spmv_drop_tol", 2.0 ** -52)
        for key, val in (("spmv_nt", -1), ("spmv_pattern", 1), ("spmv_classes", 1), ("spmv_exact_public", 1)):
            ctx.set_option(key, val)


def test_schwarz_on_a_p2_lattice(fedd_lib, ctx):
    """13^3 nodes: subdomains with the same local matrix share an inverse; the apply against the oracle's restricted additive
    Schwarz on the same bins"""
    m = fedd_lib.structured_mesh_p2(3, 1, 6)
    om = oracle_mesh(m)
    ctx.mesh_set_dict(m)
    ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    ctx.assemble(fedd_lib.FORM_LAPLACE)
    ctx.assemble_rhs([1.0])
    ctx.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    A_bc, rhs_bc, _, _, _ = fo.laplace_problem(om, bc_flags=(1, 2, 3))
    ctx.schwarz_set_target(8, 1.0)
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    info = ctx.schwarz_info()
    node_bin, nb, _ = fo.schwarz_bins(m["xyz"], 8)
    ras = fo.RAS(A_bc, node_bin, nb)
    print("P2 lattice 13^3: %s" % info)
    assert info["n_subdomains"] == nb and info["max_size"] == ras.max_size
    assert 1 <= info["n_unique"] <= info["n_subdomains"]
    r = np.random.default_rng(13).standard_normal(A_bc.shape[0])
    z, zo = ctx.schwarz_apply(r), ras.apply(r)
    np.testing.assert_allclose(z, zo, rtol=0, atol=1e-10 * np.abs(zo).max())


def test_navier_stokes_iterations_on_the_vertices_first_lattice(fedd_lib, ctx):
    """2D M=4: one fixed-point and one Newton iteration; before each the advection blocks at the current iterate against the
    restatement, and each update against a sparse direct solve of the system the device holds.  The inflow is sin(pi y): with
    the parabola, Poiseuille flow solves the problem after one step and the Newton step would have nothing to do."""
    lib = fedd_lib
    m1, mv = stokes_meshes(lib, 2, 4)
    nodes, vals, rows = stokes_bc(mv, profile=lambda y: np.sin(np.pi * y))
    nu, rho = 0.05, 1.0
    ns = NavierStokesABI(lib, ctx, m1, mv, nu, rho, rows, vals.ravel())
    R = Restatement(lib, mv)
    x = np.zeros(ns.n)
    x[rows] = vals.ravel()
    for method in ("FixedPoint", "Newton"):
        u = x[:2 * ns.nv]
        r = ns.residual(x)
        No, Wo = R.N(u), R.W(u)
        ctx.assemble_advection(lib.ADV_N, 1.0, -1, 3)
        assert_matrix_close(ctx.matrix_get(3), No)
        ctx.assemble_advection(lib.ADV_W, 1.0, -1, 3)
        assert_matrix_close(ctx.matrix_get(3), Wo)
        if method == "Newton":
            ns.system(lib.ADV_NEWTON, x)
        b = -r
        b[rows] = 0.0
        ctx.rhs_set(b)
        ctx.dirichlet_rows(rows, -r[rows])
        rowptr, col, val, _ = ctx.csr_get()
        J = sp.csr_matrix((val, col, rowptr), shape=(ns.n, ns.n))
        rhs = ctx.rhs_get()
        dx, its, rel = ctx.gmres(None, rtol=1e-12, max_it=4 * ns.n, restart=min(ns.n, 600), use_prec=False)
        dxd = fo.direct_solve(J, rhs)
        print("%s: %d iterations, relres %.2e, |r| %.3e" % (method, its, rel, np.linalg.norm(r)))
        np.testing.assert_allclose(dx, dxd, rtol=0, atol=1e-10 * np.abs(dxd).max())
        x = x + dx
    print("residual after the Newton step: %.3e" % np.linalg.norm(ns.residual(x)))

"""tests/fsi_ref.py against properties that do not depend on it, on a 2D pair of 2 x 2-cell meshes (fluid on [0,1]^2, structure
shifted by +1 in x, the interface x = 1 flagged 7 on both sides).

The children's matrices are not finite-element matrices: the FaCSI identities below are algebraic, they hold for any invertible
children on the mesh graph.  Fluid [F B^T; B C]: F = (graph Laplacian + I) x I_2 on the nodes, B a fixed sparse block, C = -I/2;
structure S = 2 (graph Laplacian + I) x I_2 with unit rows on its far side.  No fluid Dirichlet row lies on the interface (there
the row has no C1^T entry and the identity is not expected)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import fsi_ref

FLAG, DT, DIM = 7, 0.125, 2


def graph_laplacian(conn, n):
    i = np.repeat(conn, conn.shape[1], axis=1).ravel()
    j = np.tile(conn, (1, conn.shape[1])).ravel()
    G = sp.csr_matrix((np.ones(i.shape[0]), (i, j)), shape=(n, n))
    G.data[:] = 1.0
    G = G - sp.diags(G.diagonal())
    return (sp.diags(np.asarray(G.sum(axis=1)).ravel()) - G).tocsr()


def csr_arrays(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.copy()


def build(fedd_lib, mask=None):
    mf = fedd_lib.structured_mesh(2, 1, 2)
    ms = fedd_lib.structured_mesh(2, 1, 2)
    xf, xs = fsi_ref.unique_coords(mf), fsi_ref.unique_coords(ms)
    xs[:, 0] += 1.0
    ff, fs = mf["flag_uni"].copy(), ms["flag_uni"].copy()
    ff[np.abs(xf[:, 0] - 1.0) < 1e-12] = FLAG
    fs[np.abs(xs[:, 0] - 1.0) < 1e-12] = FLAG
    xf[ff == FLAG, 0] = 1.0
    xs[fs == FLAG, 0] = 1.0
    n = xf.shape[0]
    pos = {int(g): i for i, g in enumerate(mf["gid_uni"])}
    conn = np.vectorize(lambda r: pos[int(mf["gid_rep"][r])])(mf["conn"])
    L = graph_laplacian(conn, n)
    I2 = sp.identity(DIM)
    Fv = sp.kron(L + sp.identity(n), I2).tocsr()
    n_u, n_p = DIM * n, n
    rng = np.random.default_rng(3)
    B = sp.kron(L, sp.csr_matrix(np.array([[0.5, -0.25]]))).tocsr()
    B.data *= rng.uniform(0.5, 1.5, B.data.shape[0])
    M = sp.bmat([[Fv, B.T], [B, -0.5 * sp.identity(n_p)]]).tolil()
    dir_f = np.zeros(n_u + n_p, dtype=bool)
    inflow = np.nonzero(xf[:, 0] < 1e-12)[0]
    dir_f[(DIM * inflow[:, None] + np.arange(DIM)).ravel()] = True
    for r in np.nonzero(dir_f)[0]:
        M[r, :] = 0.0
        M[r, r] = 1.0
    S = (2.0 * sp.kron(L + sp.identity(n), I2)).tolil()
    dir_s = np.zeros(DIM * n, dtype=bool)
    far = np.nonzero(xs[:, 0] > 2.0 - 1e-12)[0]
    dir_s[(DIM * far[:, None] + np.arange(DIM)).ravel()] = True
    for r in np.nonzero(dir_s)[0]:
        S[r, :] = 0.0
        S[r, r] = 1.0
    i_f, i_s, ptr = fsi_ref.match(xf, ff, xs, fs, [FLAG])
    fdof, sdof = fsi_ref.interface_dofs(i_f, i_s, DIM, mask)
    A = fsi_ref.to_scipy(fsi_ref.coupled_csr(csr_arrays(M), csr_arrays(S), dir_f, dir_s, fdof, sdof, DT))
    return dict(xf=xf, xs=xs, ff=ff, fs=fs, i_f=i_f, i_s=i_s, ptr=ptr, fdof=fdof, sdof=sdof, A=A, M=sp.csr_matrix(M), S=sp.csr_matrix(S),
                n_u=n_u, n_f=n_u + n_p, n_s=DIM * n)


def test_match_equals_pairing_by_coordinate_equality(fedd_lib):
    p = build(fedd_lib)
    assert p["i_f"].shape[0] == 3 and list(p["ptr"]) == [0, 3]
    # independent pairing: every fluid interface node has exactly one structure node at its coordinates
    for a, b in zip(p["i_f"], p["i_s"]):
        same = np.nonzero((p["xs"] == p["xf"][a]).all(axis=1) & (p["fs"] == FLAG))[0]
        assert same.tolist() == [b]
    assert sorted(p["i_f"].tolist()) == np.nonzero(p["ff"] == FLAG)[0].tolist()
    y = p["xf"][p["i_f"], 1]
    assert np.all(np.diff(y) > 0)         # x is 1.0 on all of them: the order is ascending y


def test_coupling_blocks(fedd_lib):
    p = build(fedd_lib)
    A, n_f, n_s = p["A"], p["n_f"], p["n_s"]
    off = n_f + n_s
    n_l = p["fdof"].shape[0]
    C1 = A[off:, :n_f].toarray()
    C2 = A[off:, n_f:off].toarray()
    assert np.array_equal(C1, A[:n_f, off:].toarray().T) and set(np.unique(C1)) == {0.0, 1.0}
    assert np.array_equal(np.nonzero(C1)[1], p["fdof"])
    assert np.array_equal(C2[np.arange(n_l), p["sdof"]], np.full(n_l, -(1.0 / DT))) and np.count_nonzero(C2) == n_l
    C3T = A[n_f:off, off:].toarray()
    assert np.array_equal(np.nonzero(C3T.T)[1], p["sdof"]) and set(np.unique(C3T)) == {0.0, -1.0}
    assert A[off:, off:].nnz == 0 and A[:n_f, n_f:off].nnz == 0 and A[n_f:off, :n_f].nnz == 0


def exact_children(p):
    MD = p["M"].tolil()
    on = p["fdof"] >= 0
    for r in p["fdof"][on]:
        MD[r, :] = 0.0
        MD[r, r] = 1.0
    lu_f, lu_s = spla.splu(sp.csc_matrix(MD)), spla.splu(sp.csc_matrix(p["S"]))
    return lu_f.solve, lu_s.solve


def test_facsi_is_exact_except_for_the_dropped_c3t(fedd_lib):
    p = build(fedd_lib)
    A, n_f, n_s, n_u = p["A"], p["n_f"], p["n_s"], p["n_u"]
    off = n_f + n_s
    af, as_ = exact_children(p)
    x = np.random.default_rng(11).standard_normal(A.shape[0])
    y = fsi_ref.facsi_apply(A, n_u, n_f, n_s, p["fdof"], p["sdof"], DT, x, af, as_)
    r = A @ y - x
    tol = 1e-12 * np.abs(x).max()
    assert np.abs(r[:n_f]).max() <= tol and np.abs(r[off:]).max() <= tol
    c3t = A[n_f:off, off:] @ y[off:]
    assert np.abs(c3t).max() > 1e-3                    # the d block does differ
    assert np.abs(r[n_f:off] - c3t).max() <= tol       # ... by exactly C3^T y_l


def test_uncoupled_dofs(fedd_lib):
    mask = np.ones(6, dtype=np.uint8)
    mask[[1, 4]] = 0
    p = build(fedd_lib, mask)
    A, n_f, n_s, n_u = p["A"], p["n_f"], p["n_s"], p["n_u"]
    off = n_f + n_s
    for k in (1, 4):
        row = A[off + k, :]
        assert row.indices.tolist() == [off + k] and row.data.tolist() == [1.0]
        assert A[:, off + k].nnz == 1
    af, as_ = exact_children(p)
    x = np.random.default_rng(12).standard_normal(A.shape[0])
    y = fsi_ref.facsi_apply(A, n_u, n_f, n_s, p["fdof"], p["sdof"], DT, x, af, as_)
    assert np.array_equal(y[off + np.array([1, 4])], x[off + np.array([1, 4])])
    r = A @ y - x
    assert np.abs(r[:n_f]).max() <= 1e-12 * np.abs(x).max() and np.abs(r[off:]).max() <= 1e-12 * np.abs(x).max()
    d_old = np.arange(n_s, dtype=np.float64) + 1.0
    rhs = fsi_ref.interface_rhs(p["sdof"], d_old, DT)
    assert rhs[1] == 0.0 and rhs[4] == 0.0 and rhs[0] == -(1.0 / DT) * d_old[p["sdof"][0]]

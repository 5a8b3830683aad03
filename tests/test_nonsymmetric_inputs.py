"""Host side of tests/test_gpu_nonsymmetric.py: the velocity block of a BDF step of Navier-Stokes,

    A = cm M + nu L + rho (N + W)(u)        (vector mass, vector Laplacian, the two advection forms; FULL node-block pattern)

with unit Dirichlet rows on the whole boundary, built here from the oracle's M and L and the numpy restatement of N and W
(tests/test_navier_stokes_abi.py).  Nothing of the device runs.  What is asserted is that the GPU tests have power and that
their inputs are safe for the kernels they feed:

  * with S = A whose free-free block is replaced by its symmetric part (what the Laplace, elasticity and Stokes tests can
    already see), the one-level operator of A differs from that of S, and K0^-1 of the Q1 coarse level from its transpose,
    by at least 1e-3 of their size;
  * elimination without row exchanges (what the local-inverse kernels do) meets no pivot below 1e-6 of the matrix scale in
    any local matrix, and only positive pivots in K0 (coarse_setup rejects anything else as "not positive definite").

Parameters nu = 0.05, rho = 1, cm = 2.  Measured here (one and two layers of overlap): operator against S 0.21 ... 1.23 of
max |z| (smooth velocity; 0.14 ... 0.71 constant velocity), K0^-1 against its transpose 0.17 ... 0.25 of max |K0^-1|, smallest
local pivot 3.2e-2 ... 1.8e-1 of the matrix scale, smallest K0 pivot / largest 2.8e-2 ... 1.9e-1."""
import numpy as np
import pytest
import scipy.sparse as sp

import fedd_oracle as fo
from test_gpu_parity import oracle_mesh
from test_navier_stokes_abi import Restatement, smooth_velocity

NU, RHO, CM = 0.05, 1.0, 2.0
NMAX = 256                                  # dofs of the largest subdomain the dense local solver takes
# (dim, M, nodes per box, layers of overlap) of the one-level tests of the GPU file.  With 3 dofs per node the boxes of 40 and of 64
# nodes are both refined to the same lattice (138 dofs with the overlap); (2, 17, 36) and (2, 24, 72) are added for the sizes the
# issue's shapes leave out: 124 dofs, and 238, past the register-tiled inversion classes
RAS_CASES = [(2, 12, 9, 1), (3, 6, 8, 1), (3, 9, 40, 1), (3, 9, 64, 1), (2, 17, 36, 1), (2, 24, 72, 1), (2, 12, 9, 2), (3, 6, 8, 2)]
Q1_CASES = [(2, 12, 9, 9), (3, 6, 8, 8), (3, 10, 27, 27)]             # (dim, M, nodes per box, coarse cells): row e
COMBINES = ("restricted", "averaging", "full")


def velocity(which, xyz):
    """"smooth": every local matrix differs.  "constant": W = 0 and the operator is translation invariant, so a structured
    mesh repeats its local matrices."""
    if which == "smooth":
        return smooth_velocity(xyz)
    return np.tile(np.array([1.0, 0.5, 0.25])[:xyz.shape[1]], (xyz.shape[0], 1))


def _rows(A):
    return np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))


def host_system(fedd_lib, m, which="smooth", nu=NU, rho=RHO, cm=CM):
    """(A with unit Dirichlet rows on flags 1, 2, 3, mask of those rows); structural zeros of the FULL pattern kept"""
    dim = m["dim"]
    om = oracle_mesh(m)
    R = Restatement(fedd_lib, m)
    u = velocity(which, m["xyz"]).ravel()
    parts = [(cm, fo.assembly_mass(om, "Vector").tocsr()), (nu, fo.assembly_laplace_vecfield(om).tocsr()),
             (rho, R.N(u)), (rho, R.W(u))]
    n = dim * m["xyz"].shape[0]
    A = sp.coo_matrix((np.concatenate([s * P.data for s, P in parts]),
                       (np.concatenate([_rows(P) for _, P in parts]), np.concatenate([P.indices for _, P in parts]))),
                      shape=(n, n)).tocsr()                                  # duplicates summed, zeros stay
    A.sort_indices()
    is_dir = fo.dirichlet_rows(m["flag_uni"], (1, 2, 3), dofs=dim)
    A_bc, _ = fo.set_dirichlet(A, np.zeros(n), is_dir, 0.0)
    return A_bc, is_dir


def symmetrised(A, is_dir):
    """A with its free-free block replaced by (A_ff + A_ff^T) / 2; the Dirichlet rows and the columns into them stay"""
    F = sp.diags((~np.asarray(is_dir, dtype=bool)).astype(float))
    Aff = (F @ A @ F).tocsr()
    S = (A - 0.5 * Aff + 0.5 * Aff.T).tocsr()
    S.sort_indices()
    return S


def subdomain_sizes(A, node_bin, nb, dofs, overlap):
    n = A.shape[0]
    G = A.copy()
    G.data = np.ones_like(G.data)
    P = sp.csr_matrix((np.ones(n), (np.arange(n), np.repeat(node_bin, dofs))), shape=(n, nb))
    for _ in range(overlap):
        P = G @ P + P
        P.data[:] = 1.0
    return np.asarray(P.sum(axis=0)).ravel().astype(np.int64)


def lattice_bins(A, xyz, target, dofs, overlap):
    """The boxes of schwarz_setup for `target` nodes per box: fo.schwarz_bins, with the box edge shrunk by 0.85 (at most eight
    times) while an overlapping subdomain exceeds the NMAX dofs of the dense local solver (Schwarz).  Returns
    (node_bin, number of boxes, largest subdomain)."""
    for attempt in range(9):
        node_bin, nb, _ = fo.schwarz_bins(xyz, target, scale=0.85 ** attempt)
        largest = int(subdomain_sizes(A, node_bin, nb, dofs, overlap).max())
        if largest <= NMAX:
            break
    return node_bin, nb, largest


def pivots_without_exchanges(B):
    """the pivots of Gaussian elimination in the given order, no row exchanges"""
    B = np.array(B, dtype=np.float64, copy=True)
    n = B.shape[0]
    piv = np.empty(n)
    for k in range(n):
        piv[k] = B[k, k]
        if piv[k] == 0.0:
            piv[k + 1:] = 0.0
            break
        B[k + 1:, k + 1:] -= np.outer(B[k + 1:, k] / piv[k], B[k, k + 1:])
    return piv


def test_the_system_is_what_it_claims_to_be(fedd_lib):
    """unit rows on the boundary; free-free block nonsymmetric by far more than rounding for both velocities; the constant
    velocity has no W"""
    m = fedd_lib.structured_mesh(3, 1, 6)
    for which in ("smooth", "constant"):
        A, is_dir = host_system(fedd_lib, m, which)
        assert is_dir.sum() == 3 * (7 ** 3 - 5 ** 3)
        D = A[is_dir]
        assert np.array_equal(D.data != 0.0, D.indices == np.nonzero(is_dir)[0][_rows(D)]) and set(D.data) <= {0.0, 1.0}
        Aff = A[~is_dir][:, ~is_dir]
        skew = abs(Aff - Aff.T).max() / abs(Aff).max()
        print("%s velocity: |A_ff - A_ff^T| / |A_ff| = %.3f" % (which, skew))         # measured 0.34 (smooth), 0.19 (constant)
        assert skew > 0.1
    R = Restatement(fedd_lib, m)
    assert np.abs(R.W(velocity("constant", m["xyz"]).ravel()).data).max() <= 1e-14


@pytest.mark.parametrize("which", ["smooth", "constant"])
@pytest.mark.parametrize("dim,M,target,overlap", RAS_CASES)
def test_one_level_operator_tells_the_matrix_from_its_symmetric_part(fedd_lib, dim, M, target, overlap, which):
    m = fedd_lib.structured_mesh(dim, 1, M)
    A, is_dir = host_system(fedd_lib, m, which)
    S = symmetrised(A, is_dir)
    node_bin, nb, largest = lattice_bins(A, m["xyz"], target, dim, overlap)
    assert largest <= NMAX
    ras_a = fo.RAS(A, node_bin, nb, dofs=dim, overlap=overlap)
    ras_s = fo.RAS(S, node_bin, nb, dofs=dim, overlap=overlap)
    # elimination without row exchanges, in the order of the local matrix (owned dofs, then the overlap)
    worst = np.inf
    for idx, _, _ in ras_a.subs:
        Ai = A[idx][:, idx].toarray()
        worst = min(worst, np.abs(pivots_without_exchanges(Ai)).min() / np.abs(Ai).max())
    print("dim %d M %d target %d overlap %d %s: %d boxes, largest %d dofs, smallest pivot / matrix scale %.2e"
          % (dim, M, target, overlap, which, nb, largest, worst))
    assert worst >= 1e-6
    r = np.random.default_rng(3).standard_normal(A.shape[0])
    for combine in COMBINES:
        ras_a.combine = ras_s.combine = combine
        za, zs = ras_a.apply(r), ras_s.apply(r)
        diff = np.abs(za - zs).max() / np.abs(za).max()
        print("    %s: |RAS(A) r - RAS(S) r| / |RAS(A) r| = %.2e" % (combine, diff))
        assert diff >= 1e-3


@pytest.mark.parametrize("dim,M,target,cells", Q1_CASES)
def test_coarse_matrix_is_far_from_its_transpose_and_has_positive_pivots(fedd_lib, dim, M, target, cells):
    m = fedd_lib.structured_mesh(dim, 1, M)
    A, is_dir = host_system(fedd_lib, m, "smooth")
    co = fo.CoarseQ1(A, m["xyz"], is_dir, dim, cells_target=cells)
    diff = np.abs(co.K0inv - co.K0inv.T).max() / np.abs(co.K0inv).max()
    piv = pivots_without_exchanges(co.K0)
    print("dim %d M %d cells %d: n0 %d, |K0^-1 - K0^-T| / |K0^-1| = %.2e, smallest pivot / largest %.2e"
          % (dim, M, cells, co.n0, diff, piv.min() / piv.max()))
    assert diff >= 1e-3
    assert np.all(piv > 0.0)
    # ... and the coarse level as an operator tells A from S as well
    cs = fo.CoarseQ1(symmetrised(A, is_dir), m["xyz"], is_dir, dim, cells_target=cells)
    r = np.random.default_rng(5).standard_normal(A.shape[0])
    za = co.apply(r)
    assert np.abs(za - cs.apply(r)).max() >= 1e-3 * np.abs(za).max()

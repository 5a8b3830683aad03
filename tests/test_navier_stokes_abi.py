"""Advection matrices of steady Navier-Stokes, host side: the new ABI symbols, and a plain numpy restatement of
N(u) (FE::assemblyAdvectionVecField, FE_def.hpp:1759-1832) and W(u) (FE::assemblyAdvectionInUVecField, :1839-1925) written
from their formulas,

    n_ij                 = |det B| sum_q w_q (u_h(x_q) . grad phi_j(x_q)) phi_i(x_q)      on the pairs (dim i + d, dim j + d)
    W(dim i + d1, dim j + d2) = |det B| sum_q w_q (d u_d1 / d x_d2)(x_q) phi_i(x_q) phi_j(x_q)

checked here by identities that need no oracle.  tests/test_gpu_navier_stokes.py compares the device against it."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# P2 mid-side nodes: local node dim + 1 + k sits on edge EDGES[dim][k] (MeshUnstructured_def.hpp:755-772)
EDGES = {2: [(0, 1), (1, 2), (0, 2)], 3: [(0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3)]}


def lagrange_basis(dim, nen, pts):
    """phi [nq, nen] and its reference gradient [nq, nen, dim] from the barycentric coordinates: P1 lambda_i; P2
    lambda_i (2 lambda_i - 1) at the vertices and 4 lambda_a lambda_b on the edges"""
    nq = pts.shape[0]
    lam = np.concatenate([1.0 - pts.sum(axis=1, keepdims=True), pts], axis=1)            # [nq, dim + 1]
    dlam = np.concatenate([-np.ones((1, dim)), np.eye(dim)], axis=0)                       # [dim + 1, dim]
    if nen == dim + 1:
        return lam.copy(), np.broadcast_to(dlam, (nq, dim + 1, dim)).copy()
    phi = np.zeros((nq, nen)); dphi = np.zeros((nq, nen, dim))
    for i in range(dim + 1):
        phi[:, i] = lam[:, i] * (2.0 * lam[:, i] - 1.0)
        dphi[:, i, :] = (4.0 * lam[:, i] - 1.0)[:, None] * dlam[i][None, :]
    for k, (a, b) in enumerate(EDGES[dim]):
        phi[:, dim + 1 + k] = 4.0 * lam[:, a] * lam[:, b]
        dphi[:, dim + 1 + k, :] = 4.0 * (lam[:, a, None] * dlam[b][None, :] + lam[:, b, None] * dlam[a][None, :])
    return phi, dphi


def degrees(dim, nen):
    """determineDegree for the two forms (FE_def.hpp:1770-1772, 1859-1861): (N, W)"""
    return (5, 5) if nen > dim + 1 else (2, 3)


class Restatement:
    def __init__(self, fedd_lib, m):
        self.dim, self.nen = m["dim"], m["conn"].shape[1]
        self.conn = np.asarray(m["conn"], dtype=np.int64)
        self.n_node = m["xyz"].shape[0]
        X = m["xyz"][self.conn[:, :self.dim + 1]]
        B = np.transpose(X[:, 1:, :] - X[:, :1, :], (0, 2, 1))                             # B[e, i, j] = x_{j+1}[i] - x_0[i]
        self.Binv = np.linalg.inv(B)
        self.absdet = np.abs(np.linalg.det(B))
        self.rule = {}
        for deg in set(degrees(self.dim, self.nen)):
            pts, w = fedd_lib.fe_quadrature(self.dim, deg)                                 # the rule's points and weights (data)
            phi, dphi = lagrange_basis(self.dim, self.nen, pts)
            G = np.einsum("qjr,erd->eqjd", dphi, self.Binv)                                # grad phi_j at x_q, physical
            self.rule[deg] = (w, phi, G)

    def _U(self, u):
        return np.asarray(u, dtype=np.float64).reshape(-1, self.dim)[self.conn]            # [e, i, d]

    def blocks_N(self, u, absolute=False):
        """element blocks [e, i, d1, j, d2]; absolute: every product replaced by its magnitude (rounding bounds)"""
        w, phi, G = self.rule[degrees(self.dim, self.nen)[0]]
        U = self._U(u)
        f = np.abs if absolute else (lambda t: t)
        uq = np.einsum("qi,eid->eqd", f(phi), f(U))
        n = np.einsum("e,q,qi,eqd,eqjd->eij", self.absdet, f(w), f(phi), uq, f(G))
        return np.einsum("eij,ab->eiajb", n, np.eye(self.dim))

    def blocks_W(self, u, absolute=False):
        w, phi, G = self.rule[degrees(self.dim, self.nen)[1]]
        U = self._U(u)
        f = np.abs if absolute else (lambda t: t)
        gu = np.einsum("eia,eqib->eqab", f(U), f(G))                                       # d u_a / d x_b at x_q
        return np.einsum("e,q,eqab,qi,qj->eiajb", self.absdet, f(w), gu, f(phi), f(phi))

    def assemble(self, blocks):
        """FULL dim x dim node-block pattern, structural zeros kept"""
        dim, nen, n = self.dim, self.nen, self.dim * self.n_node
        dof = (dim * self.conn[:, :, None] + np.arange(dim)[None, None, :]).reshape(-1, nen * dim)
        rows = np.repeat(dof, nen * dim, axis=1).ravel()
        cols = np.tile(dof, (1, nen * dim)).ravel()
        A = sp.coo_matrix((blocks.reshape(-1), (rows, cols)), shape=(n, n)).tocsr()        # duplicates summed, zeros stay
        A.sort_indices()
        return A

    def N(self, u, **kw):
        return self.assemble(self.blocks_N(u, **kw))

    def W(self, u, **kw):
        return self.assemble(self.blocks_W(u, **kw))

    def mass_vec(self):
        w, phi, _ = self.rule[5]
        mloc = np.einsum("e,q,qi,qj->eij", self.absdet, w, phi, phi)
        return self.assemble(np.einsum("eij,ab->eiajb", mloc, np.eye(self.dim)))


def p2_meshes(fedd_lib):
    sq = fedd_lib.p2_of_p1(fedd_lib.read_mesh(os.path.join(GOLD, "square.mesh"), 2), volume_id=10)
    cy = fedd_lib.p2_of_p1(fedd_lib.read_mesh(os.path.join(GOLD, "DFG3DCylinder_1k.mesh"), 3), volume_id=0)
    return {"square_p2": sq, "cylinder_p2": cy}


def smooth_velocity(x):
    """smooth, not a polynomial, every component depends on every coordinate"""
    s = x.sum(axis=1)
    cols = [np.sin(1.3 * x[:, 0] + 0.4 * s) + 0.5, np.cos(0.9 * x[:, 1] - 0.7 * s) * np.exp(0.3 * x[:, 0])]
    if x.shape[1] == 3:
        cols.append(np.sin(1.1 * x[:, 2]) * np.cos(0.8 * s) - 0.25)
    return np.stack(cols, axis=1)


def test_new_symbols_in_header_library_and_binding(fedd_lib):
    hdr = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    L = ctypes.CDLL(fedd_lib.LIB_PATH)
    for name in ("fedd_velocity_set", "fedd_assemble_advection"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in fedd_lib.SIGNATURES
    for name, value in (("FEDD_ADV_N", fedd_lib.ADV_N), ("FEDD_ADV_W", fedd_lib.ADV_W), ("FEDD_ADV_NEWTON", fedd_lib.ADV_NEWTON)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, hdr).group(1)) == value
    assert hasattr(fedd_lib.Context, "velocity_set") and hasattr(fedd_lib.Context, "assemble_advection")
    # the entries cite the reference lines they replace
    assert "FE_def.hpp:1759-1832" in hdr and "FE_def.hpp:1839-1925" in hdr and "NavierStokes_def.hpp:282-321" in hdr


def test_calls_fail_loudly_without_a_device(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        with pytest.raises(fedd_lib.FeddError):
            c.velocity_set(np.zeros(6))
        with pytest.raises(fedd_lib.FeddError):
            c.assemble_advection(fedd_lib.ADV_NEWTON, 1.0, -1, 4)
    finally:
        c.close()


@pytest.mark.parametrize("which", ["square_p2", "cylinder_p2"])
def test_restatement_identities(fedd_lib, which):
    m = p2_meshes(fedd_lib)[which]
    dim, x = m["dim"], m["xyz"]
    R = Restatement(fedd_lib, m)
    u = smooth_velocity(x).ravel()
    N, W = R.N(u), R.W(u)
    scale = np.abs(N).max()
    # the pattern is the FULL node-block pattern; N fills the diagonal pairs only
    assert N.nnz == W.nnz and np.array_equal(N.indptr, W.indptr) and np.array_equal(N.indices, W.indices)
    rows = np.repeat(np.arange(N.shape[0]), np.diff(N.indptr))
    assert np.all(N.data[(rows % dim) != (N.indices % dim)] == 0.0)
    # sum_j grad phi_j = 0: the row sums of n_ij vanish
    assert np.abs(N @ np.ones(N.shape[0])).max() <= 1e-12 * scale
    # W(u) = 0 for constant u
    const = np.tile(np.arange(1.0, dim + 1.0), x.shape[0])
    assert np.abs(R.W(const)).max() <= 1e-12 * np.abs(R.N(const)).max()
    # N(u) u = W(u) u = int (u . grad u) phi_i, both integrated exactly by the degree-5 rule
    a, b = N @ u, W @ u
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    # linear u: (u . grad) u = G (c + G x) is linear, so its exact load is the (exactly integrated) mass matrix times its nodal values
    rng = np.random.default_rng(5)
    G, c0 = rng.standard_normal((dim, dim)), rng.standard_normal(dim)
    ul = c0[None, :] + x @ G.T
    f = ul @ G.T
    load = R.mass_vec() @ f.ravel()
    got = R.N(ul.ravel()) @ ul.ravel()
    assert np.abs(got - load).max() <= 1e-12 * np.abs(load).max()


@pytest.mark.parametrize("dim,degree", [(2, 2), (2, 3), (2, 5), (3, 2), (3, 3), (3, 5)])
def test_quadrature_rules_are_exact_to_their_degree(fedd_lib, dim, degree):
    """The restatement takes the points and weights of its rules from the library's host tables, the P1 degree remapping
    included, so the rules are pinned here on their own: points inside the reference simplex, and every monomial of total
    degree <= the degree asked for integrated exactly, int x^a y^b z^c = a! b! c! / (a + b + c + dim)!."""
    from itertools import product
    from math import factorial
    pts, w = fedd_lib.fe_quadrature(dim, degree)
    assert np.all(pts >= 0.0) and np.all(pts.sum(axis=1) <= 1.0 + 1e-15)
    for e in product(range(degree + 1), repeat=dim):
        if sum(e) > degree:
            continue
        exact = np.prod([factorial(a) for a in e]) / factorial(sum(e) + dim)
        got = float(np.sum(w * np.prod(pts ** np.array(e)[None, :], axis=1)))
        assert abs(got - exact) <= 1e-14 / factorial(dim), (e, got, exact)

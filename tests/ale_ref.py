"""ALE convection, host side: a plain numpy restatement of P(w) (FE::assemblyAdditionalConvection, FE_def.hpp:3044-3255),
written from its formula,

    P(dim i + d, dim j + d) = |det B| sum_q w_q (div w_h)(x_q) phi_i(x_q) phi_j(x_q),
    div w_h(x_q)            = sum_i sum_d w[i][d] (grad phi_i B^-1)_d(x_q),

on the Restatement of tests/test_navier_stokes_abi.py, which supplies N and W.  The rule is the one of
determineDegree(dim, FE, FE, Std, Std, determineDegree(dim, FE, Grad)) (:3064-3065): the inner call gives 1 for P1 and for P2
(:5516-5543, a degree 0 is raised to 1), so the degree is 3 for P1 and 5 for P2 -- the rule of W.  tests/test_ale_ref.py checks
this file by identities that need no oracle; the GPU tests compare the device against it."""
import numpy as np
import scipy.sparse as sp

from test_navier_stokes_abi import Restatement, degrees


def degree_P(dim, nen):
    return 5 if nen > dim + 1 else 3


class AleRestatement(Restatement):
    """Restatement on the coordinates m["xyz"] (give it x_ref + d for a moved mesh) with P(w) and the fused matrices"""

    def __init__(self, fedd_lib, m):
        super().__init__(fedd_lib, m)
        assert degree_P(self.dim, self.nen) == degrees(self.dim, self.nen)[1]           # no rule of its own is needed

    def blocks_P(self, w, absolute=False):
        """element blocks [e, i, d1, j, d2]; absolute: every product replaced by its magnitude (rounding bounds)"""
        wq, phi, G = self.rule[degree_P(self.dim, self.nen)]
        Wn = self._U(w)
        f = np.abs if absolute else (lambda t: t)
        div = np.einsum("eid,eqid->eq", f(Wn), f(G))                                      # div w_h at x_q
        p = np.einsum("e,q,eq,qi,qj->eij", self.absdet, f(wq), div, f(phi), f(phi))
        return np.einsum("eij,ab->eiajb", p, np.eye(self.dim))

    def P(self, w, **kw):
        return self.assemble(self.blocks_P(w, **kw))

    def blocks_ale(self, kind, u, w):
        """kind: "P" | "FixedPoint" | "Newton" -- P(w) | N(u - w) - P(w) | N(u - w) + W(u) - P(w)"""
        u = None if u is None else np.asarray(u, dtype=np.float64).ravel()
        w = np.asarray(w, dtype=np.float64).ravel()
        if kind == "P":
            return self.blocks_P(w)
        b = self.blocks_N(u - w) - self.blocks_P(w)
        if kind == "Newton":
            b = b + self.blocks_W(u)
        return b

    def ale(self, kind, u, w):
        return self.assemble(self.blocks_ale(kind, u, w))

    def mass_vec_P(self):
        """the vector mass matrix on the rule of P (degree 3 integrates the P1 mass exactly, degree 5 the P2 mass)"""
        wq, phi, _ = self.rule[degree_P(self.dim, self.nen)]
        mloc = np.einsum("e,q,qi,qj->eij", self.absdet, wq, phi, phi)
        return self.assemble(np.einsum("eij,ab->eiajb", mloc, np.eye(self.dim)))


def on_pattern(parts, shape):
    """sum of matrices that share the FULL pattern, structural zeros kept (scipy's + drops them)"""
    rows = np.concatenate([np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)) for A in parts])
    cols = np.concatenate([A.indices for A in parts])
    data = np.concatenate([A.data for A in parts])
    S = sp.coo_matrix((data, (rows, cols)), shape=shape).tocsr()
    S.sort_indices()
    return S

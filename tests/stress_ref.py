"""numpy restatement of FE::assemblyStress (feddlib/core/FE/FE_def.hpp:2407-2733), the velocity block of Stokes / Navier-Stokes
in stress form ("Symmetric gradient"), element by element (test infrastructure).

Per element T with B = [p_2 - p_1, ...] (:2463, 2593), the transformed gradients g_i(k) = dPhiTrans[k][i] (:2470, 2597), and
the rule determineDegree(dim, FEType, FEType, Grad, Grad) (:2427):
    e_a^i = e_a (x) g_i               (e1i, e2i, e3i: row a holds g_i, :2513-2530, 2645-2669)
    e_b^j = E + E^T, E = e_b (x) g_j  (e1j, e2j, e3j, :2501-2527, 2639-2665)
    v_ab  = |det B| sum_k c(x_k) w_k  e_a^i : e_b^j            (SmallMatrix::innerProduct = Frobenius, SmallMatrix.hpp:164-196)
          = |det B| sum_k c(x_k) w_k ( delta_ab g_i . g_j + g_i[b] g_j[a] )
    inserted at row dim * gid(i) + a, column dim * gid(j) + b  (:2550-2559, 2707-2724; v21 -> row glob_i + 1, column glob_j)
    x_k = B xi_k + p_1                                          (:2487-2493, 2616-2625)
Every (a, b) of every node pair is inserted, structural zeros included: the FULL pattern."""
import numpy as np
import scipy.sparse as sp

import fedd_oracle as fo


def fe_type(m):
    return "P1" if m["conn"].shape[1] == m["dim"] + 1 else "P2"


def rule(m):
    """(xi [nq, dim], w [nq], dphi [nq, nen, dim]) of the form's quadrature rule"""
    dim, fe = m["dim"], fe_type(m)
    deg = fo.determine_degree(fe, fe, "Grad", "Grad")
    xi, w = fo.quadrature(dim, deg)
    dphi, w2 = fo.get_dphi(dim, fe, deg)
    assert np.array_equal(w, w2)
    return np.asarray(xi)[:, :dim], np.asarray(w), np.asarray(dphi)


def quadrature_points(m):
    """x_k = B xi_k + p_1 of every element: [n_elem, nq, dim]"""
    dim = m["dim"]
    xi, _, _ = rule(m)
    X = np.asarray(m["xyz"], dtype=np.float64)[np.asarray(m["conn"])[:, :dim + 1]]
    B = np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1))           # B[:, r] = p_{r+2} - p_1
    return np.einsum("eir,kr->eki", B, xi) + X[:, :1]


def element_matrix(dim, g, w, absdet, c):
    """[nen, dim, nen, dim]: v[i, a, j, b] of one element from g [nq, nen, dim], by the element loop's own expressions"""
    nq, nen, _ = g.shape
    v = np.zeros((nen, dim, nen, dim))
    for i in range(nen):
        for j in range(nen):
            for k in range(nq):
                for a in range(dim):
                    ei = np.zeros((dim, dim))
                    ei[a] = g[k, i]
                    for b in range(dim):
                        E = np.zeros((dim, dim))
                        E[b] = g[k, j]
                        v[i, a, j, b] += c[k] * w[k] * np.sum(ei * (E + E.T))
    return absdet * v


def element_matrix_fast(dim, g, w, absdet, c):
    """the same in closed form: delta_ab g_i . g_j + g_i[b] g_j[a]"""
    cw = c * w
    gg = np.einsum("k,kid,kjd->ij", cw, g, g)
    v = np.einsum("k,kib,kja->iajb", cw, g, g)
    for a in range(dim):
        v[:, a, :, a] += gg
    return absdet * v


def assemble(m, c_q=None, loops=False):
    """CSR [dim * n_global]^2 in global ids on the FULL pattern.  c_q [n_elem, nq] or None (c = 1).
    loops: the literal e_a^i : e_b^j evaluation (slow; small meshes), else its closed form."""
    dim = m["dim"]
    conn = np.asarray(m["conn"], dtype=np.int64)
    xyz = np.asarray(m["xyz"], dtype=np.float64)
    gid = np.asarray(m["gid_rep"], dtype=np.int64)
    _, w, dphi = rule(m)
    nq = w.shape[0]
    E, nen = conn.shape
    c_q = np.ones((E, nq)) if c_q is None else np.asarray(c_q, dtype=np.float64).reshape(E, nq)
    n = dim * int(m["n_global"])
    rows, cols, vals = [], [], []
    ar = np.arange(dim)
    fn = element_matrix if loops else element_matrix_fast
    for T in range(E):
        nodes = conn[T]
        X = xyz[nodes[:dim + 1]]
        B = (X[1:] - X[0]).T
        Binv = np.linalg.inv(B)
        absdet = abs(np.linalg.det(B))
        g = dphi @ Binv                                     # applyBTinv: dPhiTrans[k][i] = dPhi[k][i] B^-1
        v = fn(dim, g, w, absdet, c_q[T])
        r = dim * gid[nodes][:, None] + ar[None, :]
        R = np.broadcast_to(r[:, :, None, None], v.shape)
        C = np.broadcast_to(r[None, None, :, :], v.shape)
        rows.append(R.ravel()); cols.append(C.ravel()); vals.append(v.ravel())
    K = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    K.sort_indices()
    return K


def vector_laplacian(m):
    """the vector Laplacian on the same rule (delta_ab g_i . g_j alone): what the stress form replaces"""
    dim = m["dim"]
    conn = np.asarray(m["conn"], dtype=np.int64)
    xyz = np.asarray(m["xyz"], dtype=np.float64)
    gid = np.asarray(m["gid_rep"], dtype=np.int64)
    _, w, dphi = rule(m)
    n = dim * int(m["n_global"])
    K = sp.lil_matrix((n, n))
    for T in range(conn.shape[0]):
        nodes = conn[T]
        X = xyz[nodes[:dim + 1]]
        B = (X[1:] - X[0]).T
        g = dphi @ np.linalg.inv(B)
        gg = abs(np.linalg.det(B)) * np.einsum("k,kid,kjd->ij", w, g, g)
        for a in range(dim):
            idx = dim * gid[nodes] + a
            K[np.ix_(idx, idx)] += gg
    return K.tocsr()


def rotations(m):
    """the linearised rotations r(x) = W x, W skew, at the nodes: [dim * n_global, 1 | 3]"""
    dim = m["dim"]
    n = int(m["n_global"])
    x = np.zeros((n, dim))
    x[np.asarray(m["gid_rep"])] = m["xyz"]
    out = []
    for a in range(dim):
        for b in range(a + 1, dim):
            r = np.zeros((n, dim))
            r[:, a] = -x[:, b]
            r[:, b] = x[:, a]
            out.append(r.ravel())
    return np.stack(out, axis=1)


def jitter(m, amplitude=0.2, seed=11):
    """a copy of a structured P1 mesh dict whose interior nodes (flag 0... any node off the boundary of the unit box) are moved
    by a seeded uniform +-amplitude * h; call before p2_of_p1 so that the mid nodes stay on their (straight) edges"""
    out = dict(m)
    xyz = np.array(m["xyz"], dtype=np.float64)
    dim = m["dim"]
    X = xyz[np.asarray(m["conn"])[:, :dim + 1]]
    h = np.abs(X[:, 1:] - X[:, :1]).max(axis=2).min()
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    inner = np.all((xyz > lo + 1e-12) & (xyz < hi - 1e-12), axis=1)
    n = int(m["n_global"])
    d = np.random.default_rng(seed).uniform(-amplitude * h, amplitude * h, (n, dim))
    xyz[inner] += d[np.asarray(m["gid_rep"])[inner]]
    out["xyz"] = xyz
    return out

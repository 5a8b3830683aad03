"""numpy restatement of the interface distances and the scaled vector Laplacian of the mesh extension (test infrastructure).

Distances -- Domain::calculateDistancesToInterface (feddlib/core/FE/Domain_def.hpp:621-647) and the loop at the end of
MeshInterface::buildMeshInterfaceParallelAndDistance (feddlib/core/Mesh/MeshInterface_def.hpp:473-491):
    dist[i] = 1000.0; for every interface point j: d = sqrt(sum_k pow(x_i[k] - p_j[k], 2.0)); if dist[i] > d: dist[i] = d
the squares summed in ascending k from 0.0 (0.0 + s = s exactly), pow(t, 2.0) = t * t exactly, every operation rounded on its
own.  numpy's elementwise -, *, + and sqrt are those IEEE operations, so `distances` is the loop bit for bit.

Coefficient -- FE::assemblyLaplaceXDim (feddlib/core/FE/FE_def.hpp:2273-2278, 2343-2349) with HeuristicScaling
(feddlib/problems/specific/Geometry_def.hpp:24-34):
    mean = (d_0 + d_1 + d_2) / 3.0   |   (d_0 + d_1 + d_2 + d_3) / 4.0      over the first dim + 1 nodes, left to right
    f = coefficient if mean < distance else 1.0

Element loop (:2279-2316, 2350-2399), rule determineDegree(dim, FEType, FEType, Grad, Grad), no doSetZeros:
    val = 0; for k: val = val + f * w_k * (g_j(k) . g_i(k)); val = |det B| * val
    inserted at (dim * gid(i) + a, dim * gid(j) + a) for every component a: the DIAG pattern."""
import numpy as np
import scipy.sparse as sp

import stress_ref as sr

CAP = 1000.0


def distances(xyz, pts):
    """[n] from xyz [n, dim] and pts [n_pts, dim] (n_pts may be 0)"""
    xyz = np.asarray(xyz, dtype=np.float64)
    dim = xyz.shape[1]
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, dim)
    best = np.full(xyz.shape[0], np.inf)
    for j in range(pts.shape[0]):
        d2 = np.zeros(xyz.shape[0])
        for k in range(dim):
            t = xyz[:, k] - pts[j, k]
            d2 = d2 + t * t
        best = np.minimum(best, np.sqrt(d2))
    return np.minimum(CAP, best)


def interface_nodes(m, flags):
    """local repeated ids of the nodes whose flag is one of `flags`"""
    return np.flatnonzero(np.isin(np.asarray(m["flag_rep"]), np.atleast_1d(flags)))


def distances_to_flags(m, flags, xyz=None):
    x = np.asarray(m["xyz"] if xyz is None else xyz, dtype=np.float64)
    return distances(x, x[interface_nodes(m, flags)])


def element_means(m, dist):
    dim = m["dim"]
    d = np.asarray(dist, dtype=np.float64)[np.asarray(m["conn"])[:, :dim + 1]]
    s = d[:, 0]
    for v in range(1, dim + 1):
        s = s + d[:, v]
    return s / (3.0 if dim == 2 else 4.0)


def coefficients(m, dist, distance, coefficient):
    return np.where(element_means(m, dist) < distance, float(coefficient), 1.0)


def assemble(m, f_elem):
    """CSR [dim * n_global]^2 in global ids on the DIAG pattern, the element loop with f_elem [n_elem]"""
    dim = m["dim"]
    conn = np.asarray(m["conn"], dtype=np.int64)
    xyz = np.asarray(m["xyz"], dtype=np.float64)
    gid = np.asarray(m["gid_rep"], dtype=np.int64)
    _, w, dphi = sr.rule(m)
    n = dim * int(m["n_global"])
    rows, cols, vals = [], [], []
    for T in range(conn.shape[0]):
        nodes = conn[T]
        X = xyz[nodes[:dim + 1]]
        B = (X[1:] - X[0]).T
        g = dphi @ np.linalg.inv(B)                     # applyBTinv: dPhiTrans[k][i] = dPhi[k][i] B^-1
        absdet = abs(np.linalg.det(B))
        val = np.zeros((nodes.shape[0], nodes.shape[0]))
        for k in range(w.shape[0]):
            val = val + f_elem[T] * w[k] * (g[k] @ g[k].T)
        val = absdet * val
        for a in range(dim):
            idx = dim * gid[nodes] + a
            rows.append(np.repeat(idx, idx.shape[0])); cols.append(np.tile(idx, idx.shape[0])); vals.append(val.ravel())
    K = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    K.sort_indices()
    return K

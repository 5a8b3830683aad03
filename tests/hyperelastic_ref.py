"""numpy restatement of the hyperelastic assembly (test infrastructure): the materials in closed form, and the element loop of
FE::assemblyElasticityJacobianAndStressAceFEM (feddlib/core/FE/FE_def.hpp:1123-1267 in 3D, :928-1066 in 2D) step by step, for
P1 / P2 in 2D / 3D.  The reference evaluates the materials with machine-generated routines (nh3d, mr3d, stvk3d, stvk2d,
:6969-7803); tests/golden/hyperelastic_materials.npz holds what those return, and test_hyperelastic_materials.py pins the
closed forms below against it."""
import numpy as np
import scipy.sparse as sp

import fedd_oracle as fo

NEOHOOKE, MOONEY_RIVLIN, STVK = "Neo-Hooke", "Mooney-Rivlin", "Saint Venant-Kirchhoff"
MODELS = (NEOHOOKE, MOONEY_RIVLIN, STVK)


def lame(E, nu):
    """mu, lambda as the generated routines derive them from E and nu (nh3d: FE_def.hpp:6973-6975)"""
    return E / (2.0 * (1.0 + nu)), E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))


def stvk_params(mu, nu):
    """what the caller hands to stvk2d / stvk3d: E = 2 mu (1 + nu), lambda from it (FE_def.hpp:887-896) -> (lambda, mu)"""
    E = mu * 2.0 * (1.0 + nu)
    return (nu * E) / ((1.0 + nu) * (1.0 - 2.0 * nu)), mu


def material(model, params, F):
    """P [d, d] and A [d, d, d, d] = dP_ij / dF_kl.
    params: Neo-Hooke (E, nu); Mooney-Rivlin (E, nu, C); Saint Venant-Kirchhoff (lambda, mu)"""
    F = np.asarray(F, dtype=np.float64)
    d = F.shape[0]
    I = np.eye(d)
    C = F.T @ F
    b = F @ F.T
    II = np.einsum("ik,jl->ijkl", I, I)
    if model == STVK:
        lam, mu = params
        E = 0.5 * (C - I)
        S = lam * np.trace(E) * I + 2.0 * mu * E
        P = F @ S
        A = (np.einsum("ik,lj->ijkl", I, S) + lam * np.einsum("ij,kl->ijkl", F, F)
             + mu * (np.einsum("il,kj->ijkl", F, F) + np.einsum("ik,jl->ijkl", b, I)))
        return P, A
    J = np.linalg.det(F)
    if not J > 0.0:
        raise ValueError("det F = %g <= 0: the material takes ln det F" % J)
    G = np.linalg.inv(F).T
    lnJ = np.log(J)
    GG = np.einsum("ij,kl->ijkl", G, G)
    GxG = np.einsum("il,kj->ijkl", G, G)
    if model == NEOHOOKE:
        mu, lam = lame(params[0], params[1])
        P = mu * (F - G) + lam * lnJ * G
        A = mu * II + lam * GG + (mu - lam * lnJ) * GxG
        return P, A
    if model == MOONEY_RIVLIN:
        E, nu, c = params
        mu = E / (2.0 * (1.0 + nu))
        kap = E / (3.0 * (1.0 - 2.0 * nu))
        I1 = np.trace(C)
        P = (1.0 - c) * mu * (F - G) + c * mu * (I1 * F - F @ C - 2.0 * G) + kap * lnJ * G
        A = ((1.0 - c) * mu * II
             + c * mu * (2.0 * np.einsum("ij,kl->ijkl", F, F) + I1 * II - np.einsum("ik,lj->ijkl", I, C)
                         - np.einsum("il,kj->ijkl", F, F) - np.einsum("jl,ik->ijkl", I, b))
             + kap * GG + (mu * (1.0 + c) - kap * lnJ) * GxG)
        return P, A
    raise ValueError("unknown material model %r" % (model,))


def fe_type(m):
    return "P1" if m["conn"].shape[1] == m["dim"] + 1 else "P2"


def assemble(m, u_rep, model, params):
    """(K, f, min J): the tangent in GLOBAL dof ids on the full node-block pattern (structural zeros kept, as insertGlobalValues
    leaves them), the force in global dof ids, the smallest det F met.  m: a one-rank mesh dict of feddlib_amd.capi; u_rep:
    [n_rep, dim] on its repeated map.  Saint Venant-Kirchhoff only in 2D (:903)."""
    dim = m["dim"]
    if dim == 2 and model != STVK:
        raise ValueError("Only Saint Venant-Kirchhoff in 2D.")
    fe = fe_type(m)
    conn = np.asarray(m["conn"], dtype=np.int64)
    xyz = np.asarray(m["xyz"], dtype=np.float64)
    gid = np.asarray(m["gid_rep"], dtype=np.int64)
    u = np.asarray(u_rep, dtype=np.float64).reshape(-1, dim)
    deg = fo.determine_degree(fe, fe, "Grad", "Grad")                 # :856
    dphi, w = fo.get_dphi(dim, fe, deg)                               # [Q, nen, dim], [Q]
    nq, nen = dphi.shape[0], dphi.shape[1]
    nall = nen * dim
    ssz = dim * dim
    n_glob = int(m["n_global"]) * dim
    f = np.zeros(n_glob)
    rows, cols, vals = [], [], []
    minJ = np.inf
    for T in range(conn.shape[0]):
        nodes = conn[T]
        X = xyz[nodes[:dim + 1]]
        B = (X[1:] - X[0]).T                                          # buildTransformation
        Binv = np.linalg.inv(B)
        absdet = abs(np.linalg.det(B))
        loc_stiff = np.zeros((nall, nall))
        loc_stress = np.zeros(nall)
        for p in range(nq):
            g = dphi[p] @ Binv                                        # row i: grad phi_i B^-1      (:1131-1134)
            F = np.eye(dim)
            for i in range(nen):
                for j in range(dim):
                    F[j, :] += u[nodes[i], j] * g[i]                  # F += u_ij (e_j (x) g_i)      (:1143-1156)
            minJ = min(minJ, np.linalg.det(F))
            P, A = material(model, params, F)
            Aloc = A.reshape(ssz, ssz)                                # Aloc[d i + j][d k + l]       (:1183-1192)
            D = np.zeros((ssz, nall))                                 # allDPhiBlas, column (i, j) = rows of e_j (x) g_i (:1202-1207)
            for i in range(nen):
                for j in range(dim):
                    D[j * dim:(j + 1) * dim, dim * i + j] = g[i]
            loc_stiff += w[p] * (D.T @ (Aloc @ D))                    # the two GEMMs, :1209-1222
            loc_stress += w[p] * (D.T @ P.reshape(ssz))               # GEMV, :1229-1243
        dof = (dim * gid[nodes][:, None] + np.arange(dim)[None, :]).ravel()
        f[dof] += absdet * loc_stress                                 # :1251-1253
        rows.append(np.repeat(dof, nall))
        cols.append(np.tile(dof, nall))
        vals.append((absdet * loc_stiff).ravel())                     # :1258-1262
    K = fo.fill_complete(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), n_glob)
    return K, f, minJ


def stress_term_magnitude(model, params, F):
    """[d, d]: the sum of the magnitudes of the terms the closed form of P adds up, entry by entry -- the size of the numbers
    that cancel when P is small against the moduli (the running-error scale of the evaluation)"""
    F = np.asarray(F, dtype=np.float64)
    d = F.shape[0]
    I = np.eye(d)
    aF = np.abs(F)
    C = F.T @ F
    if model == STVK:
        lam, mu = params
        trE = 0.5 * (np.trace(C) - d)
        return aF @ (abs(lam * trE) * I + mu * (np.abs(C) + I))
    G = np.abs(np.linalg.inv(F).T)
    lnJ = abs(np.log(np.linalg.det(F)))
    if model == NEOHOOKE:
        mu, lam = lame(params[0], params[1])
        return mu * (aF + G) + lam * lnJ * G
    E, nu, c = params
    mu = E / (2.0 * (1.0 + nu))
    kap = E / (3.0 * (1.0 - 2.0 * nu))
    return abs(1.0 - c) * mu * (aF + G) + abs(c) * mu * (np.trace(C) * aF + aF @ np.abs(C) + 2.0 * G) + kap * lnJ * G


def residual_rounding_scale(m, u_rep, model, params):
    """[global dofs]: per row, the sum of the magnitudes of everything the internal force adds up there -- |det B| w_p
    sum_k (term magnitudes of P)_dk |g_i,k| over elements and points.  One unit roundoff of it is the accuracy to which a row of
    the residual can be evaluated in floating point, whatever the order of the sums."""
    dim = m["dim"]
    fe = fe_type(m)
    conn = np.asarray(m["conn"], dtype=np.int64)
    xyz = np.asarray(m["xyz"], dtype=np.float64)
    gid = np.asarray(m["gid_rep"], dtype=np.int64)
    u = np.asarray(u_rep, dtype=np.float64).reshape(-1, dim)
    dphi, w = fo.get_dphi(dim, fe, fo.determine_degree(fe, fe, "Grad", "Grad"))
    out = np.zeros(int(m["n_global"]) * dim)
    for T in range(conn.shape[0]):
        nodes = conn[T]
        X = xyz[nodes[:dim + 1]]
        B = (X[1:] - X[0]).T
        Binv = np.linalg.inv(B)
        absdet = abs(np.linalg.det(B))
        for p in range(dphi.shape[0]):
            g = dphi[p] @ Binv
            F = np.eye(dim) + u[nodes].T @ g
            S = stress_term_magnitude(model, params, F)
            out[(dim * gid[nodes][:, None] + np.arange(dim)[None, :]).ravel()] += (absdet * abs(w[p]) * (np.abs(g) @ S.T)).ravel()
    return out


def dirichlet_mask(m, bc_flags=(2,)):
    """boolean mask over the global dofs of the nodes whose flag is in bc_flags (all components)"""
    flags = np.zeros(int(m["n_global"]), dtype=np.int32)
    flags[m["gid_uni"]] = m["flag_uni"]
    return fo.dirichlet_rows(flags, bc_flags, dofs=m["dim"])


def newton(m, model, params, rhs, is_dir, tol=1e-12, max_it=25, assemble_fn=None, solve_fn=None):
    """Newton's method as NonLinearSolver runs it on NonLinElasticity with zero Dirichlet values: residual r = f(u) - rhs with the
    Dirichlet rows set to zero, K du = -r with unit Dirichlet rows, u += du, until |r| / |r_0| <= tol.
    Returns (u [global dofs], ratios per iteration incl. the first, iterations).  assemble_fn(u_glob) -> (K, f) and
    solve_fn(K_bc, b) default to the restatement and a sparse direct solve."""
    import scipy.sparse.linalg as spla
    dim = m["dim"]
    gid = np.asarray(m["gid_rep"], dtype=np.int64)
    n = rhs.shape[0]
    u = np.zeros(n)
    if assemble_fn is None:
        def assemble_fn(ug):
            K, f, _ = assemble(m, ug.reshape(-1, dim)[gid], model, params)
            return K, f
    if solve_fn is None:
        def solve_fn(Kbc, b):
            return spla.spsolve(Kbc.tocsc(), b)
    ratios = []
    r0 = None
    for it in range(max_it + 1):
        K, f = assemble_fn(u)
        r = f - rhs
        r[is_dir] = 0.0
        nr = np.linalg.norm(r)
        if r0 is None:
            r0 = nr
        ratios.append(nr / r0)
        if ratios[-1] <= tol:
            return u, ratios, it
        Kbc, b = fo.set_dirichlet(K, -r, is_dir, 0.0)
        u = u + solve_fn(Kbc, b)
    raise RuntimeError("Newton did not reach %g in %d iterations: %r" % (tol, max_it, ratios))

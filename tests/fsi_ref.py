"""Host restatement (numpy / scipy) of the FSI coupling in include/fedd_hip.h "FSI coupling": the matched interface, the
four-block coupled matrix and the FaCSI apply.  Written from the formulas stated there; the GPU tests compare the device
entries against it, tests/test_fsi_ref.py checks it against properties that do not depend on it.

    [ F    B^T  0    C1^T ] [u]        C1  : +1 at (lambda-dof, fluid interface dof)          C1^T: its transpose
    [ B    C    0    0    ] [p]        C2  : -(1/dt) at (lambda-dof, structure interface dof)
    [ 0    0    S    C3^T ] [d]        C3^T: -1 at (structure interface dof, lambda-dof)
    [ C1   0    C2   D    ] [l]        D   : 1 on the diagonal of uncoupled lambda-dofs
"""
import numpy as np
import scipy.sparse as sp


def unique_coords(m):
    """coordinates of a capi mesh dict in the order of its unique map (the owned node ids of the device layer)"""
    pos = {int(g): i for i, g in enumerate(m["gid_rep"])}
    return np.array([m["xyz"][pos[int(g)]] for g in m["gid_uni"]], dtype=np.float64).reshape(len(m["gid_uni"]), -1)


def match(x_f, flag_f, x_s, flag_s, flags):
    """per flag, in the order given: the nodes of each side that carry it, ordered lexicographically by (x, y[, z]), paired by
    rank.  Returns (iface_f, iface_s, flag_ptr)."""
    out_f, out_s, ptr = [], [], [0]
    for fl in flags:
        side = []
        for x, flag in ((x_f, flag_f), (x_s, flag_s)):
            ids = np.nonzero(np.asarray(flag) == fl)[0]
            keys = tuple(x[ids, k] for k in reversed(range(x.shape[1])))      # lexsort: the LAST key is the primary one
            side.append(ids[np.lexsort(keys)])
        if side[0].shape[0] != side[1].shape[0]:
            raise ValueError("flag %d: %d fluid and %d structure nodes" % (fl, side[0].shape[0], side[1].shape[0]))
        out_f.append(side[0])
        out_s.append(side[1])
        ptr.append(ptr[-1] + side[0].shape[0])
    return (np.concatenate(out_f).astype(np.int32), np.concatenate(out_s).astype(np.int32), np.array(ptr, dtype=np.int64))


def interface_dofs(iface_f, iface_s, dim, mask=None):
    """fdof[k], sdof[k] of interface dof k = dim * pair + component; -1 where the mask uncouples"""
    n_l = dim * iface_f.shape[0]
    k = np.arange(n_l)
    fdof = dim * iface_f[k // dim].astype(np.int64) + k % dim
    sdof = dim * iface_s[k // dim].astype(np.int64) + k % dim
    if mask is not None:
        off = np.asarray(mask) == 0
        fdof[off] = -1
        sdof[off] = -1
    return fdof, sdof


def coupled_csr(F, S, dir_f, dir_s, fdof, sdof, dt):
    """the coupled matrix as explicit CSR arrays (rowptr, col, val), stored entries of the children kept one for one, columns
    ascending.  F, S: (rowptr, col, val) of the children's systems; dir_f, dir_s: their Dirichlet marks (bool per row)."""
    n_f, n_s, n_l = len(F[0]) - 1, len(S[0]) - 1, fdof.shape[0]
    off_l = n_f + n_s
    c2 = -(1.0 / dt)
    lam_f = -np.ones(n_f, dtype=np.int64)
    lam_s = -np.ones(n_s, dtype=np.int64)
    lam_f[fdof[fdof >= 0]] = np.nonzero(fdof >= 0)[0]
    lam_s[sdof[sdof >= 0]] = np.nonzero(sdof >= 0)[0]
    rowptr, col, val = [0], [], []
    for (rp, ci, v), lam, dr, shift, cv in ((F, lam_f, dir_f, 0, 1.0), (S, lam_s, dir_s, n_f, -1.0)):
        for i in range(len(rp) - 1):
            a, b = int(rp[i]), int(rp[i + 1])
            col.extend((np.asarray(ci[a:b], dtype=np.int64) + shift).tolist())
            val.extend(np.asarray(v[a:b]).tolist())
            if lam[i] >= 0 and not dr[i]:
                col.append(off_l + int(lam[i]))
                val.append(cv)
            rowptr.append(len(col))
    for k in range(n_l):
        if fdof[k] >= 0:
            col.extend([int(fdof[k]), n_f + int(sdof[k])])
            val.extend([1.0, c2])
        else:
            col.append(off_l + k)
            val.append(1.0)
        rowptr.append(len(col))
    return np.array(rowptr, dtype=np.int64), np.array(col, dtype=np.int32), np.array(val, dtype=np.float64)


def to_scipy(csr, n=None):
    rowptr, col, val = csr
    n = len(rowptr) - 1 if n is None else n
    return sp.csr_matrix((val, col, rowptr), shape=(len(rowptr) - 1, n))


def interface_rhs(sdof, d_old, dt):
    c2 = -(1.0 / dt)
    out = np.zeros(sdof.shape[0])
    on = sdof >= 0
    out[on] = c2 * np.asarray(d_old)[sdof[on]]
    return out


def facsi_apply(A, n_u, n_f, n_s, fdof, sdof, dt, x, apply_f, apply_s):
    """y = P^-1 x: A the coupled matrix (scipy CSR), apply_f / apply_s the children's preconditioner applies"""
    off_l = n_f + n_s
    c2 = -(1.0 / dt)
    on = fdof >= 0
    x_f, x_d, x_l = x[:n_f], x[n_f:off_l], x[off_l:]
    y_d = apply_s(x_d.copy())
    g = x_l[on] - c2 * y_d[sdof[on]]
    t = x_f.copy()
    t[fdof[on]] = g
    y_f = apply_f(t)
    rows = A[fdof[on], :]
    bt = rows[:, n_u:n_f] @ y_f[n_u:]
    f = rows[:, :n_u] @ y_f[:n_u]
    y_l = x_l.copy()                    # uncoupled dofs: the identity
    y_l[on] = (x_f[fdof[on]] - bt) - f
    return np.concatenate([y_f, y_d, y_l])

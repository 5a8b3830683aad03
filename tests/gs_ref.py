"""Plain reference of one block of the s-step Gram-Schmidt (BCGS-PIP2, csrc/gmres_sstep.hip): numpy only, no GPU.

The two sweeps over the basis have longdouble references (64-bit significand on x86) with the product of absolute values beside
them, which is what a rounding bound of a dot product or an update is stated against.  The small matrix work between the
sweeps -- gram_minus, chol_cut, the combined C and R, the Hessenberg columns -- is restated operation by operation from the
kernels k_ss_pass1 / k_ss_pass2 and runs in float64 or in longdouble.  In float64 the restatement keeps the kernels' order of
operations, and where the device compiler contracts a product and a sum (the library is built with the compiler's default,
contraction on) it rounds once, as the fused multiply-add does (`fma`, exact through integers).

Conventions: a basis piece is (rows, columns); P is (k + sa, S) with P[c, j] = V_c . W_j; cf is (k, S), ri is (S, S) upper
triangular; H is (m + 1, columns)."""
import numpy as np

LD = np.longdouble
HAVE_LONGDOUBLE = np.finfo(LD).nmant >= 63
U = 2.0 ** -53


def fma(a, b, c):
    """a * b + c of three floats, rounded once (Python's integer division rounds correctly)"""
    na, da = float(a).as_integer_ratio()
    nb, db = float(b).as_integer_ratio()
    nc, dc = float(c).as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def _muladd(dtype):
    if dtype is np.float64:
        return fma
    return lambda a, b, c: a * b + c


def gram(V0, k, sa):
    """[Q W]^T W for Q = V0[:, :k], W = V0[:, k:k+sa], in longdouble, and |V0|^T |W|"""
    V = np.asarray(V0[:, :k + sa], dtype=LD)
    W = V[:, k:k + sa]
    return V.T @ W, np.abs(V).T @ np.abs(W)


def update(Vcols, W, cf, ri, sa):
    """(W - Q cf) ri for the first sa columns, in longdouble, and (|W| + |Q| |cf|) |ri|"""
    Q = np.asarray(Vcols, dtype=LD)
    Wl = np.asarray(W[:, :sa], dtype=LD)
    c = np.asarray(cf[:Q.shape[1], :sa], dtype=LD)
    r = np.asarray(ri[:sa, :sa], dtype=LD)
    return (Wl - Q @ c) @ r, (np.abs(Wl) + np.abs(Q) @ np.abs(c)) @ np.abs(r)


def gram_minus(P, k, S, dtype=np.float64):
    """G = W^T W and A = G - C^T C from P (four partial sums over the basis columns, as the kernel takes them); the upper
    triangles of the rows P holds -- all chol_cut reads"""
    P = np.asarray(P, dtype=dtype)
    ma = _muladd(dtype)
    G = np.zeros((S, S), dtype=dtype)
    A = np.zeros((S, S), dtype=dtype)
    rows = P.shape[0] - k
    for i in range(min(S, rows)):
        for j in range(i, min(S, rows)):
            s = [dtype(0.0)] * 4
            c = 0
            while c + 4 <= k:
                for u in range(4):
                    s[u] = dtype(ma(P[c + u, i], P[c + u, j], s[u]))
                c += 4
            while c < k:
                s[0] = dtype(ma(P[c, i], P[c, j], s[0]))
                c += 1
            G[i, j] = P[k + i, j]
            A[i, j] = G[i, j] - ((s[0] + s[1]) + (s[2] + s[3]))
    return G, A


def chol_cut(A, gdiag, sa, tol, dtype=np.float64):
    """upper Cholesky factor of the unit-diagonal scaling of A[:sa, :sa], cut at the first pivot with
    pivot * A[c, c] <= tol * gdiag[c].  Returns (accepted, R, Ri, ratios): ratios[c] = pivot * A[c, c] / (tol * gdiag[c]) of
    every column that was examined (the cut is decided by ratio > 1)"""
    S = A.shape[0]
    ma = _muladd(dtype)
    one = dtype(1.0)
    dd = np.zeros(S, dtype=dtype)
    for i in range(sa):
        if A[i, i] > 0:
            dd[i] = np.sqrt(A[i, i])
    W = np.zeros((S, S), dtype=dtype)
    for i in range(S):
        for j in range(i, S):
            if dd[i] > 0 and dd[j] > 0:
                W[i, j] = A[i, j] / (dd[i] * dd[j])
    R = np.zeros((S, S), dtype=dtype)
    Ri = np.zeros((S, S), dtype=dtype)
    ok = sa
    ratios = []
    for c in range(sa):
        piv = W[c, c]
        if tol * gdiag[c] > 0:
            ratios.append(float(piv * A[c, c] / (tol * gdiag[c])))
        if not (dd[c] > 0) or not (piv > 0) or not (piv * A[c, c] > tol * gdiag[c]):
            ok = c
            break
        rp = one / np.sqrt(W[c, c])
        R[c, c:] = W[c, c:] * rp
        for i in range(c + 1, S):
            for j in range(i, S):
                W[i, j] = dtype(ma(-R[c, i], R[c, j], W[i, j]))
    for i in range(S):
        for j in range(S):
            R[i, j] = R[i, j] * dd[j] if (i <= j and j < ok) else 0.0
    for cj in range(ok):
        Ri[cj, cj] = one / R[cj, cj]
        for r in range(cj - 1, -1, -1):
            acc = dtype(0.0)
            for p in range(r + 1, cj + 1):
                acc = dtype(ma(R[r, p], Ri[p, cj], acc))
            Ri[r, cj] = -acc / R[r, r]
    return ok, R, Ri, ratios


def pass1(P, k, sa, tol, S, dtype=np.float64):
    """k_ss_pass1: returns dict(sa, cf, R, Ri, ratios)"""
    P = np.asarray(P, dtype=dtype)
    G, A = gram_minus(P, k, S, dtype)
    ok, R, Ri, ratios = chol_cut(A, np.diag(G).copy(), sa, tol, dtype)
    return {"sa": ok, "cf": P[:k].copy(), "R": R, "Ri": Ri, "ratios": ratios}


def pass2(P, k, sa1, tol, S, p1, Hbar, th, dtype=np.float64):
    """k_ss_pass2 without the Givens rotations.  P: the second products; p1: what pass1 returned (its cf is C1); Hbar: the
    final Hessenberg columns 0 .. k - 2, at least k rows; th: the S shifts.  Returns dict(sa, cf, Ri, Cc, Rc, ratios, H) with
    H = the new raw columns k - 1 .. k + sa - 2, (k + sa) rows (one column if sa = 0: breakdown)"""
    P = np.asarray(P, dtype=dtype)
    th = np.asarray(th, dtype=dtype)
    R1, R1i, C1 = p1["R"].astype(dtype), p1["Ri"].astype(dtype), p1["cf"].astype(dtype)
    sa, R2, R2i, ratios = 0, np.zeros((S, S), dtype), np.zeros((S, S), dtype), []
    if sa1 > 0:
        G, A = gram_minus(P, k, S, dtype)
        sa, R2, R2i, ratios = chol_cut(A, np.diag(G).copy(), sa1, tol, dtype)
    out = {"sa": sa, "cf": P[:k].copy(), "Ri": R2i, "ratios": ratios}
    Hk = np.zeros((k + 1, k), dtype=dtype)                 # Hbar_k with the column k - 1 of this block
    if k > 1:
        Hk[:k, :k - 1] = np.asarray(Hbar, dtype=dtype)[:k, :k - 1]
    if sa == 0:
        Hk[:k, k - 1] = C1[:, 0]
        Hk[k - 1, k - 1] += th[0]
        out.update(Cc=C1, Rc=np.zeros((S, S), dtype), H=Hk[:, k - 1:k].copy())
        return out
    Rc = np.zeros((S, S), dtype)
    Rci = np.zeros((S, S), dtype)
    Rc[:sa, :sa] = (R2 @ R1)[:sa, :sa]
    Rci[:sa, :sa] = (R1i @ R2i)[:sa, :sa]
    Cc = C1 + P[:k] @ np.triu(R1)
    Hk[:k, k - 1] = Cc[:, 0]
    Hk[k - 1, k - 1] += th[0]
    Hk[k, k - 1] = Rc[0, 0]
    H = np.zeros((k + sa, sa), dtype=dtype)
    H[:k + 1, 0] = Hk[:, k - 1]
    nc = sa - 1
    if nc > 0:
        top = np.vstack([Cc[:, :sa], Rc[:sa, :sa]])        # [C; R], (k + sa) x sa
        X = top[:, 1:sa] + top[:, :nc] * th[1:sa][None, :]
        X[:k + 1] -= Hk @ Cc[:, :nc]
        Hn = X @ Rci[:nc, :nc]
        for c in range(nc):
            H[:k + c + 2, 1 + c] = Hn[:k + c + 2, c]
    out.update(Cc=Cc, Rc=Rc, H=H)
    return out


def block(V0, k, sa_req, S, tol, Hbar, th, dtype=np.float64):
    """one whole block from the basis V0 (columns k .. k + sa_req - 1 hold the operator's products): both passes with plain
    products in `dtype`.  Returns dict(sa1, sa, V, H): V = the basis columns 0 .. k + sa - 1 afterwards, H = all raw
    Hessenberg columns 0 .. k + max(sa, 1) - 2 with k + max(sa, 1) rows"""
    V = np.array(V0[:, :k + sa_req], dtype=dtype)
    Q = V[:, :k]
    P1 = V.T @ V[:, k:]
    P1 = np.hstack([P1, np.zeros((k + sa_req, S - sa_req), dtype)])
    p1 = pass1(P1, k, sa_req, tol, S, dtype)
    sa1 = p1["sa"]
    W = V[:, k:k + sa1]
    W1 = (W - Q @ p1["cf"][:, :sa1]) @ p1["Ri"][:sa1, :sa1]
    P2 = np.zeros((k + sa_req, S), dtype)
    P2[:k, :sa1] = Q.T @ W1
    P2[k:k + sa1, :sa1] = W1.T @ W1
    p2 = pass2(P2, k, sa1, tol, S, p1, Hbar, th, dtype)
    sa = p2["sa"]
    W2 = (W1[:, :sa] - Q @ p2["cf"][:, :sa]) @ p2["Ri"][:sa, :sa]
    ncol = max(sa, 1)
    H = np.zeros((k + ncol, k - 1 + ncol), dtype)
    if k > 1:
        H[:k, :k - 1] = np.asarray(Hbar, dtype=dtype)[:k, :k - 1]
    H[:p2["H"].shape[0], k - 1:] = p2["H"]
    return {"sa1": sa1, "sa": sa, "V": np.hstack([Q, W2]), "H": H, "p1": p1, "p2": p2}


def orthogonality(V):
    """max |V^T V - I| in longdouble"""
    Vl = np.asarray(V, dtype=LD)
    return float(np.abs(Vl.T @ Vl - np.eye(V.shape[1], dtype=LD)).max())


def arnoldi_residual(apply_B, normB, V, H):
    """||B V[:, :j] - V[:, :j+1] H[:j+1, :j]||_F / (||B||_F ||V[:, :j]||_F), j = columns of H, in longdouble
    (apply_B maps a longdouble (rows, j) array to B times it)"""
    j = H.shape[1]
    Vl = np.asarray(V[:, :j + 1], dtype=LD)
    BV = apply_B(Vl[:, :j])
    res = BV - Vl @ np.asarray(H[:j + 1, :j], dtype=LD)
    return float(np.sqrt((res * res).sum()) / (LD(normB) * np.sqrt((Vl[:, :j] ** 2).sum())))

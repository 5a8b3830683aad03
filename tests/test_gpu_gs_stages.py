"""The s-step Gram-Schmidt kernels stage by stage, inside a real solve.

fedd_gmres_capture_* copies one block of the s-step solve (csrc/gmres_sstep.hip, SStep::orthogonalise) piece by piece (the basis before the block, the reduced products,
the coefficients of both passes, the block after each update, the raw Hessenberg columns); every piece is compared here with
tests/gs_ref.py: the two sweeps with their longdouble references under bounds that hold for any summation order
(u = 2^-53, elementwise, against the product of absolute values), the small matrix work with the float64 restatement of the
kernels run on the device's own products.

Systems: unpreconditioned Laplace with the seeded noisy right-hand side of test_gpu_dot_own (f = 1 with boundary conditions
plus 0.3 max |f| of normal noise, seed = cells per side), operator = the CSR read back.  512 / 729 / 1024 / 1089 / 4913 rows:
one update workgroup exactly, one and a partial one with a single row in the last lane, one dot workgroup exactly, 1024 + 65,
and five dot workgroups with cycles that reach k + sa >= 65 columns (the mid-loop LDS flush).

Cut blocks: the updates do not write the columns from the accepted count on (k_blockaxpy: "columns >= sa untouched"), so in
W1 / W2 they still hold what they held before -- asserted bit for bit against the earlier piece.

Measured on an MI355X, largest over the 75 blocks of this file (each test prints its own): RI1 / RI2 ratio 0.000 of the
allowed 8 (every entry equals the float64 restatement bit for bit), orthogonality 0.86 and Arnoldi residual 1.91 times the
float64 reference's figure (allowed 8)."""
import numpy as np
import pytest

import fedd_oracle as fo
import gs_ref

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gs_ref.HAVE_LONGDOUBLE, reason="np.longdouble has no 64-bit significand here")]

U = gs_ref.U
LD = np.longdouble
RTOL = 1e-10
CHOL_TOL_DEFAULT = 1e-13
_RHS = {}
SYSTEMS = {"3d7": (3, 7, 512), "3d8": (3, 8, 729), "2d31": (2, 31, 1024), "2d32": (2, 32, 1089), "3d16": (3, 16, 4913)}


def _system(L, c, dim, M):
    """assembles the M^dim-cell Laplace on c; returns (b, operator): the right-hand side (computed once per system) and the
    CSR of the assembled system as the device holds it"""
    m = L.structured_mesh(dim, 1, M)
    c.mesh_set_dict(m)
    c.pattern_build(1, L.BLOCK_SCALAR)
    c.assemble(L.FORM_LAPLACE)
    c.assemble_rhs([1.0])
    c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    if (dim, M) not in _RHS:
        om = fo.Mesh(dim=m["dim"], fe="P1", conn=m["conn"], xyz=m["xyz"], gid_rep=m["gid_rep"], flag_rep=m["flag_rep"],
                     gid_uni=m["gid_uni"], flag_uni=m["flag_uni"], xyz_uni=None, n_global=m["n_global"])
        rhs_bc = fo.laplace_problem(om)[1]
        b = rhs_bc + 0.3 * np.abs(rhs_bc).max() * np.random.default_rng(M).standard_normal(rhs_bc.shape[0])
        b.setflags(write=False)
        _RHS[(dim, M)] = b
    rowptr, col, val, _ = c.csr_get()
    return _RHS[(dim, M)], (rowptr, col.astype(np.int64), val.astype(LD))


def _apply(op, X):
    """B X in longdouble"""
    rowptr, col, val = op
    return np.add.reduceat(val[:, None] * X[col], rowptr[:-1], axis=0)


def _plan(s, restart, block):
    """(k, sa_req) of the block-th block of the first restart cycle when no block is cut and nothing converges: blocks of
    min(s, 8) until the Newton shifts exist (s > 8: from k - 1 >= s on), the last one cut by the room; shifted = has shifts"""
    k, s_cur, shifted = 1, min(s, 8), False
    for _ in range(block):
        k += min(s_cur, restart - (k - 1))
        assert k - 1 < restart, "the block lies behind the first cycle"
        if s > 8 and k - 1 >= s:
            s_cur, shifted = s, True
    return k, min(s_cur, restart - (k - 1)), shifted


def _restore(c):
    c.gmres_capture_arm(-1)
    c.set_option("gmres_dot_own", 1)
    c.set_option("gmres_chol_tol", CHOL_TOL_DEFAULT)
    c.set_option("gmres_tol_blocks", 1)
    c.set_option("gmres_dot_gy", 0)
    c.set_option("gmres_fuse", -1)
    c.set_option("gmres_s", 0)
    c.set_option("gmres_kind", 2)


def _near_threshold(ratios):
    return any(abs(r - 1.0) <= 1e-3 for r in ratios)


def _check_ri(label, RI, f64, ld, S, worst):
    """|RI - pass_f64| <= max(8 |pass_f64 - pass_longdouble|, S u |RI|) elementwise; the ratio |RI - pass_f64| /
    max(|pass_f64 - pass_longdouble|, S u |RI| / 8) is what the assertion holds below 8: its largest value goes to `worst`"""
    move = np.maximum(np.abs(f64 - np.asarray(ld, dtype=LD)).astype(np.float64), S * U * np.abs(RI) / 8.0)
    dev = np.abs(RI - f64)
    ratio = float(np.max(np.where(dev > 0, dev / np.where(move > 0, move, 1.0), 0.0)))
    assert not (dev[move == 0] > 0).any(), label
    worst["ri"] = max(worst["ri"], ratio)
    assert ratio <= 8.0, (label, ratio)


def _check_dot(label, P, V, k, sa, S, n):
    """|P - [Q W]^T W| <= (n + 2) u |V|^T |W| for the k + sa rows; own rows symmetric bit for bit; columns from sa on zero"""
    g, comp = gs_ref.gram(V, k, sa)
    err = np.abs(P[:k + sa, :sa] - g)
    bound = (n + 2) * U * comp
    assert (err <= bound).all(), (label, float(np.max(err / np.where(bound > 0, bound, 1.0))))
    assert np.array_equal(P[k:k + sa, :sa], P[k:k + sa, :sa].T), label
    assert not P[:k + sa, sa:].any(), label


def _check_update(label, Wout, Win, Q, cf, ri, sa, sa_req, k, S, n, canary0):
    """the first sa columns against (Win - Q cf) ri under (k + S + 3) u (|Win| + |Q| |cf|) |ri|; the columns behind them
    untouched (cut block); padding rows and the canary column untouched"""
    ref, comp = gs_ref.update(Q[:n], Win[:n], cf, ri, sa)
    err = np.abs(Wout[:n, :sa] - ref)
    bound = (k + S + 3) * U * comp
    assert (err <= bound).all(), (label, float(np.max(err / np.where(bound > 0, bound, 1.0))))
    assert np.array_equal(Wout[:, sa:sa_req], Win[:, sa:sa_req]), label          # behind a cut: not written
    assert np.array_equal(Wout[n:, :sa_req], Win[n:, :sa_req]), label            # padding rows
    if canary0 is not None:
        assert np.array_equal(Wout[:, sa_req], canary0), label


def _capture(c, op, label, worst, s, restart, block, fuse=-1, own=1, gy=0, chol_tol=CHOL_TOL_DEFAULT, b=None, cut=False):
    """arms `block`, solves, checks that the block meant is the block got and then every piece of it"""
    c.set_option("gmres_kind", 2)
    c.set_option("gmres_tol_blocks", 0)
    c.set_option("gmres_s", s)
    c.set_option("gmres_fuse", fuse)
    c.set_option("gmres_dot_own", own)
    c.set_option("gmres_dot_gy", gy)
    c.set_option("gmres_chol_tol", chol_tol)
    c.gmres_capture_arm(block)
    x, its, rel = c.gmres(b=b, rtol=RTOL, max_it=400, restart=restart, use_prec=False)
    info = c.gmres_capture_info()
    k, sa_req, shifted = _plan(s, restart, block)
    S = 4 if s <= 4 else (8 if s <= 8 else 16)
    fused = 1 if (S == 16 and fuse == 1) else 0
    n = op[0].shape[0] - 1
    assert info["captured"] == 1, (label, its, c.gmres_info())
    assert (info["k"], info["sa_req"], info["S"], info["fused"], info["n"], info["m"]) == (k, sa_req, S, fused, n, restart), (label, info)
    ldv = info["ldv"]
    assert ldv >= n + (n & 1)
    g = {w: c.gmres_capture_get(w) for w in c.CAPTURE_PIECES if not (w == "C0" and k + sa_req > restart)}
    V0, P1, P2, W1, W2, H, VEND, TH = g["V0"], g["P1"], g["P2"], g["W1"], g["W2"], g["H"], g["VEND"], g["TH"]
    H = np.triu(H, -1)          # (below the sub-diagonal the raw array is neither written nor read: stale values)
    sa1, sa2 = int(g["SA1"][0]), int(g["SA2"][0])
    assert g["SA2"][1] == sa2 and 0 <= sa2 <= sa1 <= sa_req, (label, g["SA1"], g["SA2"])
    canary0 = g["C0"][:, 0] if "C0" in g else None
    assert (canary0 is None) == (k + sa_req == restart + 1)
    assert shifted == bool(TH.any()), (label, TH)
    Q, Wraw = V0[:, :k], V0[:, k:]
    # 1. first dot
    _check_dot(label + " P1", P1, V0[:n], k, sa_req, S, n)
    # 2. pass 1 on the device's own products
    assert np.array_equal(g["CF1"], P1[:k]), label
    f1 = gs_ref.pass1(P1, k, sa_req, chol_tol, S)
    l1 = gs_ref.pass1(P1, k, sa_req, chol_tol, S, LD)
    if not _near_threshold(f1["ratios"]):
        assert sa1 == f1["sa"], (label, sa1, f1["sa"], f1["ratios"])
    if cut:
        assert sa1 < sa_req, (label, sa1)                       # (otherwise the cut path was not run)
    if sa1 == f1["sa"] == l1["sa"]:
        _check_ri(label + " RI1", g["RI1"], f1["Ri"], l1["Ri"], S, worst)
    # 3. first update
    _check_update(label + " W1", W1, Wraw, Q, g["CF1"], g["RI1"], sa1, sa_req, k, S, n, canary0)
    if sa1 == 0:
        return info
    # 4. second dot, on [Q W1]  (rows from k + SA1 on are not formed: d_sa limits the sweep)
    _check_dot(label + " P2", P2, np.hstack([Q[:n], W1[:n, :sa1]]), k, sa1, S, n)
    # 5. pass 2 and second update
    f2 = gs_ref.pass2(P2, k, sa1, chol_tol, S, f1, H, TH)
    if not _near_threshold(f2["ratios"]):
        assert sa2 == f2["sa"], (label, sa2, f2["sa"], f2["ratios"])
    if sa2 == 0:
        return info
    assert np.array_equal(g["CF2"], P2[:k]), label
    G2, A2 = gs_ref.gram_minus(P2, k, S, LD)
    l2 = gs_ref.chol_cut(A2, np.diag(G2).copy(), sa1, chol_tol, LD)
    if sa2 == f2["sa"] == l2[0]:
        _check_ri(label + " RI2", g["RI2"], f2["Ri"], l2[2], S, worst)
    _check_update(label + " W2", W2, W1, Q, g["CF2"], g["RI2"], sa2, sa_req, k, S, n, canary0)
    assert np.array_equal(VEND[:, :k], Q) and np.array_equal(VEND[:, k:], W2[:, :sa2]), label
    # 6. the block as a whole against the float64 reference run of the same block from the same V0
    ref = gs_ref.block(V0[:n], k, sa_req, S, chol_tol, H, TH)
    normB = float(np.sqrt((op[2] * op[2]).sum()))
    Hd = H[:k + sa2, :k + sa2 - 1]
    od = gs_ref.orthogonality(VEND[:n])
    ad = gs_ref.arnoldi_residual(lambda X: _apply(op, X), normB, VEND[:n], Hd)
    line = "%s: k %d sa %d/%d/%d  orthogonality %.3e  Arnoldi %.3e" % (label, k, sa_req, sa1, sa2, od, ad)
    if ref["sa"] == sa2:
        orf = gs_ref.orthogonality(ref["V"])
        arf = gs_ref.arnoldi_residual(lambda X: _apply(op, X), normB, ref["V"], ref["H"])
        ro, ra = od / max(orf, 8 * U), ad / max(arf, 8 * U)
        print(line + "  (reference %.3e %.3e: ratios %.2f %.2f)" % (orf, arf, ro, ra))
        worst["orth"], worst["arnoldi"] = max(worst["orth"], ro), max(worst["arnoldi"], ra)
        assert od <= max(8 * orf, 64 * U), (label, od, orf)
        assert ad <= max(8 * arf, 64 * U), (label, ad, arf)
    else:
        print(line + "  (the reference cut at %d: a pivot at the threshold)" % ref["sa"])
    return info


# (s, restart, block, options): every system takes these; restart 21 ends its first cycle with a block that the room cuts
# (s = 5: one column; s = 16 with gmres_fuse 1: five columns through k_blockaxpy<16, true>, no canary column behind it)
CASES = [
    (3, 100, 1, dict(own=1, gy=1)),                      # S 4, sa 3, even k
    (4, 100, 0, dict(own=0, gy=3)),                      # S 4 full, the first block (k 1)
    (5, 100, 1, dict(own=1, gy=3)),                      # S 8, sa 5, even k
    (8, 100, 1, dict(own=0, gy=1)),                      # S 8 full
    (16, 100, 0, dict(fuse=1, own=1, gy=1)),             # S 16, sa 8, k 1, fused
    (16, 100, 2, dict(fuse=1, own=1, gy=3)),             # Newton-shifted 16-block, fused
    (16, 100, 2, dict(fuse=1, own=0, gy=1)),             # ... its own columns read back
    (16, 100, 2, dict(fuse=0, own=1, gy=1)),             # ... two kernels
    (16, 100, 2, dict(fuse=0, own=0, gy=3)),
    (5, 21, 4, dict(own=1, gy=1)),                       # sa_req 1 by the room
    (16, 21, 2, dict(fuse=1, own=1, gy=3)),              # sa_req 5 by the room, the combining update
    (16, 21, 2, dict(fuse=0, own=0, gy=1)),
    (8, 100, 0, dict(own=1, gy=1, chol_tol=0.5, cut=True)),
    (16, 100, 0, dict(fuse=1, own=1, gy=3, chol_tol=0.5, cut=True)),
]
# 4913 rows: blocks at k = 49 and k = 65 -- more than 32 column groups of two, the mid-loop flush of both kernels
CASES_FLUSH = [
    (16, 100, 4, dict(fuse=1, own=1, gy=1)),
    (16, 100, 4, dict(fuse=0, own=1, gy=1)),
    (16, 100, 4, dict(fuse=0, own=0, gy=1)),
    (16, 100, 5, dict(fuse=1, own=0, gy=1)),
    (16, 100, 5, dict(fuse=0, own=1, gy=3)),
]


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_block_stage_by_stage(fedd_lib, name):
    L = fedd_lib
    dim, M, rows = SYSTEMS[name]
    c = L.Context(device=0)
    worst = {"ri": 0.0, "orth": 0.0, "arnoldi": 0.0}
    try:
        b, op = _system(L, c, dim, M)
        assert op[0].shape[0] - 1 == rows
        for s, restart, block, opt in CASES + (CASES_FLUSH if name == "3d16" else []):
            label = "%s s %d restart %d block %d %s" % (name, s, restart, block, opt)
            info = _capture(c, op, label, worst, s, restart, block, b=b, **opt)
            if (s, restart, block) in ((16, 100, 4), (16, 100, 5)):
                assert info["k"] >= 49 and info["k"] + info["sa_req"] >= 65, info
        print("%s: largest ratios  RI %.3f (bound 8)  orthogonality %.2f  Arnoldi %.2f (bound 8)"
              % (name, worst["ri"], worst["orth"], worst["arnoldi"]))
    finally:
        _restore(c)
        c.close()


def test_armed_solve_is_the_unarmed_solve(fedd_lib):
    """x, iterations, relres and gmres_info of an armed and an unarmed solve, bit for bit (4913 rows, fused and not)"""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        b, _ = _system(L, c, 3, 16)
        c.set_option("gmres_kind", 2)
        c.set_option("gmres_tol_blocks", 0)
        c.set_option("gmres_s", 16)
        for fuse in (0, 1):
            c.set_option("gmres_fuse", fuse)
            out = []
            for block in (-1, 3):
                c.gmres_capture_arm(block)
                x, its, rel = c.gmres(b=b, rtol=RTOL, max_it=400, restart=100, use_prec=False)
                out.append((x, its, rel, c.gmres_info(), c.gmres_status()))
                assert c.gmres_capture_info()["captured"] == (1 if block >= 0 else 0)
            assert out[0][1:] == out[1][1:], (out[0][1:], out[1][1:])
            assert np.array_equal(out[0][0], out[1][0])
            # the arm was consumed: the next solve copies nothing new
            c.gmres(b=b, rtol=RTOL, max_it=400, restart=100, use_prec=False, want_x=False)
            assert c.gmres_capture_info()["k"] == 33
    finally:
        _restore(c)
        c.close()


def test_capture_errors_by_message(fedd_lib):
    L = fedd_lib
    c = L.Context(device=0)
    try:
        b, _ = _system(L, c, 3, 7)
        with pytest.raises(L.FeddError, match="nothing captured"):
            c.gmres_capture_get("P1")
        c.set_option("gmres_tol_blocks", 0)
        c.set_option("gmres_s", 5)
        c.gmres_capture_arm(10 ** 6)                            # a block the solve never reaches
        c.gmres(b=b, rtol=RTOL, max_it=400, restart=21, use_prec=False)
        with pytest.raises(L.FeddError, match="nothing captured"):
            c.gmres_capture_get("P1")
        c.gmres_capture_arm(4)                                  # k 21, one column, the last of the basis: no canary
        c.gmres(b=b, rtol=RTOL, max_it=400, restart=21, use_prec=False)
        assert c.gmres_capture_info()["captured"] == 1
        with pytest.raises(L.FeddError, match="'C0' was not captured"):
            c.gmres_capture_get("C0")
        with pytest.raises(L.FeddError, match="'P1' has 176 values, the buffer holds 175"):
            c.gmres_capture_get("P1", cap=175)
        for kind in (0, 1):
            c.set_option("gmres_kind", kind)
            c.gmres_capture_arm(0)
            with pytest.raises(L.FeddError, match="gmres capture: the s-step solver only"):
                c.gmres(b=b, rtol=RTOL, max_it=400, restart=21, use_prec=False)
        c.set_option("gmres_kind", 2)
        c.gmres(b=b, rtol=RTOL, max_it=400, restart=21, use_prec=False)      # (the refused solves consumed their arms)
        assert c.gmres_capture_info()["captured"] == 0
    finally:
        _restore(c)
        c.close()
    h = L.Context(device=-1, rank=1, nranks=2, nccl_id=None)
    try:
        with pytest.raises(L.FeddError, match="fedd_gmres_capture_arm: one rank only"):
            h.gmres_capture_arm(0)
    finally:
        h.close()

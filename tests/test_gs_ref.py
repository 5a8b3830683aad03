"""tests/gs_ref.py, the plain reference of the s-step Gram-Schmidt block, checked on its own (CPU): the longdouble products
against np.dot, one pass against the orthogonality it must produce, and whole blocks -- shifts, short last block, a cut --
against the Arnoldi relation of a small dense operator."""
from fractions import Fraction

import numpy as np
import pytest

import gs_ref

pytestmark = pytest.mark.skipif(not gs_ref.HAVE_LONGDOUBLE, reason="np.longdouble has no 64-bit significand here")
U = gs_ref.U


def _basis(n, k, sa, seed):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, k)))[0]
    W = rng.standard_normal((n, sa)) + Q @ rng.standard_normal((k, sa))
    return np.hstack([Q, W])


def test_fma_rounds_once():
    rng = np.random.default_rng(1)
    for a, b, c in rng.standard_normal((200, 3)):
        c = -a * b + c * 1e-17          # (cancellation: two roundings would lose the low part of the product)
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        assert gs_ref.fma(a, b, c) == float(exact)


def test_gram_equals_dot_to_rounding():
    n, k, sa = 777, 6, 5
    V0 = _basis(n, k, sa, 2)
    g, comp = gs_ref.gram(V0, k, sa)
    assert g.dtype == np.longdouble and g.shape == (k + sa, sa)
    err = np.abs(g - V0.T @ V0[:, k:])
    assert (err <= (n + 2) * U * comp).all(), float((err / comp).max() / U)
    assert (comp >= np.abs(g)).all()
    assert np.array_equal(g[k:], g[k:].T)


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_one_pass_orthogonalises(dtype):
    n, k, sa, S = 500, 7, 4, 4
    V0 = _basis(n, k, sa, 3)
    g, _ = gs_ref.gram(V0, k, sa)
    P = np.asarray(g, dtype=np.float64)
    p1 = gs_ref.pass1(P, k, sa, 1e-13, S, dtype)
    assert p1["sa"] == sa and len(p1["ratios"]) == sa and min(p1["ratios"]) > 1e6
    assert np.array_equal(np.asarray(p1["cf"], dtype=np.float64), P[:k])
    R, Ri = np.asarray(p1["R"], np.float64), np.asarray(p1["Ri"], np.float64)
    assert np.abs(R @ Ri - np.eye(S)).max() < 1e-13 and np.array_equal(R, np.triu(R))
    W1, comp = gs_ref.update(V0[:, :k], V0[:, k:], p1["cf"], p1["Ri"], sa)
    assert (comp >= np.abs(W1)).all()
    # the Pythagorean pass loses u * cond(W)^2 (Carson et al. 2022); cond of this W is below 10
    assert float(np.abs(V0[:, :k].T @ W1).max()) < 1e-13
    assert float(np.abs(W1.T @ W1 - np.eye(sa)).max()) < 1e-13


def test_float64_and_longdouble_restatements_agree():
    n, k, sa, S = 300, 9, 7, 8
    V0 = _basis(n, k, sa, 4)
    P = np.zeros((k + sa, S))
    P[:, :sa] = np.asarray(gs_ref.gram(V0, k, sa)[0], dtype=np.float64)
    a, b = gs_ref.pass1(P, k, sa, 1e-13, S), gs_ref.pass1(P, k, sa, 1e-13, S, np.longdouble)
    assert a["sa"] == b["sa"] == sa
    d = np.abs(a["Ri"] - b["Ri"]).max()
    assert 0 < d < 1e-13                        # they differ (rounding) and only by rounding
    assert not a["Ri"][sa:].any() and not a["Ri"][:, sa:].any()


def test_dependent_column_is_cut():
    n, k, sa, S = 200, 3, 4, 4
    V0 = _basis(n, k, sa, 5)
    V0[:, k + 2] = V0[:, k] + 1e-9 * V0[:, k + 2]          # squared sine ~ 1e-18 < 1e-13
    P = np.asarray(gs_ref.gram(V0, k, sa)[0], dtype=np.float64)
    p1 = gs_ref.pass1(P, k, sa, 1e-13, S)
    assert p1["sa"] == 2 and p1["ratios"][-1] < 1
    assert not p1["Ri"][:, 2:].any() and not p1["R"][:, 2:].any()


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("s,S,shifted", [(3, 4, False), (5, 8, True), (8, 8, False)])
def test_blocks_satisfy_the_arnoldi_relation(dtype, s, S, shifted):
    """m = 13 steps of blocks of s (the last one shorter) on a dense nonsymmetric operator: V^T V = I and
    B V_j = V_{j+1} H to rounding times the condition of the block bases (monomial s = 8 on this spectrum: below 1e6)"""
    n, m = 60, 13
    rng = np.random.default_rng(6)
    B = np.diag(np.linspace(1.0, 3.0, n)) + 0.2 * rng.standard_normal((n, n)) / np.sqrt(n)
    th = np.zeros(S)
    if shifted:
        th[:s] = [2.9, 1.1, 2.0, 1.5, 2.5]
    V = np.zeros((n, m + 1))
    r0 = rng.standard_normal(n)
    V[:, 0] = r0 / np.linalg.norm(r0)
    H = np.zeros((m + 1, m))
    k = 1
    while k - 1 < m:
        sa = min(s, m - (k - 1))
        for i in range(sa):
            V[:, k + i] = B @ V[:, k - 1 + i] - th[i] * V[:, k - 1 + i]
        out = gs_ref.block(V, k, sa, S, 1e-13, H, th, dtype)
        assert out["sa1"] == sa and out["sa"] == sa
        V[:, :k + sa] = np.asarray(out["V"], dtype=np.float64)
        H[:k + sa, :k + sa - 1] = np.asarray(out["H"], dtype=np.float64)
        k += sa
    assert np.array_equal(H, np.triu(H, -1))
    assert gs_ref.orthogonality(V) < 1e-10
    res = gs_ref.arnoldi_residual(lambda X: np.asarray(B, dtype=np.longdouble) @ X, np.linalg.norm(B), V, H)
    assert res < 1e-10, res
    # and it is the Arnoldi factorisation: the same H (up to signs: none, R has a positive diagonal) as modified Gram-Schmidt
    Vm = np.zeros_like(V)
    Vm[:, 0] = V[:, 0]
    Hm = np.zeros_like(H)
    for j in range(m):
        w = B @ Vm[:, j]
        for i in range(j + 1):
            Hm[i, j] = Vm[:, i] @ w
            w = w - Hm[i, j] * Vm[:, i]
        Hm[j + 1, j] = np.linalg.norm(w)
        Vm[:, j + 1] = w / Hm[j + 1, j]
    assert np.abs(H - Hm).max() < 1e-7 * np.abs(Hm).max()

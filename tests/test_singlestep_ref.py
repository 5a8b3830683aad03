"""tests/singlestep_ref.py checked on its own, and feddlib_amd.capi.butcher_table: the stage loop on a small linear system
M u' + K u = 0 against the matrix exponential.  Observed order under step halving: 1 for table 0 (implicit Euler), 2 for table 1
(Crank-Nicolson), at least 2 for tables 2 to 4 (TimeSteppingTools.cpp:353-454 gives convOrder_ 2, 2 and 3).

Tables 2 and 4 reach their orders only with the entries butcher_table corrects (its docstring says which and why); the values
test below measures order 1 for both with the reference's entries put back."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import singlestep_ref as ssr


def _system():
    rng = np.random.default_rng(5)
    n = 6
    Q = rng.standard_normal((n, n))
    M = np.eye(n) + 0.1 * (Q @ Q.T) / n
    K = np.diag(np.linspace(0.5, 3.0, n)) + 0.2 * (Q + Q.T) / 2 + 0.3 * (Q - Q.T) / 2      # not symmetric, eigenvalues in the right half plane
    u0 = rng.standard_normal(n)
    return M, K, u0


def _error(number, dt, fedd_lib, T=1.0):
    M, K, u0 = _system()
    c, A = fedd_lib.butcher_table(number)
    Ks = sp.csr_matrix(K)
    ref = ssr.SingleStep(sp.csr_matrix(M), lambda u: Ks)
    x = ref.run(u0, dt, A, int(round(T / dt)))
    exact = sla.expm(-T * np.linalg.solve(M, K)) @ u0
    return float(np.linalg.norm(x - exact))


@pytest.mark.parametrize("number", [0, 1, 2, 3, 4])
def test_observed_order_under_step_halving(fedd_lib, number):
    e1, e2 = _error(number, 0.05, fedd_lib), _error(number, 0.025, fedd_lib)
    p = np.log2(e1 / e2)
    print("table %d: errors %.3e %.3e, observed order %.3f" % (number, e1, e2, p))
    assert e2 > 1e-11          # above the rounding floor: the ratio is an order
    if number == 0:
        assert abs(p - 1.0) < 0.1
    elif number == 1:
        assert abs(p - 2.0) < 0.1
    else:
        assert p > 1.9


@pytest.mark.parametrize("number", [0, 1, 2, 3, 4])
def test_tables_are_stiffly_accurate_with_a_dummy_first_stage(fedd_lib, number):
    c, A = fedd_lib.butcher_table(number)
    S = A.shape[0]
    assert A.shape == (S, S) and c.shape == (S,)
    assert A[0, 0] == 0.0 and not A[0].any() and c[0] == 0.0
    assert not np.triu(A, 1).any()                                   # diagonally implicit
    assert all(A[s, s] > 0.0 for s in range(1, S))
    # stiffly accurate: the weights b are the last row of A, so that row is a quadrature of the step: it sums to 1 and ends at c = 1
    b = A[-1]
    assert c[-1] == 1.0 and abs(b.sum() - 1.0) <= 4 * np.finfo(float).eps
    # row sums: c_s = sum_j a_sj
    assert np.abs(A.sum(axis=1) - c).max() <= 4 * np.finfo(float).eps
    assert S == {0: 2, 1: 2, 2: 4, 3: 3, 4: 4}[number]


def test_table_values_in_the_reference_order(fedd_lib):
    th = 1.0 - np.sqrt(2.0) / 2.0
    tt = 1.0 - 2.0 * th
    al = tt / (1.0 - th)
    be = 1.0 - al
    c, A = fedd_lib.butcher_table(2)
    assert c[1] == th and c[2] == th + tt
    assert A[1, 0] == th * be and A[1, 1] == th * al and A[2, 2] == tt * be and A[3, 2] == (th + tt) * be and A[3, 3] == th * al
    # a_22 = Theta_t * beta, not the Theta_t * alpha of TimeSteppingTools.cpp:369: with that entry row 2 misses c_2 and the
    # scheme is of order 1 on the system of this file
    assert abs(A[2].sum() - c[2]) <= 4 * np.finfo(float).eps and abs(th * be + (th + tt) * al + tt * al - c[2]) > 0.05
    B = A.copy()
    B[2, 2] = tt * al
    M, K, u0 = _system()
    errs = []
    for dt in (0.05, 0.025):
        x = ssr.SingleStep(sp.csr_matrix(M), lambda u: sp.csr_matrix(K)).run(u0, dt, B, int(round(1.0 / dt)))
        errs.append(float(np.linalg.norm(x - sla.expm(-np.linalg.solve(M, K)) @ u0)))
    assert abs(np.log2(errs[0] / errs[1]) - 1.0) < 0.15
    # table 4: alpha is the smallest root of x^3 - 3 x^2 + (3/2) x - 1/6 and the last row meets the third-order conditions;
    # with the constants of TimeSteppingTools.cpp:426, 429 (a digit doubled in alpha and in sigma) the order is 1
    c, A = fedd_lib.butcher_table(4)
    al = A[1, 1]
    assert abs(al ** 3 - 3.0 * al ** 2 + 1.5 * al - 1.0 / 6.0) < 1e-14 and al < 0.2
    b = A[-1]
    assert abs(b @ c - 0.5) < 1e-14 and abs(b @ c ** 2 - 1.0 / 3.0) < 1e-14 and abs(b @ (A @ c) - 1.0 / 6.0) < 1e-14
    al, be, ga, si = 0.1558983899988677, 1.072486270734370, 0.7685298292769537, 0.09666483609791597
    B = np.array([[0.0, 0.0, 0.0, 0.0], [al, al, 0.0, 0.0], [1.0 - be - al, be, al, 0.0], [1.0 - ga - si - al, ga, si, al]])
    assert abs(B[-1] @ B.sum(axis=1) - 0.5) > 5e-3
    errs = []
    for dt in (0.05, 0.025):
        x = ssr.SingleStep(sp.csr_matrix(M), lambda u: sp.csr_matrix(K)).run(u0, dt, B, int(round(1.0 / dt)))
        errs.append(float(np.linalg.norm(x - sla.expm(-np.linalg.solve(M, K)) @ u0)))
    assert abs(np.log2(errs[0] / errs[1]) - 1.0) < 0.15
    c, A = fedd_lib.butcher_table(1)
    assert A.tolist() == [[0.0, 0.0], [0.5, 0.5]]
    c, A = fedd_lib.butcher_table(3)
    assert A[1, 1] == th and A[2, 1] == 1.0 / (4.0 * (1.0 - th)) and A[2, 0] == 1.0 - A[2, 1] - th
    for bad in (-1, 5, 17):
        with pytest.raises(ValueError, match="tables 0 .. 4"):
            fedd_lib.butcher_table(bad)


def test_stage_rhs_is_the_stated_combination():
    rng = np.random.default_rng(2)
    n_m, n_p = 5, 3
    M = sp.csr_matrix(rng.standard_normal((n_m, n_m)))
    BT = sp.csr_matrix(rng.standard_normal((n_m, n_p)))
    Fs = [sp.csr_matrix(rng.standard_normal((n_m, n_m))) for _ in range(3)]
    Us = [rng.standard_normal(n_m + n_p) for _ in range(3)]
    cf, cbt = np.array([-0.1, -0.2, -0.3]), np.array([-0.1, 0.0, -0.3])
    b = ssr.stage_rhs(M, BT, Fs, Us, cf, cbt)
    want = M @ Us[0][:n_m] + sum(cf[j] * (Fs[j] @ Us[j][:n_m]) + cbt[j] * (BT @ Us[j][n_m:]) for j in range(3))
    np.testing.assert_allclose(b[:n_m], want, rtol=1e-13)
    assert not b[n_m:].any()
    cf, cbt, das, s_bt = ssr.stage_coefficients(np.array([[0.0, 0.0], [0.5, 0.5]]), 1, 0.1, True)
    assert cf.tolist() == [-0.05] and cbt.tolist() == [0.0] and das == 0.05 and s_bt == 0.1
    cf, cbt, das, s_bt = ssr.stage_coefficients(np.array([[0.0, 0.0], [0.5, 0.5]]), 1, 0.1, False)
    assert cbt.tolist() == [-0.05] and s_bt == 0.05

"""The stage loop of the reference's "Class" = "Singlestep" time stepping restated with numpy / scipy on given matrices
(DAESolverInTime::advanceInTimeNonLinear, DAESolverInTime_def.hpp:384-516; buildMultiStageRhs with BlockMatrix::apply,
BlockMatrix_def.hpp:371-392), for diagonally implicit, stiffly accurate tables with a dummy first stage (a_00 = 0):

    stage 0             F_0 = F(u_n), U_0 = [u_n ; p_n] are kept
    stage s = 1..S-1    rhs = [M u_0 ; 0] + sum_{j < s} [c_j (F_j u_j) + cbt_j (B^T p_j) ; 0],   c_j = -(dt a_sj),
                        cbt_j = c_j, or 0 under "Full implicit pressure"
                        solve  [(1.0 M) + (dt a_ss) F(u), s_bt B^T ; B, C] U = rhs,   s_bt = dt a_ss, or dt under full implicit pressure
                        keep F_s = F(u_s), U_s unless s is the last stage; the last stage's solution is the step's result

F(u) is the velocity block of the problem: a callable u -> sparse matrix (A + rho N(u) for Navier-Stokes; a constant K for a
linear problem, where the fixed-point iteration ends after one solve).  Dirichlet rows carry unit rows and given values."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def stage_coefficients(A, s, dt, full_implicit_pressure):
    """(coeff_f, coeff_bt, dt * a_ss, s_bt) of stage s"""
    cf = np.array([-(dt * A[s, j]) for j in range(s)])
    cbt = np.zeros(s) if full_implicit_pressure else cf.copy()
    das = dt * A[s, s]
    return cf, cbt, das, (dt if full_implicit_pressure else das)


def stage_rhs(M, BT, Fs, Us, cf, cbt):
    """buildMultiStageRhs in the reference's order: M u_0, then stage by stage (c_j (F_j u_j)) + (cbt_j (B^T p_j))"""
    n_m = M.shape[0]
    t = M @ Us[0][:n_m]
    for j in range(len(cf)):
        mv = cf[j] * (Fs[j] @ Us[j][:n_m])
        if cbt[j] != 0.0:
            mv = mv + cbt[j] * (BT @ Us[j][n_m:])
        t = t + mv
    return np.concatenate([t, np.zeros(Us[0].shape[0] - n_m)])


class SingleStep:
    """M: velocity mass matrix; F: u -> velocity block; BT, B (and C): the pressure blocks, None for a problem without pressure;
    rows / vals: Dirichlet rows of the whole system and their values."""

    def __init__(self, M, F, BT=None, B=None, C=None, rows=(), vals=(), full_implicit_pressure=True, nl_tol=1e-13, nl_max=60):
        self.M, self.F = sp.csr_matrix(M), F
        self.n_m = self.M.shape[0]
        self.n_p = 0 if B is None else B.shape[0]
        self.n = self.n_m + self.n_p
        self.BT = sp.csr_matrix((self.n_m, 0)) if BT is None else sp.csr_matrix(BT)
        self.B, self.C = B, C
        self.rows, self.vals = np.asarray(rows, dtype=np.int64), np.asarray(vals, dtype=np.float64)
        self.free = np.ones(self.n, dtype=bool)
        self.free[self.rows] = False
        self.fip = full_implicit_pressure
        self.nl_tol, self.nl_max = nl_tol, nl_max
        self.iterations = []

    def system(self, u, das, s_bt):
        V = self.M + das * self.F(u)
        if self.n_p == 0:
            return sp.csr_matrix(V)
        return sp.bmat([[V, s_bt * self.BT], [self.B, self.C]], format="csr")

    def residual(self, x, das, s_bt, b):
        r = self.system(x[:self.n_m], das, s_bt) @ x - b
        r[self.rows] = 0.0
        return r

    def solve_stage(self, x0, das, s_bt, b):
        """fixed point: the system at the iterate, solved for the new iterate, until the residual stops falling"""
        x = x0.copy()
        x[self.rows] = self.vals
        hist = []
        for k in range(self.nl_max):
            K = self.system(x[:self.n_m], das, s_bt).tocsc()
            r = K @ x - b
            r[self.rows] = 0.0
            hist.append(float(np.linalg.norm(r)))
            if k > 0 and (hist[-1] <= self.nl_tol * max(hist[0], 1e-300) or hist[-1] == 0.0 or (k > 3 and hist[-1] >= 0.5 * hist[-2])):
                break
            dx = np.zeros(self.n)
            dx[self.free] = spla.splu(K[self.free][:, self.free].tocsc()).solve(-r[self.free])
            x += dx
        self.iterations.append(len(hist) - 1)
        return x, hist

    def step(self, x_n, dt, A):
        """one step with the table A (S x S); returns (x_{n+1}, the stage operators kept, the stage solutions kept)"""
        S = A.shape[0]
        assert A[0, 0] == 0.0
        Fs, Us = [sp.csr_matrix(self.F(x_n[:self.n_m]))], [x_n.copy()]
        x = x_n
        for s in range(1, S):
            cf, cbt, das, s_bt = stage_coefficients(A, s, dt, self.fip)
            b = stage_rhs(self.M, self.BT, Fs, Us, cf, cbt)
            x, _ = self.solve_stage(x, das, s_bt, b)
            if s + 1 < S:
                Fs.append(sp.csr_matrix(self.F(x[:self.n_m])))
                Us.append(x.copy())
        return x, Fs, Us

    def run(self, x0, dt, A, n_steps):
        x = np.array(x0, dtype=np.float64)
        for _ in range(n_steps):
            x = self.step(x, dt, A)[0]
        return x

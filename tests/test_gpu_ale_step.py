"""Unsteady Navier-Stokes on a breathing mesh at the ABI level: three BDF steps (a BDF1 start, then BDF2) of P2 / P1 on the
4 x 4-cell structured square (vertices first), the mesh moved by d(t) = a sin(omega t) b(x) with b = 0 on the boundary.  Per step
the device runs

    fedd_mesh_move(d_k), fedd_mesh_velocity_diff(d_k, d_{k-1}, dt)
    A, B, B^T, M on the moved mesh                          slots 0, 1, 2, 5
    slot 6 <- (cm * M[5]) + (1.0 * A[0])                    fedd_matrix_combine + fedd_matrix_store
    history, b <- [M t ; 0]                                 fedd_solution_set + fedd_multistep_advance
    N_IT fixed-point iterations                             fedd_velocity_set, fedd_assemble_advection_ale(FEDD_ALE_FIXEDPOINT,
                                                            rho, slot_add = 6, slot_out = 4), fedd_block_merge, Dirichlet rows,
                                                            GMRES on K(x_j) x_{j+1} = b

Reference: the same sequence on the host with oracle matrices of the moved mesh, the restated ALE block (tests/ale_ref.py) and a
sparse direct solve per iteration.

Bar.  That of tests/test_gpu_time_navier_stokes.py with its linear tolerance: ||x - x_ref|| <= 1.05 ||K^-1||_2 (||r(x)|| +
||r(x_ref)||).  The iterations are a fixed number, so what is solved is the LINEAR system of each iteration and the bracket is
taken for it: the reference of iteration j starts from the iterate the device returned (as the reference of a step starts from
the device's earlier states there), K = K(x_j) is the host's matrix of that system on the free rows, ||K^-1||_2 comes from its
sparse factors, r(x) = K x - b is formed on the host for both sides, and e = K^-1 (r(x) - r(x_ref)) exactly.  The device side
is driven to ||r_dev|| <= TOL * r_0 by its own residual (fedd_spmv of the merged matrix minus the right-hand side), r_0 the
steady residual of the start state as there.

The input exposes a missing ALE term: the same iteration with w left out (N(u) in the place of N(u - w) - P(w)) lands far
outside the bar, asserted in every iteration."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import fedd_oracle as fo
from ale_ref import AleRestatement
from test_gpu_parity import oracle_mesh
from test_gpu_time_navier_stokes import BDF, RTOL_LIN, TOL, profile

pytestmark = pytest.mark.gpu

SLOT_A, SLOT_B, SLOT_BT, SLOT_F, SLOT_M, SLOT_AT = 0, 1, 2, 4, 5, 6
NU, RHO, DT, N_IT = 0.01, 1.0, 0.05, 3
AMP, OMEGA = 0.03, 9.0


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def meshes(lib):
    """P2 velocity mesh with the P1 lattice nodes first and the P1 pressure mesh on them; one rank, so the global ids are
    labels: the local numbering serves as such on both sides"""
    mv = dict(lib.structured_mesh_p2(2, 1, 4, vertices_first=True))
    m1 = lib.structured_mesh(2, 1, 4)
    n = mv["xyz"].shape[0]
    mv["gid_rep"] = np.arange(n, dtype=mv["gid_rep"].dtype)
    mv["gid_uni"] = mv["gid_rep"].copy()
    assert np.array_equal(mv["xyz"][:mv["n_p1"]], m1["xyz"]) and np.array_equal(mv["conn"][:, :3], m1["conn"])
    return m1, mv


def breathing(x, t):
    """a sin(omega t) b(x): b smooth, zero on the boundary of the unit square, not symmetric"""
    b = np.sin(np.pi * x[:, 0]) * np.sin(np.pi * x[:, 1])
    d = AMP * np.sin(OMEGA * t) * np.stack([b * (0.6 + x[:, 1]), b * np.cos(1.3 * x[:, 0])], axis=1)
    d[np.any((x == 0.0) | (x == 1.0), axis=1)] = 0.0
    return d


def boundary(mv):
    """inflow profile(y) on x = 0, no-slip walls y = 0, 1, natural outflow on x = 1 (the channel of the fixed-mesh tests)"""
    X = mv["xyz"]
    inflow = X[:, 0] < 1e-12
    wall = (X[:, 1] < 1e-12) | (X[:, 1] > 1 - 1e-12)
    nodes = np.nonzero(inflow | wall)[0]
    rows = (2 * nodes[:, None] + np.arange(2)[None, :]).ravel()
    vals = np.zeros((nodes.shape[0], 2))
    sel = inflow[nodes] & ~wall[nodes]
    vals[sel, 0] = profile(X[nodes, 1])[sel]
    return rows, vals.ravel()


def coefficients(step):
    cm, hist = BDF[1 if step == 0 else 2]
    return cm / DT, [h / DT for h in hist]


class Host:
    """one time level on the host: oracle matrices of the moved mesh, restated ALE block"""

    def __init__(self, lib, m1, mv, d, w, rows, vals):
        mvk, m1k = dict(mv), dict(m1)
        mvk["xyz"] = mv["xyz"] + d
        m1k["xyz"] = mvk["xyz"][:mv["n_p1"]].copy()
        self.R = AleRestatement(lib, mvk)
        self.A, self.BT, self.B = fo.stokes_blocks(oracle_mesh(mvk), oracle_mesh(m1k), RHO * NU)
        self.M = (RHO * fo.assembly_mass(oracle_mesh(mvk), "Vector")).tocsr()
        self.nvd, self.n_p = self.A.shape[0], self.B.shape[0]
        self.n = self.nvd + self.n_p
        self.w, self.rows, self.vals = w.ravel(), rows, vals
        self.free = np.ones(self.n, dtype=bool)
        self.free[rows] = False

    def K(self, x, cm, with_w=True):
        u = x[:self.nvd]
        E = self.R.ale("FixedPoint", u, self.w) if with_w else self.R.N(u)
        return sp.bmat([[cm * self.M + self.A + RHO * E, self.BT], [self.B, None]], format="csc")

    def rhs(self, step, states):
        t = sum(ci * xi[:self.nvd] for ci, xi in zip(coefficients(step)[1], states))
        return np.concatenate([self.M @ t, np.zeros(self.n_p)])

    def iterate(self, x, cm, b, with_w=True):
        """(x_next, ||r(x_next)||, ||K^-1||_2, K) of K(x) x_next = b with the Dirichlet values on their rows"""
        K = self.K(x, cm, with_w)
        y = np.zeros(self.n)
        y[self.rows] = self.vals
        Kff = K[self.free][:, self.free].tocsc()
        lu = spla.splu(Kff)
        y[self.free] = lu.solve((b - K @ y)[self.free])
        r = (K @ y - b)[self.free]
        z = np.random.default_rng(3).standard_normal(int(self.free.sum()))
        est = 0.0
        for it in range(200):                       # power iteration on K^-T K^-1, as Host.jinv of the fixed-mesh test
            z /= np.linalg.norm(z)
            v = lu.solve(z)
            new = float(np.linalg.norm(v))
            z = lu.solve(v, trans="T")
            if it > 5 and abs(new - est) <= 0.01 * new:
                est = new
                break
            est = new
        return y, float(np.linalg.norm(r)), est, K


def test_three_bdf_steps_on_a_breathing_mesh(fedd_lib, ctx):
    lib = fedd_lib
    m1, mv = meshes(lib)
    rows, vals = boundary(mv)
    dim, nv, n_p = 2, mv["xyz"].shape[0], m1["xyz"].shape[0]
    n = dim * nv + n_p
    x_start = np.zeros(n)
    x_start[rows] = vals
    ctx.mesh_set_dict(mv)
    states, began, r0 = [x_start], False, None
    d_old = breathing(mv["xyz"], 0.0)
    for step in range(3):
        d = breathing(mv["xyz"], (step + 1) * DT)
        ctx.mesh_move(d)
        assert ctx.mesh_move_info()["min_det_ratio"] > 0.5
        ctx.mesh_velocity_diff(d, d_old, DT)
        w = (d - d_old) * (1.0 / DT)
        assert np.array_equal(ctx.mesh_velocity(), w)
        H = Host(lib, m1, mv, d, w, rows, vals)
        if r0 is None:
            r0 = float(np.linalg.norm((H.K(x_start, 0.0, with_w=False) @ x_start)[H.free]))
        stop = TOL * r0
        # the constant blocks and the mass matrix on the moved mesh
        ctx.pattern_build(dim, lib.BLOCK_DIAG)
        ctx.assemble(lib.FORM_LAPLACE_VEC)
        ctx.matrix_scale(-1, RHO * NU)
        ctx.matrix_store(SLOT_A)
        ctx.assemble_div(n_p, SLOT_B, SLOT_BT)
        ctx.matrix_scale(SLOT_B, -1.0)
        ctx.matrix_scale(SLOT_BT, -1.0)
        ctx.pattern_build(dim, lib.BLOCK_DIAG)
        ctx.assemble(lib.FORM_MASS_VEC)
        ctx.matrix_scale(-1, RHO)
        ctx.matrix_store(SLOT_M)
        cm, coeff = coefficients(step)
        assert not ctx.matrix_combine_current(SLOT_M, cm, SLOT_A, 1.0)       # new coordinates: nothing of the last step stands
        ctx.matrix_combine(SLOT_M, cm, SLOT_A, 1.0)
        ctx.matrix_store(SLOT_AT)
        x = states[0].copy()

        def system(z):
            ctx.velocity_set(z[:dim * nv])
            ctx.assemble_advection_ale(lib.ALE_FIXEDPOINT, RHO, SLOT_AT, SLOT_F)
            ctx.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)

        system(x)                                   # the merged system the history is as long as
        if not began:
            ctx.multistep_begin(2)
            began = True
        ctx.solution_set(x)
        ctx.multistep_advance(SLOT_M, coeff)
        b = ctx.rhs_get()
        bh = H.rhs(step, states)
        assert np.abs(b - bh).max() <= 1e-12 * np.abs(bh).max()
        for j in range(N_IT):
            if j > 0:
                system(x)
            ctx.rhs_set(b)
            ctx.dirichlet_rows(rows, vals)
            y, its, rel = ctx.gmres(None, rtol=RTOL_LIN, max_it=4 * n, restart=min(n, 600), use_prec=False)
            r_dev = ctx.spmv(y) - ctx.rhs_get()
            xr, rr, kinv, K = H.iterate(x, cm, b)
            rx = float(np.linalg.norm((K @ y - b)[H.free]))
            bound = 1.05 * kinv * (stop + rr)
            err = float(np.linalg.norm(y - xr))
            x_now = H.iterate(x, cm, b, with_w=False)[0]
            miss = float(np.linalg.norm(x_now - xr))
            print("step %d iteration %d: GMRES %d its, ||r_dev|| %.2e (stop %.2e), host residual of the device iterate %.2e, "
                  "||x - x_ref|| %.3e bound %.3e (||K^-1|| %.2e, ||r(x_ref)|| %.2e); without w %.3e"
                  % (step + 1, j + 1, its, np.linalg.norm(r_dev), stop, rx, err, bound, kinv, rr, miss))
            assert np.linalg.norm(r_dev) <= stop
            assert err <= bound
            assert miss > 1e3 * bound                # a missing ALE term would show
            x = y
        states = [x] + states[:1]
        d_old = d

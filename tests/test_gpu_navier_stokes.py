"""Advection matrices of steady Navier-Stokes on the GPU (fedd_velocity_set, fedd_assemble_advection) against the numpy
restatement of tests/test_navier_stokes_abi.py, and the nonlinear iterations they feed, run at the ABI level: assembly, merge
(values only from the second iteration on), Dirichlet rows and GMRES on the device, the loop itself on the host."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import fedd_oracle as fo
from test_gpu_distorted import check_mesh, distorted
from test_gpu_parity import assert_matrix_close, oracle_mesh
from test_navier_stokes_abi import GOLD, Restatement, degrees, p2_meshes, smooth_velocity

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def _mesh(fedd_lib, which):
    if which in ("square_p2", "cylinder_p2"):
        return p2_meshes(fedd_lib)[which]
    if which == "cube_p1":
        return fedd_lib.structured_mesh(3, 1, 6)
    if which == "square_p1":
        return fedd_lib.structured_mesh(2, 1, 9)
    if which == "distorted_p1":
        m = distorted(fedd_lib.structured_mesh(3, 1, 7), 0.15, "all", seed=3)
        check_mesh(m, 0.8)
        return m
    m = distorted(fedd_lib.structured_mesh(2, 1, 8), 0.15, "all", seed=4)       # distorted_p2: the P2 mesh of a distorted lattice
    check_mesh(m, 0.8)
    return fedd_lib.p2_of_p1(m, volume_id=0)


@pytest.mark.parametrize("which", ["square_p2", "cylinder_p2", "cube_p1", "square_p1", "distorted_p1", "distorted_p2"])
def test_advection_matrices_match_the_restatement(fedd_lib, ctx, which):
    """N, W and N + W: same pattern (FULL, structural zeros included) and the value criterion of the other parity tests; the
    slot_add path; bitwise reproducibility.  (square_p1 is the one case whose two forms take different rules: 3 and 7 points.)"""
    m = _mesh(fedd_lib, which)
    dim = m["dim"]
    R = Restatement(fedd_lib, m)
    u = smooth_velocity(m["xyz"])
    ctx.mesh_set_dict(m)
    ctx.velocity_set(u)
    No, Wo = R.N(u.ravel()), R.W(u.ravel())
    got = {}
    for kind, ref in ((fedd_lib.ADV_N, No), (fedd_lib.ADV_W, Wo), (fedd_lib.ADV_NEWTON, No + Wo)):
        ctx.assemble_advection(kind, 1.0, -1, 4)
        A = ctx.matrix_get(4)
        if kind == fedd_lib.ADV_NEWTON:     # scipy's sum drops the structural zeros: put it back on the pattern
            ref = sp.coo_matrix((np.concatenate([No.data, Wo.data]), (np.concatenate([_rows(No), _rows(Wo)]),
                                                                       np.concatenate([No.indices, Wo.indices]))),
                                shape=No.shape).tocsr()
        err = assert_matrix_close(A, ref)
        print("%s kind %d: max error / row scale %.2e" % (which, kind, err))
        got[kind] = A.data.copy()
        ctx.assemble_advection(kind, 1.0, -1, 4)
        assert np.array_equal(got[kind], ctx.matrix_get(4).data)                 # bit for bit
    # scale and slot_add: F = A + rho N with A = nu * vector Laplacian on the DIAG pattern
    nu, rho = 0.37, 1.9
    ctx.pattern_build(dim, fedd_lib.BLOCK_DIAG)
    ctx.assemble(fedd_lib.FORM_LAPLACE_VEC)
    ctx.matrix_scale(-1, nu)
    ctx.matrix_store(0)
    for kind in (fedd_lib.ADV_N, fedd_lib.ADV_NEWTON):
        ctx.assemble_advection(kind, 1.0, -1, 3)
        Nd, Ad = ctx.matrix_get(3), ctx.matrix_get(0)
        ctx.assemble_advection(kind, rho, 0, 4)
        F = ctx.matrix_get(4)
        ref = sp.coo_matrix((np.concatenate([rho * Nd.data, Ad.data]), (np.concatenate([_rows(Nd), _rows(Ad)]),
                                                                         np.concatenate([Nd.indices, Ad.indices]))),
                            shape=Nd.shape).tocsr()
        assert_matrix_close(F, ref)
        # ... and with a FULL matrix in slot_add
        ctx.assemble_advection(kind, -0.5, 4, 2)
        ref2 = F.copy()
        ref2.data = F.data - 0.5 * Nd.data
        assert_matrix_close(ctx.matrix_get(2), ref2)
    with pytest.raises(fedd_lib.FeddError, match="must differ"):
        ctx.assemble_advection(fedd_lib.ADV_N, 1.0, 4, 4)


def _rows(A):
    return np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))


def test_velocity_is_needed_and_dropped_with_the_mesh(fedd_lib, ctx):
    m = fedd_lib.structured_mesh(2, 1, 3)
    ctx.mesh_set_dict(m)
    with pytest.raises(fedd_lib.FeddError, match="fedd_velocity_set"):
        ctx.assemble_advection(fedd_lib.ADV_N, 1.0, -1, 4)
    ctx.velocity_set(np.ones((m["xyz"].shape[0], 2)))
    ctx.assemble_advection(fedd_lib.ADV_N, 1.0, -1, 4)
    ctx.mesh_set_dict(fedd_lib.structured_mesh(2, 1, 4))
    with pytest.raises(fedd_lib.FeddError, match="fedd_velocity_set"):
        ctx.assemble_advection(fedd_lib.ADV_N, 1.0, -1, 4)
    with pytest.raises(fedd_lib.FeddError, match="unknown kind"):
        ctx.assemble_advection(7, 1.0, -1, 4)


def test_set_zeros_threshold_on_the_advection_matrices(fedd_lib, ctx):
    """setZeros_ / myeps_ (FE_def.hpp:1816, 1908) under the existing option "asm_zero_eps": element values of N and of W below
    the threshold are dropped before they are added"""
    m = p2_meshes(fedd_lib)["square_p2"]
    R = Restatement(fedd_lib, m)
    u = smooth_velocity(m["xyz"])
    bn, bw = R.blocks_N(u.ravel()), R.blocks_W(u.ravel())
    d = np.arange(m["dim"])
    vals = np.unique(np.abs(bn[:, :, d, :, d]))        # (the values of N are the larger ones: a threshold inside their range cuts into W too)
    vals = vals[vals > 1e-8 * vals.max()]
    k = int(0.1 * vals.shape[0])
    i = k - 50 + int(np.argmax(vals[k - 49:k + 51] / vals[k - 50:k + 50]))      # the widest gap near the 0.1 quantile (no value of N or W within 1e-3 of it)
    eps = float(np.sqrt(vals[i] * vals[i + 1]))
    ctx.mesh_set_dict(m)
    ctx.velocity_set(u)
    try:
        ctx.set_option("asm_zero_eps", eps)
        for kind, blocks in ((fedd_lib.ADV_N, [bn]), (fedd_lib.ADV_W, [bw]), (fedd_lib.ADV_NEWTON, [bn, bw])):
            ref = R.assemble(sum(np.where(np.abs(b) < eps, 0.0, b) for b in blocks))
            ctx.assemble_advection(kind, 1.0, -1, 4)
            assert_matrix_close(ctx.matrix_get(4), ref)
            assert abs(ref - R.assemble(sum(blocks))).max() > 1e-3 * abs(ref).max()        # the threshold did something
    finally:
        ctx.set_option("asm_zero_eps", 0.0)


@pytest.mark.parametrize("which", ["square_p2", "cylinder_p2", "cube_p1"])
def test_newton_matrix_is_the_jacobian(fedd_lib, ctx, which):
    """[N(u + eps v)(u + eps v) - N(u) u] / eps against (N(u) + W(u)) v, all matrices from the device.  N is linear in u, so the
    quotient differs from the derivative by exactly eps N(v) v; the rest is rounding.  Rounding bound of one product (A x)_i
    with a device matrix: ops * 2^-53 * (|A| |x|)_i, where |A| is the restatement with every product replaced by its magnitude
    (what the computed entries can be off by, cancellation inside the element integrals included) and ops counts the
    floating-point operations behind one term: the quadrature sum of an entry (nq points, dim + 2 products and a sum each, after
    u_h / grad u_h from nen values), the row sum over the incident elements, the product with x over the row.  eps is chosen
    so that the truncation term is a tenth of the rounding term of the quotient."""
    m = _mesh(fedd_lib, which)
    dim, nen = m["dim"], m["conn"].shape[1]
    R = Restatement(fedd_lib, m)
    rng = np.random.default_rng(11)
    n = dim * m["xyz"].shape[0]
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    ctx.mesh_set_dict(m)

    def dev(kind, w):
        ctx.velocity_set(w)
        ctx.assemble_advection(kind, 1.0, -1, 4)
        return ctx.matrix_get(4)

    Nabs_u = R.N(np.abs(u), absolute=True)
    JabsV = (Nabs_u + R.W(np.abs(u), absolute=True)) @ np.abs(v)
    nq = max(fedd_lib.fe_quadrature(dim, d)[1].shape[0] for d in degrees(dim, nen))
    deg = np.bincount(m["conn"].ravel()).max()
    rowlen = np.diff(Nabs_u.indptr).max()
    ops = nq * (dim + 3) + 2 * nen * dim + deg + rowlen
    trunc_unit = np.abs(R.N(v) @ v)                                             # eps times this is the truncation term
    round_unit = ops * U * 2.0 * (Nabs_u @ np.abs(u))                           # this over eps is the quotient's rounding term
    eps = float(np.sqrt(0.1 * round_unit.max() / trunc_unit.max()))
    w = u + eps * v
    q = (dev(fedd_lib.ADV_N, w) @ w - dev(fedd_lib.ADV_N, u) @ u) / eps
    Jv = dev(fedd_lib.ADV_NEWTON, u) @ v
    bound = eps * trunc_unit + ops * U * ((R.N(np.abs(w), absolute=True) @ np.abs(w)) + Nabs_u @ np.abs(u)) / eps + ops * U * JabsV
    err = np.abs(q - Jv)
    print("%s: eps %.2e, max error %.2e, max bound %.2e, largest error / bound %.2e"
          % (which, eps, err.max(), bound.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert eps * trunc_unit.max() < (round_unit / eps).max()
    assert np.all(err <= bound)


# ---- nonlinear iterations at the ABI level ---------------------------------------------------------------------------------
SLOT_A, SLOT_B, SLOT_BT, SLOT_F = 0, 1, 2, 4


class NavierStokesABI:
    """P2 / P1 steady Navier-Stokes on a one-rank mesh: A = rho nu * vector Laplacian, B, B^T scaled by -1
    (NavierStokes::assembleConstantMatrices), and per iteration F = A + rho (N | N + W)(u) from one device pass, merged with
    B, B^T.  residual = system x - rhs with x - g on the Dirichlet rows."""

    def __init__(self, fedd_lib, ctx, m1, mv, nu, rho, rows, vals):
        self.L, self.c, self.dim = fedd_lib, ctx, mv["dim"]
        self.nv, self.n_p = mv["xyz"].shape[0], m1["xyz"].shape[0]
        self.n = self.dim * self.nv + self.n_p
        self.rho, self.rows, self.vals = rho, np.asarray(rows), np.asarray(vals, dtype=np.float64)
        ctx.mesh_set_dict(mv)
        ctx.pattern_build(self.dim, fedd_lib.BLOCK_DIAG)
        ctx.assemble(fedd_lib.FORM_LAPLACE_VEC)
        ctx.matrix_scale(-1, rho * nu)
        ctx.matrix_store(SLOT_A)
        ctx.assemble_div(self.n_p, SLOT_B, SLOT_BT)
        ctx.matrix_scale(SLOT_B, -1.0)
        ctx.matrix_scale(SLOT_BT, -1.0)

    def system(self, kind, x):
        self.c.velocity_set(x[:self.dim * self.nv])
        self.c.assemble_advection(kind, self.rho, SLOT_A, SLOT_F)
        self.c.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)

    def residual(self, x):
        self.system(self.L.ADV_N, x)
        r = self.c.spmv(x)
        r[self.rows] = x[self.rows] - self.vals
        return r

    def linear_solve(self, rtol_lin, prec):
        if prec:        # the matrix has changed: monolithic one-level Schwarz is set up again on it, as cfg 4 does once
            self.c.schwarz_setup(overlap=1, combine=self.L.COMBINE_RESTRICTED)
            return self.c.gmres(None, rtol=rtol_lin, max_it=1500, restart=300, use_prec=True)
        return self.c.gmres(None, rtol=rtol_lin, max_it=4 * self.n, restart=min(self.n, 600), use_prec=False)

    def solve(self, method, x0, tol, max_its, rtol_lin, after_iteration=None, prec=False):
        """residual first, relative to the first one; then the linear solve and the update"""
        x = np.array(x0, dtype=np.float64)
        hist = []
        for k in range(max_its + 1):
            r = self.residual(x)
            hist.append(float(np.linalg.norm(r)))
            if hist[-1] / hist[0] < tol or k == max_its:
                break
            # both linearisations solve for the update, system * dx = -r (NonLinearProblem::solveAndUpdate), so the linear rtol is
            # relative to the current nonlinear residual; fixed point keeps the matrix of the residual, Newton adds W
            if method == "Newton":
                self.system(self.L.ADV_NEWTON, x)
            b = -r
            b[self.rows] = 0.0
            self.c.rhs_set(b)
            self.c.dirichlet_rows(self.rows, -r[self.rows])
            dx, its, rel = self.linear_solve(rtol_lin, prec)
            x += dx
            assert rel <= 100 * rtol_lin, rel
            if after_iteration:
                after_iteration(k)
        return x, hist


def _channel(fedd_lib, M, profile):
    """unit square, P2 / P1: inflow profile(y) on x = 0, no-slip walls y = 0, 1, natural outflow on x = 1"""
    m1 = fedd_lib.structured_mesh(2, 1, M)
    mv = fedd_lib.p2_of_p1(m1, volume_id=0)
    X = mv["xyz"]
    inflow = X[:, 0] < 1e-12
    wall = (X[:, 1] < 1e-12) | (X[:, 1] > 1 - 1e-12)
    nodes = np.nonzero(inflow | wall)[0]
    rows = (2 * nodes[:, None] + np.arange(2)[None, :]).ravel()
    vals = np.zeros((nodes.shape[0], 2))
    sel = inflow[nodes] & ~wall[nodes]
    vals[sel, 0] = profile(X[nodes, 1])[sel]
    return m1, mv, rows, vals.ravel()


def _host_reference(fedd_lib, m1, mv, nu, rho, rows, vals, tol=1e-12):
    """sparse-direct Newton on the restatement, to `tol` on the update and the residual; returns x, the residual history and
    ||J^-1||_2 of the Jacobian on the free rows at the solution (power iteration on J^-T J^-1 with the sparse factors, run until
    the estimate moves by less than 1 %; it approaches the norm from below, hence the factor 1.05 at its use)"""
    dim = mv["dim"]
    R = Restatement(fedd_lib, mv)
    Ao, BTo, Bo = fo.stokes_blocks(oracle_mesh(mv), oracle_mesh(m1), rho * nu)
    nvd, n_p = Ao.shape[0], Bo.shape[0]
    n = nvd + n_p
    free = np.ones(n, dtype=bool); free[rows] = False
    x = np.zeros(n); x[rows] = vals
    hist = []
    for k in range(40):
        u = x[:nvd]
        N = R.N(u)
        K = sp.bmat([[Ao + rho * N, BTo], [Bo, None]], format="csr")
        r = K @ x
        r[rows] = 0.0
        hist.append(float(np.linalg.norm(r)))
        if k > 0 and hist[-1] <= tol * hist[0] and step <= tol * np.abs(x).max():
            break
        J = sp.bmat([[Ao + rho * (N + R.W(u)), BTo], [Bo, None]], format="csc")
        dx = np.zeros(n)
        dx[free] = spla.splu(J[free][:, free]).solve(-r[free])
        step = np.abs(dx).max()
        x += dx
    lu = spla.splu(sp.bmat([[Ao + rho * (R.N(x[:nvd]) + R.W(x[:nvd])), BTo], [Bo, None]], format="csc")[free][:, free])
    z = np.random.default_rng(3).standard_normal(int(free.sum()))
    est = 0.0
    for it in range(200):
        z /= np.linalg.norm(z)
        y = lu.solve(z)
        new = float(np.linalg.norm(y))
        z = lu.solve(y, trans="T")
        if it > 5 and abs(new - est) <= 0.01 * new:
            est = new
            break
        est = new
    return x, hist, est


def test_poiseuille_is_the_stokes_solution(fedd_lib, ctx):
    """Channel with parabolic inflow and natural outflow: u = (4 y (1 - y), 0), p = 8 nu rho (1 - x) solves Stokes, lies in
    P2 / P1, and (u . grad) u = 0 -- so it solves Navier-Stokes too.  Started there, the first nonlinear residual is at rounding
    level of the residual at the zero state (which carries the boundary values) for both linearisations; from zero both reach it."""
    nu, rho = 0.05, 1.3
    m1, mv, rows, vals = _channel(fedd_lib, 4, lambda y: 4.0 * y * (1.0 - y))
    ns = NavierStokesABI(fedd_lib, ctx, m1, mv, nu, rho, rows, vals)
    X, nvd = mv["xyz"], 2 * mv["xyz"].shape[0]
    exact = np.zeros(ns.n)
    exact[0:nvd:2] = 4.0 * X[:, 1] * (1.0 - X[:, 1])
    exact[nvd:] = 8.0 * nu * rho * (1.0 - m1["xyz"][:, 0])
    r0 = np.linalg.norm(ns.residual(np.zeros(ns.n)))
    rel = np.linalg.norm(ns.residual(exact)) / r0
    print("Poiseuille: residual at the exact state / residual at zero = %.2e" % rel)
    assert rel <= 1e-12
    for method in ("FixedPoint", "Newton"):
        x, hist = ns.solve(method, np.zeros(ns.n), 1e-10, 10, 1e-12)
        print("Poiseuille %s from zero: residuals %s" % (method, ["%.2e" % h for h in hist]))
        assert hist[-1] / hist[0] < 1e-10
        np.testing.assert_allclose(x, exact, rtol=0, atol=1e-9 * np.abs(exact).max())
        assert np.linalg.norm(ns.residual(x)) <= 1e-10 * r0         # restarted there, the first residual is already converged


def _cylinder(fedd_lib):
    """the 1k DFG cylinder, P2 / P1, with the boundary conditions of the cfg-4 Stokes test (test_gpu_stokes.py): no-slip on flags
    1 and 4, parabolic_benchmark inflow on flag 2 (height 0.41, largest velocity 1), flag 3 natural"""
    m1 = fedd_lib.read_mesh(os.path.join(GOLD, "DFG3DCylinder_1k.mesh"), 3)
    mv = fedd_lib.p2_of_p1(m1, volume_id=0)
    X, flag, H = mv["xyz"], mv["flag_uni"], 0.41
    nodes = np.nonzero(np.isin(flag, (1, 2, 4)))[0]
    rows = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
    vals = np.zeros((nodes.shape[0], 3))
    inflow = flag[nodes] == 2
    y, z = X[nodes, 1], X[nodes, 2]
    vals[inflow, 0] = (16.0 * y * (H - y) * z * (H - z) / H ** 4)[inflow]
    return m1, mv, rows, vals.ravel()


@pytest.mark.parametrize("which", ["cylinder_1k", "channel"])
def test_flow_where_advection_matters_and_no_symbolic_rebuild(fedd_lib, ctx, which):
    """cylinder_1k: the reference's 1k cylinder with the cfg-4 boundary conditions at viscosity 0.01 (Reynolds number about 4 on
    the cylinder: the scipy runs take 5 Newton and 10 fixed-point iterations to 1e-8), every linear system solved by GMRES with
    monolithic one-level Schwarz SET UP AGAIN on the re-assembled merged matrix.  channel: a 6 x 6 unit square with a skewed
    inflow, unpreconditioned GMRES.  Reference: sparse-direct Newton on the restatement, run to 1e-12 here.

    Margin.  The iterations stop when the true nonlinear residual r(x) = K(x) x - f (a device SpMV with the re-assembled
    matrix) is below relNonLinTol * ||r_0||, whatever the linear rtol was: rtol decides how many iterations that takes (an
    inexact Newton step leaves rtol * ||r_k|| plus the quadratic term, so rtol must be below relNonLinTol: 1e-10 against 1e-8),
    not where they stop.  With e = x - x*, r(x) - r(x*) = J(x*) e + N(e) e, so ||e|| <= ||J^-1|| (||r(x)|| + ||r(x*)|| + O(||e||^2))
    on the free rows; the Dirichlet rows carry the same values.  Asserted: ||x - x_ref||_2 <= 1.05 * ||J^-1||_2 * (relNonLinTol *
    ||r_0|| + ||r(x_ref)||), ||J^-1||_2 computed here from the sparse factors (1.05: the power iteration's 1 % stop and the
    second-order term).

    Newton's residuals fall quadratically: every ratio r_{k+1} / r_k^2 is at most ten times the largest ratio of the scipy run
    (the device takes inexact steps); ratios are taken where r_{k+1} >= 100 * rtol * r_k, i.e. where the linear residual is at
    most 1 % of it, and above the rounding floor 1e-11 ||r_0|| of the scipy run.  Fixed point takes more iterations than
    Newton.  With timing on, the symbolic timer (adjacency, patterns, gather lists) counts launches in the first iteration
    only, while the Schwarz setup runs in every one."""
    prec = which == "cylinder_1k"
    nu, rho, tol, rtol = 0.01, 1.0, 1e-8, 1e-10
    if prec:
        m1, mv, rows, vals = _cylinder(fedd_lib)
    else:
        m1, mv, rows, vals = _channel(fedd_lib, 6, lambda y: 6.0 * y * y * (1.0 - y) + np.sin(np.pi * y))
    xref, href, jinv = _host_reference(fedd_lib, m1, mv, nu, rho, rows, vals)
    print("%s: scipy Newton residuals %s, ||J^-1||_2 = %.3e" % (which, ["%.2e" % h for h in href], jinv))
    assert len(href) >= 4
    ns = NavierStokesABI(fedd_lib, ctx, m1, mv, nu, rho, rows, vals)
    x_start = np.zeros(ns.n); x_start[rows] = vals
    ctx.timing_enable(True)
    ctx.timing_reset()
    launches = []

    def record(k):
        t = ctx.timing_get()
        launches.append((t["symbolic"][1], t["schwarz_setup"][1]))

    xn, hn = ns.solve("Newton", x_start, tol, 25, rtol, after_iteration=record, prec=prec)
    ctx.timing_enable(False)
    print("device Newton residuals", ["%.2e" % h for h in hn], "(symbolic, Schwarz setup) launches after each iteration", launches)
    assert len(launches) >= 3 and launches[0][0] >= 1 and all(l[0] == launches[0][0] for l in launches)
    if prec:
        assert all(launches[k + 1][1] > launches[k][1] for k in range(len(launches) - 1)) and launches[0][1] >= 1
    assert hn[-1] / hn[0] < tol
    bound = 1.05 * jinv * (tol * hn[0] + href[-1])
    err_n = np.linalg.norm(xn - xref)
    print("Newton: ||x - x_ref|| = %.3e, bound %.3e" % (err_n, bound))
    assert err_n <= bound

    def ratios(h, floor_rel):
        return [h[k + 1] / h[k] ** 2 for k in range(len(h) - 1) if h[k + 1] >= floor_rel * h[k] and h[k + 1] > 1e-11 * h[0]]

    assert max(ratios(hn, 100 * rtol)) <= 10.0 * max(ratios(href, 0.0))
    xf, hf = ns.solve("FixedPoint", x_start, tol, 200, rtol, prec=prec)
    err_f = np.linalg.norm(xf - xref)
    print("device fixed-point iterations %d, Newton %d; fixed point ||x - x_ref|| = %.3e, bound %.3e"
          % (len(hf) - 1, len(hn) - 1, err_f, 1.05 * jinv * (tol * hf[0] + href[-1])))
    assert hf[-1] / hf[0] < tol
    assert err_f <= 1.05 * jinv * (tol * hf[0] + href[-1])
    assert len(hf) > len(hn)

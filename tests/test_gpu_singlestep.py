"""Single-step (Runge-Kutta) time stepping at the ABI level (include/fedd_hip.h "Single-step time stepping", singlestep.hip):
the stage store, fedd_stage_rhs bit for bit against the numpy composition of fedd_matrix_apply results in the normative order,
fedd_block_merge_scaled, fedd_stage_error, and whole steps on the channel of tests/test_gpu_time_navier_stokes.py (same mesh
builder, boundary data, nu, dt, tolerances) against tests/singlestep_ref.py.

Meshes and the row-length classes they reach (G = the lane group of a block: 8 lanes up to 32 entries in its longest row, else 16;
"short" = a row with fewer entries than G, "long" = one with more).  Asserted below from fedd_matrix_get:
    square  4 x 4 cells, P2 / P1   M (DIAG) G 8, rows 6 .. 19: short and long;  F (FULL) G 16, rows 12 .. 38: short and long;
                                   B^T G 8, rows 3 .. 7: short only.                     The kernel runs 16 lanes per row.
    cube    3 x 3 x 3 cells        M G 16, rows 10 .. 65: short and long;  F G 16, rows 30 .. 195: long only;
                                   B^T G 8, rows 4 .. 15: short and long.                16 lanes per row.
    cell    1 x 1 cell, 2D         every block G 8 (F rows 12 .. 18, B^T 3 .. 4): the kernel with 8 lanes per row.

Bar of the step tests: that of tests/test_gpu_time_navier_stokes.py, taken over with its procedure and applied stage by stage.
With e = x - x_ref of one stage solve, ||e|| <= 1.05 ||J^-1||_2 (||r(x)|| + ||r(x_ref)||), J the Jacobian of the stage system
[M + (dt a_ss) (A + rho (N + W)), s_bt B^T ; B, 0] at the reference, both residuals driven to the floor.  The floor is that
file's absolute one, TOL * ||r_0||, times dt * a_ss: the stage system is (dt a_ss) times a system of that file's scaling,
(1 / (dt a_ss)) M + A + rho N.  The reference of a stage starts from what the DEVICE kept of the stages before it (fedd_stage_get),
so no error of an earlier stage is carried through the bound."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import singlestep_ref as ssr
from test_gpu_navier_stokes import NavierStokesABI, SLOT_A, SLOT_B, SLOT_BT, SLOT_F
from test_gpu_time_navier_stokes import DT, NU, RHO, RTOL_LIN, SLOT_AT, SLOT_M, TOL, Device, case
from test_navier_stokes_abi import Restatement

pytestmark = pytest.mark.gpu

CLASSES = {      # mesh -> block -> (G, short, long)
    "square": {"M": (8, True, True), "F": (16, True, True), "BT": (8, True, False)},
    "cube": {"M": (16, True, True), "F": (16, False, True), "BT": (8, True, True)},
    "cell": {"M": (8, True, True), "F": (8, False, True), "BT": (8, True, False)},
}


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


_MESH = {}


def meshes(fedd_lib, which):
    if which not in _MESH:
        dim, cells = {"square": (2, 4), "cube": (3, 3), "cell": (2, 1)}[which]
        m1 = fedd_lib.structured_mesh(dim, 1, cells)
        _MESH[which] = (m1, fedd_lib.p2_of_p1(m1, volume_id=0))
    return _MESH[which]


class Blocks:
    """A, B, B^T, M in slots 0, 1, 2, 5 and F(u) = A + rho N(u) in slot 4; the merged system, so that the solution vector has its
    length"""

    def __init__(self, L, c, m1, mv, seed=0):
        self.L, self.c, self.dim = L, c, mv["dim"]
        self.nv, self.n_p = mv["xyz"].shape[0], m1["xyz"].shape[0]
        self.nvd = self.dim * self.nv
        self.n = self.nvd + self.n_p
        self.rng = np.random.default_rng(seed)
        c.mesh_set_dict(mv)
        c.pattern_build(self.dim, L.BLOCK_DIAG)
        c.assemble(L.FORM_LAPLACE_VEC)
        c.matrix_scale(-1, 0.3)
        c.matrix_store(SLOT_A)
        c.assemble_div(self.n_p, SLOT_B, SLOT_BT)
        c.pattern_build(self.dim, L.BLOCK_DIAG)
        c.assemble(L.FORM_MASS_VEC)
        c.matrix_store(SLOT_M)

    def operator(self, x):
        self.c.velocity_set(x[:self.nvd])
        self.c.assemble_advection(self.L.ADV_N, 1.7, SLOT_A, SLOT_F)

    def push(self, x, merge=False):
        self.operator(x)
        if merge:
            self.c.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)
        self.c.solution_set(x)
        self.c.stage_push(SLOT_F)

    def three_stages(self, max_stages=4):
        self.c.stage_begin(max_stages)
        U = [self.rng.standard_normal(self.n) for _ in range(3)]
        vals = []
        for j, x in enumerate(U):
            self.push(x, merge=j == 0)
            vals.append(self.c.matrix_get(SLOT_F).data.copy())
        return U, vals


def _classes(A):
    rows = np.diff(A.indptr)
    G = 8 if rows.max() <= 32 else 16
    return G, bool((rows < G).any()), bool((rows > G).any())


@pytest.mark.parametrize("which", ["square", "cube", "cell"])
def test_stage_rhs_bit_for_bit(fedd_lib, ctx, which):
    m1, mv = meshes(fedd_lib, which)
    b = Blocks(fedd_lib, ctx, m1, mv, seed=1)
    c, nvd = ctx, b.nvd
    ctx.stage_begin(3)
    U = [b.rng.standard_normal(b.n) for _ in range(3)]
    Fu, Bp = [], []
    for j, x in enumerate(U):
        b.push(x, merge=j == 0)
        Fu.append(c.matrix_apply(SLOT_F, x[:nvd]))
        Bp.append(c.matrix_apply(SLOT_BT, x[nvd:]))
    Mu0 = c.matrix_apply(SLOT_M, U[0][:nvd])
    got = {k: _classes(c.matrix_get(s)) for k, s in (("M", SLOT_M), ("F", SLOT_F), ("BT", SLOT_BT))}
    print(which, "classes (G, short, long):", got)
    assert got == CLASSES[which]
    # the slot's own values have moved on to stage 2; the store holds all three
    cf = np.array([-0.0125, 0.3, -1.7])
    for n_prior in (1, 2, 3):
        variants = [("zero", np.zeros(n_prior), SLOT_BT), ("zero, no slot", np.zeros(n_prior), -1),
                    ("nonzero", np.array([0.7, -0.05, 2.5])[:n_prior], SLOT_BT),
                    ("mixed", np.array([0.0, -0.05, 0.0])[:n_prior] if n_prior > 1 else np.array([0.9]), SLOT_BT),
                    ("mixed 2", np.array([0.4, 0.0, 1.5])[:n_prior], SLOT_BT)]
        for name, cbt, slot_bt in variants:
            t = Mu0.copy()
            for j in range(n_prior):
                mv_ = cf[j] * Fu[j]
                if cbt[j] != 0.0:
                    mv_ = mv_ + (cbt[j] * Bp[j])
                t = t + mv_
            c.rhs_set(np.full(b.n, 7.0))
            c.stage_rhs(SLOT_M, slot_bt, cf[:n_prior], cbt)
            r1 = c.rhs_get()
            np.testing.assert_array_equal(r1[:nvd], t, err_msg="%s n_prior %d %s" % (which, n_prior, name))
            assert not r1[nvd:].any() and not np.signbit(r1[nvd:]).any()
            c.rhs_set(np.full(b.n, -3.0))
            c.stage_rhs(SLOT_M, slot_bt, cf[:n_prior], cbt)
            np.testing.assert_array_equal(c.rhs_get(), r1)


@pytest.mark.parametrize("which", ["square", "cube"])
def test_stage_store_keeps_what_was_pushed(fedd_lib, ctx, which):
    m1, mv = meshes(fedd_lib, which)
    b = Blocks(fedd_lib, ctx, m1, mv, seed=2)
    assert ctx.stage_info() == (0, 0, 0, 0)
    U, vals = b.three_stages(max_stages=4)
    nnz = vals[0].shape[0]
    assert ctx.stage_info() == (4, 3, nnz, b.n)
    # between push and read-back: another operator in slot 4, a merge, Dirichlet rows
    b.operator(b.rng.standard_normal(b.n))
    ctx.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)
    ctx.dirichlet_rows(np.arange(0, b.nvd, 7), np.zeros(len(range(0, b.nvd, 7))))
    for j in range(3):
        v, u = ctx.stage_get(j)
        np.testing.assert_array_equal(v, vals[j])
        np.testing.assert_array_equal(u, U[j])
    assert not np.array_equal(vals[0], vals[1])
    # a new step: the count starts over, the buffers stay (the stage pushed next is read back, the old ones are out of reach)
    ctx.stage_begin(2)
    assert ctx.stage_info() == (2, 0, 0, 0)
    with pytest.raises(fedd_lib.FeddError, match="stage 0 of 0"):
        ctx.stage_get(0)
    x = b.rng.standard_normal(b.n)
    b.push(x)
    assert ctx.stage_info() == (2, 1, nnz, b.n)
    np.testing.assert_array_equal(ctx.stage_get(0)[1], x)
    np.testing.assert_array_equal(ctx.stage_get(0)[0], ctx.matrix_get(SLOT_F).data)


def _merged(c):
    rowptr, col, val, _ = c.csr_get()
    return rowptr, col, val


@pytest.mark.parametrize("which", ["square", "cube"])
def test_block_merge_scaled(fedd_lib, ctx, which):
    m1, mv = meshes(fedd_lib, which)
    b = Blocks(fedd_lib, ctx, m1, mv, seed=3)
    c = ctx
    b.operator(b.rng.standard_normal(b.n))
    bt_before = c.matrix_get(SLOT_BT)
    c.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)
    rp0, ci0, v0 = _merged(c)
    # a fresh context state for the pattern-building path of the scaled merge: the combine takes the system slot away
    c.matrix_combine(SLOT_M, 1.0, SLOT_A, 0.5)
    c.block_merge_scaled(SLOT_F, SLOT_BT, 1.0, SLOT_B, -1)
    rp1, ci1, v1 = _merged(c)
    np.testing.assert_array_equal(rp1, rp0)
    np.testing.assert_array_equal(ci1, ci0)
    np.testing.assert_array_equal(v1, v0)
    c.block_merge_scaled(SLOT_F, SLOT_BT, 1.0, SLOT_B, -1)          # ... and the values-only path
    np.testing.assert_array_equal(_merged(c)[2], v0)
    rows = np.repeat(np.arange(b.n), np.diff(rp0))
    is_bt = (rows < b.nvd) & (ci0 >= b.nvd)
    assert is_bt.sum() == bt_before.nnz
    c.block_merge_scaled(SLOT_F, SLOT_BT, 0.125, SLOT_B, -1)
    rp2, ci2, v2 = _merged(c)
    np.testing.assert_array_equal(rp2, rp0)
    np.testing.assert_array_equal(ci2, ci0)
    np.testing.assert_array_equal(v2[is_bt], 0.125 * v0[is_bt])
    np.testing.assert_array_equal(v2[~is_bt], v0[~is_bt])
    np.testing.assert_array_equal(c.rhs_get(), np.zeros(b.n))
    np.testing.assert_array_equal(c.solution_get(), np.zeros(b.n))
    after = c.matrix_get(SLOT_BT)
    np.testing.assert_array_equal(after.data, bt_before.data)
    np.testing.assert_array_equal(after.indices, bt_before.indices)
    # fedd_block_merge keeps its bits
    c.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)
    np.testing.assert_array_equal(_merged(c)[2], v0)


def test_scaled_merge_with_another_factor_keeps_the_pattern_generation(fedd_lib, ctx):
    """What hangs on the pattern generation and can be read at the ABI: the solver's SpMV stream is kept (verified, not built)
    from one matrix to the next while the generation stands (fedd_spmv_reuse_info).  Exact zeros only and no row classes, so
    that the verification depends on the pattern of zeros alone, which a factor of two to some power cannot change."""
    C = case(fedd_lib)
    b = Blocks(fedd_lib, ctx, C["m1"], C["mv"], seed=4)
    c = ctx
    c.set_option("spmv_drop_tol", 0.0)
    c.set_option("spmv_classes", 0)
    b.operator(b.rng.standard_normal(b.n))
    rhs = b.rng.standard_normal(b.n)
    rhs[C["rows"]] = 0.0
    counts = []
    for s_bt in (0.125, 0.5, 2.0):
        c.block_merge_scaled(SLOT_F, SLOT_BT, s_bt, SLOT_B, -1)
        c.rhs_set(rhs)
        c.dirichlet_rows(C["rows"], np.zeros(len(C["rows"])))
        c.gmres(None, rtol=1e-6, max_it=60, restart=60, use_prec=False)
        counts.append(c.spmv_reuse_info())
    print("SpMV stream reuse after the three scaled merges:", counts)
    assert not counts[0]["last_reused"]
    assert counts[1]["last_reused"] and counts[2]["last_reused"]
    assert counts[2]["n_reused"] == counts[0]["n_reused"] + 2


# ---- whole steps --------------------------------------------------------------------------------------------------------------
class StageDevice(Device):
    """Device of tests/test_gpu_time_navier_stokes.py with the stage loop of the header in place of the multistep history"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.have_system = False
        self.stage_log = []         # (das, s_bt, b, kept operators, kept vectors, x, residual history) per stage solve

    def stage_system(self, kind, x, das, s_bt):
        self.combine(1.0, das)                                  # slot 6 <- (1.0 * M) + (das * A), when das changed
        self.c.velocity_set(x[:self.dim * self.nv])
        self.c.assemble_advection(kind, das * self.rho, SLOT_AT, SLOT_F)
        self.c.block_merge_scaled(SLOT_F, SLOT_BT, s_bt, SLOT_B, -1)
        self.have_system = True

    def push(self, x):
        self.c.velocity_set(x[:self.dim * self.nv])
        self.c.assemble_advection(self.L.ADV_N, self.rho, SLOT_A, SLOT_F)       # reAssembleAndFill: F = A + rho N(u)
        if not self.have_system:                                # the first push of a run: the solution vector needs its system
            self.c.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)
            self.have_system = True
        self.c.solution_set(x)
        self.c.stage_push(SLOT_F)

    def kept(self):
        P = self.c.matrix_get(SLOT_F)
        count = self.c.stage_info()[1]
        Fs, Us = [], []
        for j in range(count):
            v, u = self.c.stage_get(j)
            Fs.append(sp.csr_matrix((v, P.indices, P.indptr), shape=P.shape))
            Us.append(u)
        return Fs, Us

    def step(self, x_n, A, stop, fip=True):
        S = A.shape[0]
        self.c.stage_begin(S)
        self.push(x_n)
        x = x_n.copy()
        for s in range(1, S):
            cf, cbt, das, s_bt = ssr.stage_coefficients(A, s, self.dt, fip)
            self.stage_system(self.L.ADV_N, x, das, s_bt)       # the merged system the right-hand side is as long as
            self.c.stage_rhs(SLOT_M, SLOT_BT, cf, cbt)
            self.b = self.c.rhs_get()
            assert not self.b[self.dim * self.nv:].any()
            Fs, Us = self.kept()
            hist = []
            for k in range(40):
                self.stage_system(self.L.ADV_N, x, das, s_bt)
                r = self.c.spmv(x) - self.b
                r[self.rows] = x[self.rows] - self.vals
                hist.append(float(np.linalg.norm(r)))
                if (hist[-1] <= das * stop and k > 0) or k == 39:
                    break
                rhs = -r
                rhs[self.rows] = 0.0
                self.c.rhs_set(rhs)
                self.c.dirichlet_rows(self.rows, -r[self.rows])
                dx, its, rel = self.linear_solve(RTOL_LIN, False)
                x = x + dx
            self.stage_log.append(dict(das=das, s_bt=s_bt, b=self.b.copy(), Fs=Fs, Us=Us, cf=cf, cbt=cbt, x=x.copy(), hist=hist))
            if s + 1 < S:
                self.push(x)
        return x


class StageHost:
    """singlestep_ref on the matrices the device holds (fedd_matrix_get) and the restated advection"""

    def __init__(self, fedd_lib, ctx, mv, rows, vals):
        self.R = Restatement(fedd_lib, mv)
        self.A, self.M = ctx.matrix_get(SLOT_A).tocsr(), ctx.matrix_get(SLOT_M).tocsr()
        self.B, self.BT = ctx.matrix_get(SLOT_B).tocsr(), ctx.matrix_get(SLOT_BT).tocsr()
        self.nvd = self.M.shape[0]
        self.ref = ssr.SingleStep(self.M, lambda u: self.A + RHO * self.R.N(u), self.BT, self.B, None, rows, vals, nl_tol=1e-15)

    def jinv(self, x, das, s_bt):
        u = x[:self.nvd]
        V = self.M + das * (self.A + RHO * (self.R.N(u) + self.R.W(u)))
        J = sp.bmat([[V, s_bt * self.BT], [self.B, None]], format="csc")
        free = self.ref.free
        lu = spla.splu(J[free][:, free].tocsc())
        z = np.random.default_rng(3).standard_normal(int(free.sum()))
        est = 0.0
        for it in range(200):
            z /= np.linalg.norm(z)
            y = lu.solve(z)
            new = float(np.linalg.norm(y))
            z = lu.solve(y, trans="T")
            if it > 5 and abs(new - est) <= 0.01 * new:
                return new
            est = new
        return est

    def check(self, log, stop, what, x_ref=None):
        """the bar of the module docstring for one stage solve; x_ref given: that state against the device's (steady state)"""
        das, s_bt = log["das"], log["s_bt"]
        b = ssr.stage_rhs(self.M, self.BT, log["Fs"], log["Us"], log["cf"], log["cbt"])
        if x_ref is None:
            xr, hist = self.ref.solve_stage(log["Us"][-1], das, s_bt, b)
            rr = hist[-1]
        else:
            xr = x_ref
            rr = float(np.linalg.norm(self.ref.residual(xr, das, s_bt, b)))
        jinv = self.jinv(xr, das, s_bt)
        bound = 1.05 * jinv * (das * stop + rr)
        err = float(np.linalg.norm(log["x"] - xr))
        print("%s: residuals %s ||x - x_ref|| = %.3e bound %.3e (||J^-1|| %.3e, ||r(x_ref)|| %.2e)"
              % (what, ["%.2e" % h for h in log["hist"]], err, bound, jinv, rr))
        assert log["hist"][-1] <= das * stop
        assert err <= bound
        return bound


def _start(fedd_lib):
    C = case(fedd_lib)
    H = C["host"]
    x_start = np.zeros(H.n)
    x_start[C["rows"]] = C["vals"]
    return C, H, x_start, TOL * H.r0(x_start)


def _changes(A, dt, n_steps):
    """how often dt * a_ss differs from the stage before it over the run: the combines a loop needs"""
    seq = [ssr.stage_coefficients(A, s, dt, True)[2] for _ in range(n_steps) for s in range(1, A.shape[0])]
    return 1 + sum(1 for a, b in zip(seq, seq[1:]) if a != b)


@pytest.mark.parametrize("number,n_steps", [(1, 3), (2, 2)])
def test_steps_against_the_host_reference_and_combine_counts(fedd_lib, ctx, number, n_steps):
    """three Crank-Nicolson steps; two steps of table 2 (four stages, three prior stages in the last one); full implicit
    pressure, fixed point"""
    C, H, x_start, stop = _start(fedd_lib)
    c_, A = fedd_lib.butcher_table(number)
    d = StageDevice(fedd_lib, ctx, C["m1"], C["mv"], C["rows"], C["vals"])
    SH = StageHost(fedd_lib, ctx, C["mv"], C["rows"], C["vals"])
    x = x_start
    per_step = []
    for step in range(n_steps):
        before = d.combines
        x = d.step(x, A, stop)
        per_step.append(d.combines - before)
    for k, log in enumerate(d.stage_log):
        SH.check(log, stop, "table %d step %d stage %d" % (number, k // (A.shape[0] - 1) + 1, k % (A.shape[0] - 1) + 1))
        assert len(log["Fs"]) == k % (A.shape[0] - 1) + 1
    want = [_changes(A, DT, s + 1) - (_changes(A, DT, s) if s else 0) for s in range(n_steps)]
    print("combines per step", per_step, "expected from the changes of dt * a_ss", want)
    assert per_step == want
    assert per_step[0] >= 1 and (number != 1 or per_step == [1, 0, 0])
    assert np.linalg.norm(x - x_start) > 1e-3 * np.linalg.norm(x_start)       # the flow moved: the steps did something


def test_table_0_against_the_bdf1_step(fedd_lib, ctx):
    """One step of table 0 through the stage entries and one BDF1 step through fedd_multistep_*, from the same state.  The stage
    system is dt times the BDF1 system on the velocity rows and equal to it on the pressure rows, the right-hand sides likewise
    (M u_n against (1 / dt) M u_n; the prior stage enters with the coefficient -(dt * 0)).  A stage residual below dt * stop is
    therefore a BDF1 residual below stop, and both solutions lie within the bar of test_gpu_time_navier_stokes.py of each other:
    ||x_a - x_b|| <= 1.05 ||J^-1|| (stop + stop), J the Jacobian of the BDF1 system at the BDF1 solution."""
    C, H, x_start, stop = _start(fedd_lib)
    c_, A = fedd_lib.butcher_table(0)
    d = StageDevice(fedd_lib, ctx, C["m1"], C["mv"], C["rows"], C["vals"])
    xa = d.step(x_start, A, stop)
    assert d.stage_log[-1]["hist"][-1] <= DT * stop and d.combines == 1
    d2 = Device(fedd_lib, ctx, C["m1"], C["mv"], C["rows"], C["vals"])
    xb, hist = d2.time_step(0, x_start, "FixedPoint", stop)
    assert hist[-1] <= stop
    jinv = H.jinv(xb, 1.0 / DT)
    err, bound = float(np.linalg.norm(xa - xb)), 1.05 * jinv * 2.0 * stop
    print("table 0 against BDF1: ||x_a - x_b|| = %.3e bound %.3e (||J^-1|| %.3e)" % (err, bound, jinv))
    assert err <= bound
    assert np.linalg.norm(xb - x_start) > 1e-3 * np.linalg.norm(x_start)


def test_steady_state_stays_where_it_is(fedd_lib, ctx):
    """Started from the converged steady solution of the device, three Crank-Nicolson steps leave it there: with U_0 = x_s the
    stage residual of x_s is (dt / 2) F(x_s) u_s + dt B^T p_s + (dt / 2) F_0 u_0 = dt * r_steady(x_s) on the velocity rows.  The
    bar applies with x_ref = x_s and ||r(x_ref)|| formed on the host from what the device kept (exactly that term in the first
    step, plus the drift of the device's states afterwards).  A wrong coefficient, a wrong sign of the prior-stage term or a
    B^T factor other than dt leaves a term of the size of dt ||F x_s|| and breaks it."""
    C, H, x_start, stop = _start(fedd_lib)
    ns = NavierStokesABI(fedd_lib, ctx, C["m1"], C["mv"], NU, RHO, C["rows"], C["vals"])
    xs, hs = ns.solve("Newton", x_start, TOL, 25, RTOL_LIN)
    assert hs[-1] <= stop
    c_, A = fedd_lib.butcher_table(1)
    d = StageDevice(fedd_lib, ctx, C["m1"], C["mv"], C["rows"], C["vals"])
    SH = StageHost(fedd_lib, ctx, C["mv"], C["rows"], C["vals"])
    x = xs
    for step in range(3):
        x = d.step(x, A, stop)
        SH.check(d.stage_log[-1], stop, "steady state step %d" % (step + 1), x_ref=xs)
    Fx = SH.A @ xs[:SH.nvd] + RHO * (SH.R.N(xs[:SH.nvd]) @ xs[:SH.nvd])
    print("scale of the operator term dt ||F x_s|| = %.3e, steady residual %.2e" % (DT * np.linalg.norm(Fx), hs[-1]))
    assert d.combines == 1


# ---- error norms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["square", "cube"])
def test_stage_error(fedd_lib, ctx, which):
    m1, mv = meshes(fedd_lib, which)
    b = Blocks(fedd_lib, ctx, m1, mv, seed=5)
    c, L = ctx, fedd_lib
    U, _ = b.three_stages()
    cur = b.rng.standard_normal(b.n)
    c.solution_set(cur)
    vec = {0: U[0], 1: U[1], 2: U[2], -1: cur}
    eps = 2.0 ** -52
    for ja, jb in ((0, 1), (2, 0), (1, -1), (-1, 2)):
        dvec = vec[ja] - vec[jb]
        # Euclidean: any order of summing n non-negative terms d_i^2 is within n * 2^-52 of any other, relatively (each of the
        # at most n - 1 additions and the square contribute a factor 1 + delta, |delta| <= 2^-53); the root halves it
        e = c.stage_error(L.STAGE_ERR_EUCLIDEAN, -1, ja, jb)
        want = float(np.sqrt(np.sum(dvec * dvec)))
        print("%s (%d, %d): Euclidean %.17g numpy %.17g" % (which, ja, jb, e, want))
        assert abs(e - want) <= b.n * eps * want
        assert e == c.stage_error(L.STAGE_ERR_EUCLIDEAN, -1, ja, jb)
        # L2: the terms d_i (M d)_i with the device's own row sums (fedd_matrix_apply of d, bit for bit the kernel's), summed
        # in another order: the terms have both signs, so the bound is relative to the sum of their magnitudes
        Md = c.matrix_apply(SLOT_M, dvec[:b.nvd])
        terms = dvec[:b.nvd] * Md
        e2 = c.stage_error(L.STAGE_ERR_L2, SLOT_M, ja, jb)
        want2 = float(np.sum(terms))
        print("%s (%d, %d): L2 squared %.17g numpy %.17g" % (which, ja, jb, e2 * e2, want2))
        assert want2 > 0.0
        assert abs(e2 * e2 - want2) <= b.nvd * eps * float(np.sum(np.abs(terms))) + 4 * eps * want2
        assert e2 == c.stage_error(L.STAGE_ERR_L2, SLOT_M, ja, jb)
    for kind in (L.STAGE_ERR_EUCLIDEAN, L.STAGE_ERR_L2):
        assert c.stage_error(kind, SLOT_M, 1, 1) == 0.0
        assert c.stage_error(kind, SLOT_M, -1, -1) == 0.0
    # -1 is the current solution: equal to stage 0 when that is what the solution holds
    c.solution_set(U[0])
    assert c.stage_error(L.STAGE_ERR_EUCLIDEAN, -1, -1, 0) == 0.0
    assert c.stage_error(L.STAGE_ERR_EUCLIDEAN, -1, -1, 1) == c.stage_error(L.STAGE_ERR_EUCLIDEAN, -1, 0, 1)


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_entry_and_the_cause_and_change_nothing(fedd_lib, ctx):
    m1, mv = meshes(fedd_lib, "square")
    b = Blocks(fedd_lib, ctx, m1, mv, seed=6)
    c, L = ctx, fedd_lib
    x = b.rng.standard_normal(b.n)
    b.operator(x)
    c.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)
    c.solution_set(x)
    with pytest.raises(L.FeddError, match="fedd_stage_push: no open step"):
        c.stage_push(SLOT_F)
    for bad in (1, 9):
        with pytest.raises(L.FeddError, match="fedd_stage_begin: max_stages must be 2 .. 8"):
            c.stage_begin(bad)
    assert c.stage_info() == (0, 0, 0, 0)
    c.stage_begin(2)
    with pytest.raises(L.FeddError, match="fedd_stage_rhs: no stages"):
        c.stage_rhs(SLOT_M, SLOT_BT, [-0.1])
    with pytest.raises(L.FeddError, match="fedd_stage_push: slot 3 is empty"):
        c.stage_push(3)
    c.stage_push(SLOT_F)
    nnz = c.matrix_get(SLOT_F).nnz
    state = (2, 1, nnz, b.n)
    with pytest.raises(L.FeddError, match="fedd_stage_push: slot 0 holds another pattern"):
        c.stage_push(SLOT_A)                                    # the DIAG slot 0 after the FULL slot 4
    assert c.stage_info() == state
    for bad in ([], [-0.1, -0.2]):
        with pytest.raises(L.FeddError, match=r"fedd_stage_rhs: n_prior must be 1 .. count = 1"):
            c.stage_rhs(SLOT_M, SLOT_BT, bad)
    with pytest.raises(L.FeddError, match="fedd_stage_rhs: slot_bt < 0 needs every coeff_bt to be 0.0"):
        c.stage_rhs(SLOT_M, -1, [-0.1], [0.25])
    with pytest.raises(L.FeddError, match="fedd_stage_rhs: slot 3 is empty"):
        c.stage_rhs(3, SLOT_BT, [-0.1])
    with pytest.raises(L.FeddError, match="fedd_stage_rhs: slot 3 is empty"):
        c.stage_rhs(SLOT_M, 3, [-0.1], [0.25])
    with pytest.raises(L.FeddError, match="fedd_stage_rhs: B\\^T in slot 1 has"):
        c.stage_rhs(SLOT_M, SLOT_B, [-0.1], [0.25])             # B in the place of B^T: the wrong shape
    with pytest.raises(L.FeddError, match="fedd_stage_error: stage indices"):
        c.stage_error(L.STAGE_ERR_EUCLIDEAN, -1, 0, 1)
    with pytest.raises(L.FeddError, match="fedd_stage_error: unknown kind"):
        c.stage_error(5, -1, 0, 0)
    c.stage_push(SLOT_F)
    with pytest.raises(L.FeddError, match="fedd_stage_push: the step was opened for 2 stages and holds 2"):
        c.stage_push(SLOT_F)
    assert c.stage_info() == (2, 2, nnz, b.n)
    # nothing above touched the store or the right-hand side
    c.rhs_set(np.full(b.n, 2.0))
    with pytest.raises(L.FeddError, match="n_prior"):
        c.stage_rhs(SLOT_M, SLOT_BT, [0.1, 0.2, 0.3])
    np.testing.assert_array_equal(c.rhs_get(), np.full(b.n, 2.0))
    np.testing.assert_array_equal(c.stage_get(0)[1], x)
    # a new mesh releases the store
    c.mesh_set_dict(mv)
    assert c.stage_info() == (0, 0, 0, 0)
    for call in (lambda: c.stage_push(SLOT_F), lambda: c.stage_rhs(SLOT_M, SLOT_BT, [-0.1]),
                 lambda: c.stage_error(L.STAGE_ERR_EUCLIDEAN, -1, 0, 0)):
        with pytest.raises(L.FeddError, match="no open step"):
            call()

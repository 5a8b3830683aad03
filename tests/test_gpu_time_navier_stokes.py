"""Unsteady Navier-Stokes at the ABI level: three BDF2 steps with a BDF1 start on the 2D P2 / P1 channel of
tests/test_gpu_navier_stokes.py at its smallest size (4 x 4), Dirichlet values constant in time.  Per step the device runs

    slot 6 <- (cm * M[5]) + (1.0 * A[0])       fedd_matrix_combine + fedd_matrix_store, when (cm, ca) changed: twice in the run
    history, rhs <- [M t ; 0]                  fedd_solution_set + fedd_multistep_advance
    per nonlinear iteration                    fedd_assemble_advection(kind, rho, slot_add = 6, slot_out = 4), fedd_block_merge,
                                               residual = fedd_spmv(x) - rhs, Dirichlet rows, GMRES

Reference: the same scheme on the host with oracle matrices, the restated advection (tests/test_navier_stokes_abi.py) and a
sparse direct solve per Newton step.

Bar.  That of test_flow_where_advection_matters_and_no_symbolic_rebuild, taken over with its procedure: with e = x - x_ref of one
step, r(x) - r(x_ref) = J e + N(e) e on the free rows, so ||e|| <= 1.05 ||J^-1||_2 (||r(x)|| + ||r(x_ref)||), J the Jacobian of
the step's system, cm M + A + rho (N + W), at the reference, ||J^-1||_2 from its sparse factors.  Two things differ from the
steady case and are accounted for inside the same bracket, nothing is widened:
  * both sides are driven to the rounding floor, which is an ABSOLUTE residual here (the first residual of a later step is
    small, so a relative one would mean nothing): ||r(x)|| <= TOL * ||r_0||, r_0 the steady residual of the start state
    (boundary values, zero inside), formed on the host;
  * the comparison is per step: the reference of step k starts from the states the DEVICE returned for the steps before it
    (the host forms M (c_0 x_{k-1} + c_1 x_{k-2}) from them itself), so no error of an earlier step has to be carried through
    the bound, while a wrong coefficient, a wrong shift of the device's own history or a wrong mass block still lands in x_k."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import fedd_oracle as fo
from test_gpu_navier_stokes import NavierStokesABI, _channel, SLOT_A, SLOT_B, SLOT_BT, SLOT_F
from test_gpu_parity import oracle_mesh
from test_navier_stokes_abi import Restatement

pytestmark = pytest.mark.gpu

SLOT_M, SLOT_AT = 5, 6
NU, RHO, DT = 0.01, 1.0, 0.05
TOL, RTOL_LIN = 1e-11, 1e-13
BDF = {1: (1.0, [1.0]), 2: (1.5, [2.0, -0.5])}            # TimeSteppingTools.cpp:493-515: mass coefficient, history coefficients


def profile(y):
    return 6.0 * y * y * (1.0 - y) + np.sin(np.pi * y)


def coefficients(step, dt=DT):
    cm, hist = BDF[1 if step == 0 else 2]
    return cm / dt, [h / dt for h in hist]


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


_CASE = {}


def case(fedd_lib):
    if not _CASE:
        m1, mv, rows, vals = _channel(fedd_lib, 4, profile)
        _CASE.update(m1=m1, mv=mv, rows=rows, vals=vals, host=Host(fedd_lib, m1, mv, rows, vals))
    return _CASE


class Host:
    """the scheme on the host: oracle matrices, restated advection, sparse direct Newton"""

    def __init__(self, fedd_lib, m1, mv, rows, vals):
        self.R = Restatement(fedd_lib, mv)
        self.A, self.BT, self.B = fo.stokes_blocks(oracle_mesh(mv), oracle_mesh(m1), RHO * NU)
        self.M = (RHO * fo.assembly_mass(oracle_mesh(mv), "Vector")).tocsr()
        self.nvd, self.n_p = self.A.shape[0], self.B.shape[0]
        self.n = self.nvd + self.n_p
        self.rows, self.vals = rows, vals
        self.free = np.ones(self.n, dtype=bool)
        self.free[rows] = False
        self.normM = abs(self.M).sum(axis=1).max()

    def K(self, x, cm, newton=False):
        u = x[:self.nvd]
        F = cm * self.M + self.A + RHO * (self.R.N(u) + (self.R.W(u) if newton else 0.0 * self.R.N(u)))
        return sp.bmat([[F, self.BT], [self.B, None]], format="csc")

    def residual(self, x, cm, b):
        r = self.K(x, cm) @ x - b
        r[self.rows] = 0.0
        return r

    def r0(self, x_start):
        """the scale of the stop: the steady residual of the start state"""
        return float(np.linalg.norm(self.residual(x_start, 0.0, np.zeros(self.n))))

    def jinv(self, x, cm):
        """||J^-1||_2 on the free rows: power iteration on J^-T J^-1 with the sparse factors, as _host_reference does"""
        lu = spla.splu(self.K(x, cm, newton=True)[self.free][:, self.free].tocsc())
        z = np.random.default_rng(3).standard_normal(int(self.free.sum()))
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

    def step(self, x0, cm, b):
        x = x0.copy()
        hist = []
        for k in range(40):
            r = self.residual(x, cm, b)
            hist.append(float(np.linalg.norm(r)))
            if k > 0 and (hist[-1] <= 1e-14 * hist[0] or (k > 2 and hist[-1] >= 0.5 * hist[-2])):   # the rounding floor
                break
            dx = np.zeros(self.n)
            dx[self.free] = spla.splu(self.K(x, cm, newton=True)[self.free][:, self.free].tocsc()).solve(-r[self.free])
            x += dx
        return x, hist

    def rhs(self, step, states):
        """[M (c_0 x_{k-1} + c_1 x_{k-2}) ; 0] from the states before step k = step + 1, newest first"""
        c = coefficients(step)[1]
        t = sum(ci * xi[:self.nvd] for ci, xi in zip(c, states))
        return np.concatenate([self.M @ t, np.zeros(self.n_p)])

    def step_after(self, step, states):
        """(x_k, ||r(x_k)||, ||J_k^-1||) of the step that follows `states`"""
        cm = coefficients(step)[0]
        x, hist = self.step(states[0], cm, self.rhs(step, states))
        return x, hist[-1], self.jinv(x, cm)


class Device(NavierStokesABI):
    """NavierStokesABI with the mass matrix in slot 5 and the time-combined velocity block in slot 6"""

    def __init__(self, fedd_lib, ctx, m1, mv, rows, vals, nu=NU, rho=RHO, dt=DT):
        super().__init__(fedd_lib, ctx, m1, mv, nu, rho, rows, vals)
        self.dt = dt
        ctx.pattern_build(self.dim, fedd_lib.BLOCK_DIAG)     # TimeProblem::assembleMassSystem: vector mass * density
        ctx.assemble(fedd_lib.FORM_MASS_VEC)
        ctx.matrix_scale(-1, rho)
        ctx.matrix_store(SLOT_M)
        self.combines, self.last, self.began = 0, None, False
        self.b = np.zeros(self.n)
        self.nl_its = []

    def combine(self, cm, ca):
        if self.last == (cm, ca):
            return
        if not self.c.matrix_combine_current(SLOT_M, cm, SLOT_A, ca):
            self.c.matrix_combine(SLOT_M, cm, SLOT_A, ca)
        self.c.matrix_store(SLOT_AT)
        self.combines += 1
        self.last = (cm, ca)

    def system(self, kind, x):
        self.c.velocity_set(x[:self.dim * self.nv])
        self.c.assemble_advection(kind, self.rho, SLOT_AT, SLOT_F)
        self.c.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)

    def residual(self, x):
        self.system(self.L.ADV_N, x)
        r = self.c.spmv(x) - self.b
        r[self.rows] = x[self.rows] - self.vals
        return r

    def advance(self, step, x):
        """combine when the coefficients changed, record x, b <- [M t ; 0]"""
        cm, coeff = coefficients(step, self.dt)
        self.combine(cm, 1.0)
        self.system(self.L.ADV_N, x)                        # the merged system the history is as long as
        if not self.began:
            self.c.multistep_begin(2)
            self.began = True
        self.c.solution_set(x)                              # fedd_block_merge has reset it
        self.c.multistep_advance(SLOT_M, coeff)
        self.b = self.c.rhs_get()
        assert not self.b[self.dim * self.nv:].any()

    def time_step(self, step, x, method, stop, after_iteration=None):
        self.advance(step, x)
        x = x.copy()
        hist = []
        for k in range(30):
            r = self.residual(x)
            hist.append(float(np.linalg.norm(r)))
            if (hist[-1] <= stop and k > 0) or k == 29:     # at least one iteration: a step that starts converged is still solved
                break
            if method == "Newton":
                self.system(self.L.ADV_NEWTON, x)
            rhs = -r
            rhs[self.rows] = 0.0
            self.c.rhs_set(rhs)
            self.c.dirichlet_rows(self.rows, -r[self.rows])
            dx, its, rel = self.linear_solve(RTOL_LIN, False)
            x += dx
            if after_iteration:
                after_iteration(step, k)
        self.nl_its.append(len(hist) - 1)
        return x, hist


def check_against(got, ref, stop, what):
    """the bar of the module docstring, step by step; got[k] = (x, residual history), ref[k] = (x_ref, ||r(x_ref)||, ||J^-1||)"""
    bounds = []
    for step, ((x, hist), (xr, rr, jinv)) in enumerate(zip(got, ref)):
        bound = 1.05 * jinv * (stop + rr)
        err = float(np.linalg.norm(x - xr))
        print("%s step %d: residuals %s ||x - x_ref|| = %.3e bound %.3e (||J^-1|| %.3e, ||r(x_ref)|| %.2e)"
              % (what, step + 1, ["%.2e" % h for h in hist], err, bound, jinv, rr))
        assert hist[-1] <= stop
        assert err <= bound
        bounds.append(bound)
    return bounds


def run_device(d, H, x_start, method, stop, after_iteration=None):
    """three steps; the reference of each from the device's earlier states"""
    got, ref, states = [], [], [x_start]
    for step in range(3):
        ref.append(H.step_after(step, states))
        x, hist = d.time_step(step, states[0], method, stop, after_iteration=after_iteration)
        got.append((x, hist))
        states = [x] + states[:1]
    return got, ref


def test_three_bdf2_steps_against_the_host_reference_and_launch_counts(fedd_lib, ctx):
    C = case(fedd_lib)
    H = C["host"]
    x_start = np.zeros(H.n)
    x_start[C["rows"]] = C["vals"]
    d = Device(fedd_lib, ctx, C["m1"], C["mv"], C["rows"], C["vals"])
    ctx.timing_enable(True)
    ctx.timing_reset()
    launches = {}

    def record(step, k):
        t = ctx.timing_get()
        launches[(step, k)] = (t["symbolic"][1], t["multistep_state"][1], t["block_apply"][1])

    stop = TOL * H.r0(x_start)
    got_n, ref_n = run_device(d, H, x_start, "Newton", stop, after_iteration=record)
    ctx.timing_enable(False)
    print("launches (symbolic, multistep_state, block_apply) after (step, iteration):", launches, "combines", d.combines,
          "Newton iterations per step", d.nl_its)
    bound_n = check_against(got_n, ref_n, stop, "Newton")
    # the coefficients changed once: BDF1 for the first step, BDF2 afterwards
    assert d.combines == 2
    # one symbolic build for the advection structures (node pattern, gather lists, tables), in the first iteration.  The other
    # launches of that class are the pattern copies of the two fedd_matrix_combine calls into the system slot, which the mass
    # matrix (first step) and the merged matrix (second step) had occupied: timestep.hip counts that copy as symbolic.  So the
    # count is exactly 2 through the first step and exactly 3 from the second step on.
    first, last = launches[(0, 0)], launches[max(launches)]
    assert first[0] == 2 and last[0] == 3
    assert all(launches[k][0] == first[0] for k in launches if k[0] == 0)
    assert all(launches[k][0] == last[0] for k in launches if k[0] >= 1)
    assert last[1] == 3 and last[2] == 3                    # one history kernel and one block apply per step
    # fixed point reaches the same states, by the same bar
    d2 = Device(fedd_lib, ctx, C["m1"], C["mv"], C["rows"], C["vals"])
    got_f, ref_f = run_device(d2, H, x_start, "FixedPoint", stop)
    print("fixed-point iterations per step", d2.nl_its, "Newton", d.nl_its)
    bound_f = check_against(got_f, ref_f, stop, "FixedPoint")
    assert d2.combines == 2 and sum(d2.nl_its) > sum(d.nl_its)
    # the same solution within the nonlinear tolerance used.  Step 1 starts from the same state on both sides, so both results
    # lie within their bounds of ONE reference.  From step 2 on each run's reference starts from that run's own earlier states:
    # the two references differ by what the difference D of those states does to the right-hand side, M (c_0 D_{k-1} + c_1
    # D_{k-2}), i.e. by at most 1.05 ||J^-1|| ||M||_inf (|c_0| d_{k-1} + |c_1| d_{k-2}) through the same argument, added to the
    # two bounds of the step.
    assert np.array_equal(ref_n[0][0], ref_f[0][0])
    d = [0.0, 0.0]                                          # bounds on the difference of the two runs' states, newest first
    for step in range(3):
        c = coefficients(step)[1]
        carried = 1.05 * ref_n[step][2] * H.normM * sum(abs(ci) * di for ci, di in zip(c, d))
        bound = bound_n[step] + bound_f[step] + carried
        err = float(np.linalg.norm(got_f[step][0] - got_n[step][0]))
        print("fixed point vs Newton after step %d: %.3e bound %.3e" % (step + 1, err, bound))
        assert err <= bound
        d = [bound, d[0]]


def test_steady_state_stays_where_it_is(fedd_lib, ctx):
    """An invariant that owes nothing to the restatement's scheme: started from the converged steady solution of the device,
    three BDF2 steps leave it there, because 1.5 - 2 + 0.5 = 0 and, for the BDF1 start, 1 - 1 = 0.  With x_s the steady state,
    r_time(x_s) = r_steady(x_s) + M (c_0 (x_s - x_{k-1}) + c_1 (x_s - x_{k-2})), so the bar of the module docstring applies with
    x_ref = x_s and ||r(x_ref)|| <= ||r_steady(x_s)|| + ||M (c_0 (x_s - x_{k-1}) + c_1 (x_s - x_{k-2}))||, the second term formed
    on the host from the states the device returned (exactly 0 in the first step).  Wrong coefficients or a wrong shift order
    leave a term of size ||M x_s|| / dt in the residual and break it.  (||J^-1|| is the host's, at x_s.)"""
    C = case(fedd_lib)
    H = C["host"]
    x_start = np.zeros(H.n)
    x_start[C["rows"]] = C["vals"]
    ns = NavierStokesABI(fedd_lib, ctx, C["m1"], C["mv"], NU, RHO, C["rows"], C["vals"])
    stop = TOL * H.r0(x_start)
    xs, hs = ns.solve("Newton", x_start, TOL, 25, RTOL_LIN)
    assert hs[-1] <= stop
    d = Device(fedd_lib, ctx, C["m1"], C["mv"], C["rows"], C["vals"])
    got, ref, states = [], [], [xs]
    for step in range(3):
        drift = H.rhs(step, [xs - st for st in states])
        ref.append((xs, hs[-1] + float(np.linalg.norm(drift)), H.jinv(xs, coefficients(step)[0])))
        x, hist = d.time_step(step, states[0], "Newton", stop)
        got.append((x, hist))
        states = [x] + states[:1]
    print("steady residuals", ["%.2e" % h for h in hs], "scale of the mass term ||M x_s|| / dt = %.3e"
          % (np.linalg.norm(H.M @ xs[:H.nvd]) / DT))
    check_against(got, ref, stop, "steady state")
    assert d.combines == 2 and all(k >= 1 for k in d.nl_its)

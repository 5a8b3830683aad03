"""Newmark state and steps on the device (fedd_newmark_*, fedd_matrix_combine, fedd_rhs_axpy, fedd_dirichlet_rhs; timestep.hip)
for unsteady linear elasticity on the structured cube: mu, nu, density and the volume force of the reference's unsteadyLinElas
settings (tests/golden/unsteadylinelas_xml/parametersProblem.xml), load ramped up over T_RAMP, dt = 0.025, beta = 1/4, gamma = 1/2.

  (a) the vector part of a step against the numpy restatement of the header's operation order, bit for bit
  (b) every step's solve against scipy's direct solve of the system the device holds (1e-10 max|x|), with
      fedd_cg_x0 and fedd_gmres_x0, the right-hand side against M t + f, and (e) one symbolic / one Schwarz setup over the loop
  (c) the whole loop against an independent restatement (oracle matrices, scipy direct solves)
  (d) energy conservation after the load is switched off, no restatement involved in the device's figure

The bounds of (c) and (d) are measured, not chosen: the restatement runs once with direct solves and once with scipy's CG
stopped at the device's rtol (relative to ||b - A x_0||, x_0 = the previous step, as fedd_cg_x0 counts); their difference is
what a tolerance-limited solve does to the steps, and the device, whose iterates differ, gets ten times that.
test_restatement_bounds_cpu prints those figures and checks the scheme itself (direct solves) stays below the energy bound;
the figures it gave are recorded next to FACTOR below."""
import numpy as np
import pytest
import scipy.sparse as sp

import fedd_oracle as fo

MU, NU, RHO, FORCE = 0.5e6, 0.4, 1000.0, -7.0
DT, BETA, GAMMA = 0.025, 0.25, 0.5
T_RAMP = 0.1
LAM = 2.0 * MU * NU / (1.0 - 2.0 * NU)
LOOP_RTOL = 1e-10          # the device's rtol in (c) and (d)
FACTOR = 10.0              # device bound = FACTOR * (restatement with CG at LOOP_RTOL  vs  restatement with direct solves)

# measured by test_restatement_bounds_cpu (informative; the tests compute them again):
#   M = 4 : loop difference CG vs direct 1.4e-11 (u) 8.4e-12 (v) 1.1e-10 (w); energy drift CG 6.6e-12, direct 2.6e-15
#   M = 12: loop difference CG vs direct 2.4e-11 (u) 1.6e-11 (v) 7.7e-10 (w); energy drift CG 1.3e-12, direct 1.7e-14


def coefs(dt, beta, gamma):
    """the coefficients exactly as include/fedd_hip.h writes them"""
    return dict(cuu=1.0 / ((dt * dt) * beta), cuv=1.0 / (dt * beta), cuw=(0.5 - beta) / beta,
                cvu=gamma / (dt * beta), cvv=1.0 - (gamma / beta), cvw=(dt * (beta - (0.5 * gamma))) / beta)


def advance_numpy(k, u, un, v, w, first):
    """the header's operation order: every product and every sum is its own numpy operation"""
    if not first:
        d = u - un
        v1 = ((k["cvu"] * d) + (k["cvv"] * v)) + (k["cvw"] * w)
        w1 = ((k["cuu"] * d) - (k["cuv"] * v)) - (k["cuw"] * w)
        v, w = v1, w1
    t = ((k["cuu"] * u) + (k["cuv"] * v)) + (k["cuw"] * w)
    return u.copy(), v, w, t


def ramp(t):
    return FORCE * min(t / T_RAMP, 1.0)


def ramp_then_off(t):
    return ramp(t) if t <= 2.0 * DT + 1e-12 else 0.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# the independent restatement: oracle matrices, numpy vectors, scipy solves
# ---------------------------------------------------------------------------------------------------------------------------
def scipy_cg(A, b, x0, rtol, max_it=20000):
    """scipy's CG on the symmetric free-free system, stopped where fedd_cg_x0 stops: ||r|| <= rtol * ||b - A x_0|| (scipy's
    own relative tolerance refers to ||b||, so the bound is handed over as the absolute one)"""
    import inspect
    from scipy.sparse.linalg import cg
    stop = rtol * np.linalg.norm(b - A @ x0)
    rel_key = "rtol" if "rtol" in inspect.signature(cg).parameters else "tol"
    x, info = cg(A, b, x0=x0.copy(), atol=stop, maxiter=max_it, **{rel_key: 0.0})
    assert info == 0, info
    return x


_REST = {}


class Restatement:
    def __init__(self, fedd_lib, M):
        from test_gpu_parity import oracle_mesh
        om = oracle_mesh(fedd_lib.structured_mesh(3, 1, M))
        self.M = (RHO * fo.assembly_mass(om, "Vector")).tocsr()
        self.K = fo.assembly_linelas(om, LAM, MU).tocsr()
        fr = fo.assembly_rhs(om, [0.0, 1.0, 0.0], "Vector", 0)
        gd = (3 * om.gid_rep[:, None] + np.arange(3)[None, :]).ravel()
        self.f_unit = fo.export_add(fr, gd, 3 * om.n_global)
        flags = np.zeros(om.n_global, dtype=np.int32)
        flags[om.gid_uni] = om.flag_uni
        self.is_dir = fo.dirichlet_rows(flags, (2,), dofs=3)
        k = coefs(DT, BETA, GAMMA)
        A = (k["cuu"] * self.M + self.K).tocsr()
        self.A_bc, _ = fo.set_dirichlet(A, np.zeros(A.shape[0]), self.is_dir, 0.0)
        free = np.nonzero(~self.is_dir)[0]
        self.free = free
        self.A_ff = A[free][:, free].tocsr()
        self._runs = {}

    def run(self, n_steps, load, solver):
        """states[j] = (u_j, v_j, w_j) for j = 0 ... n_steps (consistent triples: v_j, w_j follow from the advance after step j)"""
        key = (n_steps, load.__name__, solver)
        if key in self._runs:
            return self._runs[key]
        k = coefs(DT, BETA, GAMMA)
        n = self.M.shape[0]
        u, un, v, w = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        first = True
        states = []
        for step in range(n_steps + 1):
            un, v, w, t = advance_numpy(k, u, un, v, w, first)
            first = False
            states.append((un.copy(), v.copy(), w.copy()))
            if step == n_steps:
                break
            rhs = self.M @ t + load(step * DT + DT) * self.f_unit
            rhs[self.is_dir] = 0.0
            if solver == "direct":
                u = fo.direct_solve(self.A_bc, rhs)
            else:
                u = np.zeros(n)
                u[self.free] = scipy_cg(self.A_ff, rhs[self.free], un[self.free], solver)
        self._runs[key] = states
        return states

    def energy(self, u, v):
        return 0.5 * (v @ (self.M @ v)) + 0.5 * (u @ (self.K @ u))


def restatement(fedd_lib, M):
    if M not in _REST:
        _REST[M] = Restatement(fedd_lib, M)
    return _REST[M]


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def loop_bounds(R):
    """(difference of the five-step loop CG vs direct per state vector, relative to the vector's largest entry)"""
    sd, sc = R.run(5, ramp, "direct")[-1], R.run(5, ramp, LOOP_RTOL)[-1]
    return [rel(sc[i], sd[i]) for i in range(3)]


def energy_drift(energies):
    """states 3 ... 10: the load is off from step 3 on, so E_4 = E_3, ... (E_{n+1} - E_n = (u_{n+1} - u_n) . (f_{n+1} + f_n) / 2)"""
    e = np.asarray(energies[3:11])
    return np.abs(e - e[0]).max() / e[0]


def energy_bounds(R):
    out = {}
    for solver in ("direct", LOOP_RTOL):
        st = R.run(10, ramp_then_off, solver)
        out[solver] = energy_drift([R.energy(s[0], s[1]) for s in st])
    return out


@pytest.mark.parametrize("M", [4, 12])
def test_restatement_bounds_cpu(fedd_lib, M):
    """no GPU: the measured bounds, and the restatement alone (direct solves: the scheme and its rounding) below the energy bound"""
    R = restatement(fedd_lib, M)
    lb = loop_bounds(R)
    eb = energy_bounds(R)
    print("M", M, "loop CG vs direct: u %.2e v %.2e w %.2e" % tuple(lb), "energy drift: CG %.2e direct %.2e" % (eb[LOOP_RTOL], eb["direct"]))
    assert all(0.0 < x < 1e-4 for x in lb)
    assert eb["direct"] <= FACTOR * eb[LOOP_RTOL]
    st = R.run(10, ramp_then_off, "direct")
    assert R.energy(st[3][0], st[3][1]) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------------
class Device:
    """the sequence a time loop over the C ABI runs (what the facade's DAESolverInTime would issue)"""

    def __init__(self, fedd_lib, M, timing=False):
        L = self.L = fedd_lib
        c = self.c = L.Context(device=0)
        self.m = L.structured_mesh(3, 1, M)
        c.mesh_set_dict(self.m)
        c.pattern_build(3, L.BLOCK_FULL)
        c.assemble(L.FORM_LINELAS, [LAM, MU])
        c.matrix_store(1)
        c.assemble_rhs([0.0, 1.0, 0.0])
        self.f_unit = c.rhs_get()
        c.pattern_build(3, L.BLOCK_DIAG)                  # TimeProblem::assembleMassSystem: mass, scaled by the density
        c.assemble(L.FORM_MASS_VEC)
        c.matrix_scale(-1, RHO)
        c.matrix_store(0)
        self.Mdev = c.matrix_get(0)
        self.Kdev = c.matrix_get(1)
        self.n = self.Mdev.shape[0]
        self.k = coefs(DT, BETA, GAMMA)
        self.step_no = 0
        self.began = False
        self.combines = 0
        if timing:
            c.timing_enable(1)
            c.timing_reset()

    def close(self):
        self.c.close()

    def step(self, load, solver="cg", rtol=1e-13, check=False):
        c, L, k = self.c, self.L, self.k
        fresh = not c.matrix_combine_current(0, k["cuu"], 1, 1.0)
        if fresh:
            c.matrix_combine(0, k["cuu"], 1, 1.0)
            self.combines += 1
        if not self.began:
            c.newmark_begin()
            self.began = True
            first = True
        else:
            first = False
        out = {}
        if check:
            u = c.solution_get()
            un, v, w = c.newmark_get()
            e_un, e_v, e_w, t = advance_numpy(k, u, un, v, w, first)
        c.newmark_advance(0, DT, BETA, GAMMA, 1.0)
        f = load(self.step_no * DT + DT)
        c.rhs_axpy(f, self.f_unit)
        if check:
            g_un, g_v, g_w = c.newmark_get()
            assert np.array_equal(bits(g_un), bits(e_un)) and np.array_equal(bits(g_v), bits(e_v)) and np.array_equal(bits(g_w), bits(e_w))
            b_pre = c.rhs_get()
            expect = (self.Mdev @ t) + (f * self.f_unit)
            tol = 1e-14 * np.abs(self.Mdev).sum(axis=1).max() * np.abs(t).max()          # the bound of the block apply (test_gpu_time_combine.py)
            out["rhs_err"], out["rhs_tol"] = np.abs(b_pre - expect).max(), tol
            assert out["rhs_err"] <= tol, (self.step_no, out)
        if fresh:
            c.dirichlet([2], np.zeros(3))
            c.schwarz_set_target(8, 1.0)
            c.schwarz_setup(1, L.COMBINE_FULL)
        else:
            c.dirichlet_rhs([2], np.zeros(3))
        if check:
            rowptr, col, val, _ = c.csr_get()
            out["A"] = sp.csr_matrix((val, col, rowptr), shape=(self.n, self.n))
            out["b"] = c.rhs_get()
        if solver == "cg":
            x, its, relres = c.cg_x0(None, None, rtol=rtol, max_it=3000, use_prec=True)
        else:
            x, its, relres = c.gmres_x0(None, None, rtol=rtol, max_it=1000, restart=100, use_prec=True)
        out.update(x=x, its=its, relres=relres)
        self.step_no += 1
        return out

    def final_state(self):
        """one more advance: the (u, v, w) triple of the last solved step"""
        self.c.newmark_advance(0, DT, BETA, GAMMA, 1.0)
        return self.c.newmark_get()


@pytest.mark.gpu
@pytest.mark.parametrize("dt,beta,gamma", [(DT, BETA, GAMMA), (0.0125, 0.3, 0.6)])
@pytest.mark.parametrize("M", [4, 12])
def test_vector_part_bit_for_bit(fedd_lib, M, dt, beta, gamma):
    d = Device(fedd_lib, M)
    try:
        c, n = d.c, d.n
        assert n % 2 == 1                                   # the scalar tail row of the 16-byte accesses is exercised
        c.matrix_combine(0, 1.0, 1, 1.0)                    # a system of the elasticity's size
        k = coefs(dt, beta, gamma)
        rng = np.random.default_rng(7)
        u, un, v, w = (rng.standard_normal(n) * s for s in (1e-3, 1e-3, 1e-1, 10.0))
        c.solution_set(u)
        c.newmark_set(un, v, w)
        c.newmark_advance(0, dt, beta, gamma, 0.5)
        e_un, e_v, e_w, t = advance_numpy(k, u, un, v, w, False)
        g_un, g_v, g_w = c.newmark_get()
        for name, g, e in (("u_n", g_un, e_un), ("v", g_v, e_v), ("w", g_w, e_w)):
            print("M", M, name, "differing entries", int(np.count_nonzero(bits(g) != bits(e))))
            assert np.array_equal(bits(g), bits(e)), name
        assert np.array_equal(bits(c.solution_get()), bits(u))
        expect = 0.5 * (d.Mdev @ t)
        tol = 0.5 * 1e-14 * np.abs(d.Mdev).sum(axis=1).max() * np.abs(t).max()
        err = np.abs(c.rhs_get() - expect).max()
        print("rhs err %.3e tol %.3e" % (err, tol))
        assert err <= tol
        # the first-step branch: v and w stay zero, u_n <- u, t = cuu * u
        c.solution_set(u)
        c.newmark_begin()
        b_un, b_v, b_w = c.newmark_get()
        assert np.array_equal(bits(b_un), bits(u)) and not b_v.any() and not b_w.any()
        c.solution_set(2.0 * u)                             # a first step does not read u_n
        c.newmark_advance(0, dt, beta, gamma, 1.0)
        g_un, g_v, g_w = c.newmark_get()
        assert np.array_equal(bits(g_un), bits(2.0 * u)) and np.array_equal(bits(g_v), bits(np.zeros(n))) and np.array_equal(bits(g_w), bits(np.zeros(n)))
        t1 = advance_numpy(k, 2.0 * u, u, np.zeros(n), np.zeros(n), True)[3]
        assert np.abs(c.rhs_get() - d.Mdev @ t1).max() <= 1e-14 * np.abs(d.Mdev).sum(axis=1).max() * np.abs(t1).max()
        # ... and the step after it is not a first step
        c.solution_set(u)
        c.newmark_advance(0, dt, beta, gamma, 1.0)
        e_un, e_v, e_w, _ = advance_numpy(k, u, 2.0 * u, np.zeros(n), np.zeros(n), False)
        g_un, g_v, g_w = c.newmark_get()
        assert np.array_equal(bits(g_un), bits(e_un)) and np.array_equal(bits(g_v), bits(e_v)) and np.array_equal(bits(g_w), bits(e_w))
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["cg", "gmres"])
@pytest.mark.parametrize("M", [4, 12])
def test_steps_against_direct_solve(fedd_lib, M, solver):
    d = Device(fedd_lib, M, timing=True)
    try:
        for step in range(5):
            o = d.step(ramp, solver=solver, rtol=1e-13, check=True)
            xd = fo.direct_solve(o["A"], o["b"])
            err = np.abs(o["x"] - xd).max() / np.abs(xd).max()
            print("M", M, solver, "step", step, "its", o["its"], "relres %.2e" % o["relres"], "err vs direct %.2e" % err,
                  "rhs err %.2e tol %.2e" % (o["rhs_err"], o["rhs_tol"]))
            assert err <= 1e-10
            assert o["relres"] <= 1e-13
        # (e) the combine, the pattern copy and both setups happen once for the one coefficient set
        tm = d.c.timing_get()
        info = d.c.schwarz_reuse_info()
        print("combines", d.combines, "symbolic", tm["symbolic"][1], "schwarz_setup", tm["schwarz_setup"][1], "spmv_setup", tm["spmv_setup"][1],
              "newmark", tm["newmark_state"][1], "block_apply", tm["block_apply"][1], info)
        assert d.combines == 1
        assert tm["symbolic"][1] == 1 and tm["schwarz_setup"][1] == 1
        assert tm["spmv_setup"][1] <= 1
        assert tm["newmark_state"][1] == 5 and tm["block_apply"][1] == 5
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [4, 12])
def test_whole_loop_against_restatement(fedd_lib, M):
    R = restatement(fedd_lib, M)
    measured = loop_bounds(R)                               # recorded above: 1e-11 ... 8e-10 by vector
    ref = R.run(5, ramp, "direct")[-1]
    d = Device(fedd_lib, M)
    try:
        for step in range(5):
            d.step(ramp, solver="cg", rtol=LOOP_RTOL)
        got = d.final_state()
        for name, g, e, mval in zip("uvw", got, ref, measured):
            err = rel(g, e)
            print("M", M, name, "device vs restatement %.2e" % err, "measured CG-vs-direct %.2e" % mval, "bound %.2e" % (FACTOR * mval))
            assert err <= FACTOR * mval                     # ten times the measured effect of a solve stopped at LOOP_RTOL
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [4, 12])
def test_energy_is_conserved_after_the_load(fedd_lib, M):
    R = restatement(fedd_lib, M)
    bound = FACTOR * energy_bounds(R)[LOOP_RTOL]            # recorded above: CG drift 1e-12 ... 7e-12, times ten
    d = Device(fedd_lib, M)
    try:
        energies = [0.0]                                    # state 0: u = v = 0
        for step in range(10):
            d.step(ramp_then_off, solver="cg", rtol=LOOP_RTOL)
            if step > 0:                                    # the advance inside step() completed the triple of the step before
                u, v, _ = d.c.newmark_get()
                energies.append(0.5 * (v @ (d.Mdev @ v)) + 0.5 * (u @ (d.Kdev @ u)))
        u, v, _ = d.final_state()
        energies.append(0.5 * (v @ (d.Mdev @ v)) + 0.5 * (u @ (d.Kdev @ u)))
        assert len(energies) == 11
        drift = energy_drift(energies)
        print("M", M, "energies", ["%.6e" % e for e in energies], "drift %.2e bound %.2e" % (drift, bound))
        assert energies[3] > 0.0
        assert drift <= bound
    finally:
        d.close()

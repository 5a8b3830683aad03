"""FROSch "Level Combination" = "Multiplicative" inside every apply (fedd_schwarz_set_level_combination): the operator
z = (I - Pc A) M1^-1 r against its composition from the additive apply, the coarse level and the SpMV of the same context; the
coarse-orthogonality it leaves; the additive apply untouched; solves of the three GMRES forms against the oracle's restatement
(start x_0 = Pc b, the reference's pre-apply, LinearSolver_def.hpp:98-104); restarts at 1e-12; the errors; thread ranks; the
facade's key."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import fedd_oracle as fo
from test_gpu_parity import oracle_mesh
from test_gpu_two_level import laplace_setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "laplace_xml")


def elasticity_setup(fedd_lib, c, M):
    m = fedd_lib.structured_mesh(3, 1, M)
    c.mesh_set_dict(m)
    c.pattern_build(3, fedd_lib.BLOCK_FULL)
    mu, nu = 1.0, 0.3
    lam = 2.0 * mu * nu / (1.0 - 2.0 * nu)
    c.assemble(fedd_lib.FORM_LINELAS, [lam, mu])
    c.assemble_rhs([0.0, 1.0, 0.0])
    c.dirichlet([2], [0.0, 0.0, 0.0])
    om = oracle_mesh(m)
    A_bc, rhs_bc, _, _, flags = fo.linelas_problem(om, mu, nu)
    return m, om, A_bc, rhs_bc, fo.dirichlet_rows(flags, (2,), dofs=3)


def coarse_kind(fedd_lib, kind):
    return {"q1": fedd_lib.COARSE_Q1, "gdsw": fedd_lib.COARSE_GDSW, "rgdsw": fedd_lib.COARSE_RGDSW}[kind]


CASES = [("laplace", 3, 12, "q1", 27, 0), ("laplace", 3, 12, "gdsw", 8, 0), ("laplace", 3, 12, "rgdsw", 27, 0),
         ("laplace", 2, 24, "q1", 36, 0), ("laplace", 2, 24, "gdsw", 16, 0),
         ("elasticity", 3, 8, "q1", 8, 0), ("elasticity", 3, 8, "gdsw", 8, 0), ("elasticity", 3, 8, "gdsw", 8, 1),
         ("elasticity", 3, 9, "rgdsw", 27, 1)]


@pytest.mark.parametrize("combine", ["restricted", "averaging"])
@pytest.mark.parametrize("problem,dim,M,kind,cells,rot", CASES)
def test_multiplicative_operator_identity(fedd_lib, problem, dim, M, kind, cells, rot, combine):
    """z_mult = y1 - Pc (A y1) with y1 = z_add - Pc r, every piece from the same context (1e-12 of max |z|); the result
    is coarse-orthogonal, ||Pc A z_mult|| <= 1e-9 ||Pc A y1||; switching back gives the additive apply bit for bit."""
    c = fedd_lib.Context(device=0)
    try:
        if problem == "laplace":
            laplace_setup(fedd_lib, c, dim, M)
            c.schwarz_set_target(27 if dim == 3 else 9, 1.0)
        else:
            elasticity_setup(fedd_lib, c, M)
            c.schwarz_set_target(8, 1.0)
            c.set_option("gdsw_rotations", rot)
        c.schwarz_set_coarse(cells)
        c.set_option("gdsw_tol", 1e-13)
        cmb = {"restricted": fedd_lib.COMBINE_RESTRICTED, "averaging": fedd_lib.COMBINE_AVERAGING}[combine]
        c.schwarz_setup(1, cmb, two_level=1, coarse_kind=coarse_kind(fedd_lib, kind))
        assert c.schwarz_get_level_combination() == fedd_lib.LEVELS_ADDITIVE
        n = c.csr_sizes()[0]
        r = np.random.default_rng(11).standard_normal(n)
        z_add = c.schwarz_apply(r)
        c.schwarz_set_level_combination(fedd_lib.LEVELS_MULTIPLICATIVE)
        assert c.schwarz_get_level_combination() == fedd_lib.LEVELS_MULTIPLICATIVE
        z_mult = c.schwarz_apply(r)
        y1 = z_add - c.schwarz_coarse_apply(r)
        pc_ay1 = c.schwarz_coarse_apply(c.spmv(y1))
        want = y1 - pc_ay1
        scale = np.abs(z_mult).max()
        assert scale > 0 and np.abs(pc_ay1).max() > 1e-6 * scale      # the coarse correction is not negligible here
        np.testing.assert_allclose(z_mult, want, rtol=0, atol=1e-12 * scale)
        left = np.linalg.norm(c.schwarz_coarse_apply(c.spmv(z_mult)))
        assert left <= 1e-9 * np.linalg.norm(pc_ay1), left / np.linalg.norm(pc_ay1)
        c.schwarz_set_level_combination(fedd_lib.LEVELS_ADDITIVE)
        if combine == "restricted":
            np.testing.assert_array_equal(c.schwarz_apply(r), z_add)
        else:   # (the averaging apply sums the overlapping local solutions with atomics: its last bits vary from run to run)
            np.testing.assert_allclose(c.schwarz_apply(r), z_add, rtol=0, atol=1e-14 * np.abs(z_add).max())
    finally:
        c.close()


@pytest.fixture(scope="module")
def cube12(fedd_lib):
    """3D Laplace, H/h = 12, 27-node boxes, Q1 coarse level of 27 cells, and the oracle's pieces of the same operator"""
    c = fedd_lib.Context(device=0)
    m, om, A_bc, rhs_bc, is_dir = laplace_setup(fedd_lib, c, 3, 12)
    c.schwarz_set_target(27, 1.0)
    c.schwarz_set_coarse(27)
    c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED, two_level=1, coarse_kind=fedd_lib.COARSE_Q1)
    node_bin, nb, _ = fo.schwarz_bins(m["xyz"], 27)
    ras = fo.RAS(A_bc, node_bin, nb)
    co = fo.CoarseQ1(A_bc, m["xyz"], is_dir, 1, cells_target=27)
    yield c, A_bc, rhs_bc, ras, co
    c.close()


def restated(A, b, ras, co, rtol, x0=None, restart=100, max_it=400):
    """the oracle's restatement: right-preconditioned GMRES with (I - Pc A) M1^-1 from the projected start (the step
    x += Pc (b - A x) twice, as the library takes it: K0^-1 inverts K0 with a 1e-12 diagonal shift)"""
    x0 = np.zeros_like(b) if x0 is None else x0
    x0p = x0 + co.apply(b - A @ x0)
    x0p = x0p + co.apply(b - A @ x0p)
    return fo.gmres_right(A, b, lambda v: (y := ras.apply(v)) - co.apply(A @ y), rtol=rtol, max_it=max_it, restart=restart, x0=x0p)


@pytest.mark.parametrize("gk,s", [(0, 0), (1, 0), (2, 8), (2, 16)])
def test_multiplicative_solves_match_the_restatement(fedd_lib, cube12, gk, s):
    c, A, b, ras, co = cube12
    c.set_option("gmres_kind", gk)
    if gk == 2:
        c.set_option("gmres_s", s)
    try:
        c.schwarz_set_level_combination(fedd_lib.LEVELS_MULTIPLICATIVE)
        x, its, rel = c.gmres(None, rtol=1e-8, max_it=400, restart=100, use_prec=True)
        _, its_o, _ = restated(A, b, ras, co, 1e-8)
        assert abs(its - its_o) <= 2, (its, its_o)
        x0p = co.apply(b)
        r0 = np.linalg.norm(b - A @ (x0p + co.apply(b - A @ x0p)))     # ||r_0|| of the projected start
        assert rel <= 1e-8 and np.linalg.norm(b - A @ x) <= 1.05e-8 * r0
        # tight: the solution of the direct solver
        x, its12, rel = c.gmres(None, rtol=1e-12, max_it=400, restart=100, use_prec=True)
        xd = fo.direct_solve(A, b)
        assert rel <= 1e-12
        np.testing.assert_allclose(x, xd, rtol=0, atol=1e-10 * np.abs(xd).max())
        # the reference's sequence: coarse pre-apply into the solution vector, then the solve from it -- the same run
        c.schwarz_coarse_apply(None)
        _, its_pre, _ = c.gmres_x0(None, rtol=1e-12, max_it=400, restart=100, use_prec=True)
        assert its_pre == its12
        # from a random guess: the projection makes its residual coarse-orthogonal, and the solve converges
        x0 = np.random.default_rng(4).standard_normal(b.shape[0])
        r_raw = b - c.spmv(x0)
        x0p = x0 + c.schwarz_coarse_apply(r_raw)
        assert np.linalg.norm(c.schwarz_coarse_apply(b - c.spmv(x0p))) <= 1e-9 * np.linalg.norm(c.schwarz_coarse_apply(r_raw))
        x0p = x0p + c.schwarz_coarse_apply(b - c.spmv(x0p))
        x, its_x0, rel = c.gmres_x0(x0, rtol=1e-10, max_it=400, restart=100, use_prec=True)
        _, its_xo, _ = restated(A, b, ras, co, 1e-10, x0=x0)
        assert rel <= 1e-10 and abs(its_x0 - its_xo) <= 2, (its_x0, its_xo)
        assert np.linalg.norm(b - A @ x) <= 1.05e-10 * np.linalg.norm(b - A @ x0p)
    finally:
        c.schwarz_set_level_combination(fedd_lib.LEVELS_ADDITIVE)
        c.set_option("gmres_kind", 2)
        c.set_option("gmres_s", 0)


@pytest.mark.parametrize("gk", [0, 1, 2])
def test_multiplicative_restarts_reach_1e12(fedd_lib, gk):
    """restart 30, rtol 1e-12 on 3D elasticity (H/h = 16, steadyLinElas_Perf's mu 2e6, nu 0.4, 8-node boxes, Q1 coarse level
    of 8 cells; the oracle's restatement takes 70 iterations): three cycles, each started from a re-projected true residual;
    the tolerance is met and the s-step solver reports no floor"""
    c = fedd_lib.Context(device=0)
    try:
        m = fedd_lib.structured_mesh(3, 1, 16)
        c.mesh_set_dict(m)
        c.pattern_build(3, fedd_lib.BLOCK_FULL)
        mu, nu = 2.0e6, 0.4
        c.assemble(fedd_lib.FORM_LINELAS, [2.0 * mu * nu / (1.0 - 2.0 * nu), mu])
        c.assemble_rhs([0.0, 1.0, 0.0])
        c.dirichlet([2], [0.0, 0.0, 0.0])
        A, b, _, _, _ = fo.linelas_problem(oracle_mesh(m), mu, nu)
        c.schwarz_set_target(8, 1.0)
        c.schwarz_set_coarse(8)
        c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED, two_level=1, coarse_kind=fedd_lib.COARSE_Q1)
        c.schwarz_set_level_combination(fedd_lib.LEVELS_MULTIPLICATIVE)
        c.set_option("gmres_kind", gk)
        x, its, rel = c.gmres(None, rtol=1e-12, max_it=600, restart=30, use_prec=True)
        st = c.gmres_status()
        print("restart 30, gmres_kind %d: %d iterations, relres %.3e, status %r" % (gk, its, rel, st))
        assert its > 60 and its < 600
        assert rel <= 1e-12 and st["floor_reached"] == 0
        x0p = c.schwarz_coarse_apply(b)
        x0p = x0p + c.schwarz_coarse_apply(b - A @ x0p)
        assert np.linalg.norm(b - A @ x) <= 1.05e-12 * np.linalg.norm(b - A @ x0p)
        # what the restart projection buys: the coarse part of the final residual stays at rounding level.  Measured
        # ||Pc r|| / ||Pc b|| = 2e-15 ... 1.9e-14 with it and 3.9e-12 for all three solvers with the restart projection left
        # out (the iteration count and the tolerance are the same either way: profiles/level_combination.txt)
        bd = c.rhs_get()
        r = bd - c.spmv(x)
        coarse_part = np.linalg.norm(c.schwarz_coarse_apply(r)) / np.linalg.norm(c.schwarz_coarse_apply(bd))
        assert coarse_part <= 1e-13, coarse_part
    finally:
        c.close()


def test_multiplicative_errors_and_setup(fedd_lib):
    from test_gpu_stokes import _stokes_system_on_cylinder
    c = fedd_lib.Context(device=0)
    try:
        with pytest.raises(fedd_lib.FeddError, match="fedd_schwarz_set_level_combination"):
            c.schwarz_set_level_combination(2)
        m, om, A, b, is_dir = laplace_setup(fedd_lib, c, 3, 12)
        c.schwarz_set_target(27, 1.0)
        c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)           # one level
        c.schwarz_set_level_combination(fedd_lib.LEVELS_MULTIPLICATIVE)
        r = np.random.default_rng(1).standard_normal(b.shape[0])
        with pytest.raises(fedd_lib.FeddError, match="coarse level"):
            c.schwarz_apply(r)
        with pytest.raises(fedd_lib.FeddError, match="coarse level"):
            c.gmres(None, rtol=1e-8, max_it=100, restart=50, use_prec=True)
        with pytest.raises(fedd_lib.FeddError, match="coarse level"):
            c.gmres_x0(None, rtol=1e-8, max_it=100, restart=50, use_prec=True)
        _, its, rel = c.gmres(None, rtol=1e-8, max_it=100, restart=50, use_prec=False)   # (no preconditioner: nothing to combine)
        assert rel <= 1e-8
        # the option set before the setup: the GDSW extension solves stay one-level, K0^-1 is the one built without it
        c.schwarz_set_coarse(8)
        c.set_option("gdsw_tol", 1e-13)
        c.schwarz_set_level_combination(fedd_lib.LEVELS_ADDITIVE)
        c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED, two_level=1, coarse_kind=fedd_lib.COARSE_GDSW)
        _, K_add = c.schwarz_coarse()
        c.schwarz_set_level_combination(fedd_lib.LEVELS_MULTIPLICATIVE)
        c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED, two_level=1, coarse_kind=fedd_lib.COARSE_GDSW)
        _, K_mult = c.schwarz_coarse()
        np.testing.assert_allclose(K_mult, K_add, rtol=0, atol=1e-13 * np.abs(K_add).max())
        assert c.schwarz_get_level_combination() == fedd_lib.LEVELS_MULTIPLICATIVE
        c.schwarz_apply(r)
        # the large-subdomain path on a system that is not merged (option schwarz_big): refused by its own message
        c.set_option("schwarz_big", 1)
        c.set_option("schwarz_big_target", 150)
        c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        with pytest.raises(fedd_lib.FeddError, match="large-subdomain path"):
            c.schwarz_apply(r)
        with pytest.raises(fedd_lib.FeddError, match="large-subdomain path"):
            c.gmres(None, rtol=1e-8, max_it=100, restart=50, use_prec=True)
        c.schwarz_set_level_combination(fedd_lib.LEVELS_ADDITIVE)
        assert np.all(np.isfinite(c.schwarz_apply(r)))
    finally:
        c.close()
    c = fedd_lib.Context(device=0)
    try:
        n, nv, n_p = _stokes_system_on_cylinder(fedd_lib, c, "1k", 1.0)
        c.schwarz_set_level_combination(fedd_lib.LEVELS_MULTIPLICATIVE)
        c.schwarz_setup(overlap=1, combine=fedd_lib.COMBINE_RESTRICTED)     # merged system: the large-subdomain path
        r = np.random.default_rng(2).standard_normal(n)
        with pytest.raises(fedd_lib.FeddError, match="merged block systems"):
            c.schwarz_apply(r)
        with pytest.raises(fedd_lib.FeddError, match="merged block systems"):
            c.gmres(None, rtol=1e-8, max_it=100, restart=50, use_prec=True)
        c.schwarz_set_level_combination(fedd_lib.LEVELS_ADDITIVE)
        assert np.all(np.isfinite(c.schwarz_apply(r)))
    finally:
        c.close()


def test_multiplicative_is_independent_of_the_number_of_ranks(fedd_lib):
    """2 x 2 x 2 thread ranks, whole boxes (4 ghost layers), Q1 coarse level: the multiplicative apply equals the one-rank
    apply to 1e-13, the solve takes the same iteration count and x agrees to 1e-9"""
    capi = fedd_lib
    G, dec, target, layers = 12, (2, 2, 2), 27, 4

    def setup(c):
        c.pattern_build(1, capi.BLOCK_SCALAR)
        c.assemble(capi.FORM_LAPLACE)
        c.assemble_rhs([1.0])
        c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
        c.schwarz_set_target(target, 1.0)
        c.schwarz_set_coarse(27)
        c.schwarz_setup(1, capi.COMBINE_RESTRICTED, two_level=1, coarse_kind=capi.COARSE_Q1)
        c.schwarz_set_level_combination(capi.LEVELS_MULTIPLICATIVE)

    ref = capi.structured_mesh(3, 1, G)
    c0 = capi.Context(device=0)
    c0.mesh_set_dict(ref)
    setup(c0)
    r = np.random.default_rng(3).standard_normal(ref["n_global"])
    z_ref = c0.schwarz_apply(r)
    x_ref, its_ref, _ = c0.gmres(None, rtol=1e-10, max_it=500, restart=100, use_prec=True)
    c0.close()
    world = int(np.prod(dec))
    cells = [G // d for d in dec]
    group = capi.ThreadGroup(world)
    out, errs = [None] * world, []

    def rank_main(rank):
        try:
            m = capi.structured_mesh(3, dec, cells, rank, ghosts=layers)
            c = capi.Context(device=0, rank=rank, nranks=world, nccl_id=None)
            c.mesh_set_dict(m)
            c.halo_set_owners(m["gid_rep"], capi.structured_owner(3, dec, cells, m["gid_rep"]))
            c.comm_set_thread_group(group)
            setup(c)
            gd = m["gid_uni"]
            z = c.schwarz_apply(r[gd])
            x, its, _ = c.gmres(None, rtol=1e-10, max_it=500, restart=100, use_prec=True)
            out[rank] = (gd, z, x, its)
            c.close()
        except Exception as e:      # pragma: no cover
            errs.append(repr(e))
            group._barrier.abort()

    th = [threading.Thread(target=rank_main, args=(k,)) for k in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    z, x = np.zeros_like(z_ref), np.zeros_like(x_ref)
    for gu, zz, xx, its in out:
        z[gu] = zz
        x[gu] = xx
        assert its == its_ref
    np.testing.assert_allclose(z, z_ref, rtol=0, atol=1e-13 * np.abs(z_ref).max())
    np.testing.assert_allclose(x, x_ref, rtol=0, atol=1e-9 * np.abs(x_ref).max())


def test_facade_multiplicative_runs_the_multiplicative_preconditioner(fedd_lib, tmp_path):
    """the laplace driver with "Level Combination" = "Multiplicative" (Q1, restricted, 3D, H/h = 12, rtol 1e-12) takes the
    iteration count of the ABI-level multiplicative run with the facade's defaults, not that of the additive one, and
    solves to the direct solution"""
    from feddlib_amd import build
    driver = build.build_driver(verbose=False)
    prob = tmp_path / "p.xml"
    prob.write_text(open(os.path.join(XML, "parametersProblem.xml")).read()
                    .replace('name="Dimension" type="int" value="2"', 'name="Dimension" type="int" value="3"')
                    .replace('name="H/h" type="int" value="10"', 'name="H/h" type="int" value="12"'))
    sol = tmp_path / "s.xml"
    sol.write_text(open(os.path.join(XML, "parametersSolver.xml")).read()
                   .replace('value="1e-8"', 'value="1e-12"').replace('"Maximum Iterations" type="int" value="100"',
                                                                     '"Maximum Iterations" type="int" value="400"'))
    prec_txt = open(os.path.join(XML, "parametersPrec.xml")).read() \
        .replace('name="Combine Values in Overlap" type="string" value="Averaging"',
                 'name="Combine Values in Overlap" type="string" value="Restricted"')
    prec_txt = re.sub(r'(name="TwoLevel" type="bool" value=")[a-z]+"', r'\1true"', prec_txt)
    prec_txt = re.sub(r'(name="CoarseOperator Type" type="string" value=")[A-Za-z0-9]+"', r'\1Q1"', prec_txt)
    prec_txt = re.sub(r'(name="Level Combination" type="string" value=")[A-Za-z]+"', r'\1Multiplicative"', prec_txt)
    prec = tmp_path / "c.xml"
    prec.write_text(prec_txt)
    out = tmp_path / "x.txt"
    r = subprocess.run([driver, "--problemfile=%s" % prob, "--precfile=%s" % prec, "--solverfile=%s" % sol, "--out=%s" % out],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    mt = re.search(r"iterations (\d+) relres (\S+)", r.stdout)
    assert mt, r.stdout
    its_facade, rel_facade = int(mt.group(1)), float(mt.group(2))
    part = np.loadtxt(out)
    x = np.zeros(int(part[:, 0].max()) + 1)
    x[part[:, 0].astype(int)] = part[:, 1]
    c = fedd_lib.Context(device=0)
    try:
        _, om, A, b, _ = laplace_setup(fedd_lib, c, 3, 12)
        c.schwarz_set_target(0, 1.0)
        c.schwarz_set_coarse(0)
        c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED, two_level=1, coarse_kind=fedd_lib.COARSE_Q1)
        _, its_add, _ = c.gmres(None, rtol=1e-12, max_it=400, restart=100, use_prec=True)
        c.schwarz_set_level_combination(fedd_lib.LEVELS_MULTIPLICATIVE)
        c.schwarz_coarse_apply(None)
        _, its_mult, _ = c.gmres_x0(None, rtol=1e-12, max_it=400, restart=100, use_prec=True)
    finally:
        c.close()
    print("facade %d, ABI multiplicative %d, ABI additive %d iterations" % (its_facade, its_mult, its_add))
    assert its_facade == its_mult and its_mult != its_add
    assert rel_facade <= 1e-12
    xd = fo.direct_solve(A, b)
    np.testing.assert_allclose(x, xd, rtol=0, atol=1e-10 * np.abs(xd).max())

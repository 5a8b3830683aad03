"""The C++ host facade for unsteady nonlinear elasticity (DAESolverInTime::advanceInTimeNonLinearNewmark, TimeProblem on
NonLinElasticity, NonLinearSolver::solve(TimeProblem&, time)) through the g++-built driver
examples/drivers/unsteadynonlinelasticity_main.cpp, the reference's call sequence
(feddlib/problems/tests/unsteadyNonLinElasticity/main.cpp), on the parameter files of tests/golden/unsteadynonlinelasticity_xml."""
import os
import re
import subprocess

import numpy as np
import pytest

import fedd_oracle as fo
import hyperelastic_ref as hr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "unsteadynonlinelasticity_xml")


@pytest.fixture(scope="module")
def driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="unsteadynonlinelasticity")


def _sub(txt, key, value):
    old = re.search(r'name="%s"\s+type="\w+"\s+value="[^"]*"' % re.escape(key), txt).group(0)
    assert txt.count(old) == 1, key
    return txt.replace(old, re.sub(r'value="[^"]*"', 'value="%s"' % value, old))


def _files(tmp_path, problem=(), solver=()):
    out = []
    for name, edits in (("parametersProblem.xml", problem), ("parametersPrec.xml", ()), ("parametersSolver.xml", solver)):
        txt = open(os.path.join(XML, name)).read()
        for key, value in edits:
            txt = _sub(txt, key, value)
        f = tmp_path / name
        f.write_text(txt)
        out.append(str(f))
    return out


def _run(driver, tmp_path, files):
    out = tmp_path / "sol.txt"
    r = subprocess.run([driver, "--problemfile=%s" % files[0], "--precfile=%s" % files[1], "--solverfile=%s" % files[2],
                        "--out=%s" % out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    return r, out


def _steps(stdout):
    """per time step the relative nonlinear residuals the Newton loop printed"""
    steps, cur = [], None
    for k, v in re.findall(r"### Newton iteration : (\d+)  relative nonlinear residual : (\S+)", stdout):
        if int(k) == 0:
            cur = []
            steps.append(cur)
        cur.append(float(v))
    return steps


def _solution(out):
    x = np.loadtxt(out)
    u = np.zeros(int(x[:, 0].max()) + 1)
    u[x[:, 0].astype(np.int64)] = x[:, 1]
    return u


def test_fixture_files_are_the_settings_the_issue_names():
    txt = open(os.path.join(XML, "parametersProblem.xml")).read()
    assert 'value="Newton"' in txt and 'value="Newmark"' in txt
    v = lambda k: float(re.search(r'name="%s" type="double"\s+value="([^"]+)"' % k, txt).group(1))
    for key, base in (("Mu1", "Mu"), ("Mu2", "Mu"), ("E1", "E"), ("E2", "E")):
        assert v(key) == v(base), key
    readme = open(os.path.join(XML, "README.md")).read()
    assert "Linearization" in readme and "Mu2" in readme and "E2" in readme and "E1" in readme


def test_driver_on_the_shipped_settings(driver, tmp_path):
    """2D, P1, H/h 4, two steps: every step's Newton loop reaches relNonLinTol 1e-4 within MaxNonLinIts 6, and the exported last
    step is the --out vector bit for bit"""
    r, out = _run(driver, tmp_path, _files(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    steps = _steps(r.stdout)
    print(steps)
    assert len(steps) == 2
    for s in steps:
        assert s[0] == 1.0 and s[-1] < 1e-4 and len(s) - 1 < 6, s
    m = re.search(r"time steps (\d+) nonlinear iterations((?: \d+)+)", r.stdout)
    assert m and int(m.group(1)) == 2 and [int(k) for k in m.group(2).split()] == [len(s) - 1 for s in steps]
    u = _solution(out)
    assert np.abs(u).max() > 0.0
    last = np.fromfile(str(tmp_path / "u.u.2.bin"), dtype="<f8").reshape(-1, 3)     # the exporter writes vectors with three components
    np.testing.assert_array_equal(last[:, :2].ravel(), u)
    assert np.all(last[:, 2] == 0.0)
    assert "newton residual" in r.stdout and "newton update" in r.stdout        # the device classes in the timer report


def restatement(M, dim, model, params, density, dt, beta, gamma, force, n_steps, fedd_lib, max_its=6):
    """the steps in numpy / scipy: hyperelastic_ref tangent and force, oracle mass, sparse direct solves, the Newmark formulas of
    include/fedd_hip.h.  The source enters twice, as in the reference (right-hand side and residual)."""
    from test_gpu_newton_newmark import newmark_advance, newmark_coefs
    from test_gpu_parity import oracle_mesh
    m = fedd_lib.structured_mesh(dim, 1, M)
    om = oracle_mesh(m)
    n = dim * int(m["n_global"])
    Mm = (density * fo.assembly_mass(om, "Vector")).tocsr()
    fvec = [0.0] * dim
    fvec[1] = 1.0
    gd = (dim * om.gid_rep[:, None] + np.arange(dim)[None, :]).ravel()
    f_unit = fo.export_add(fo.assembly_rhs(om, fvec, "Vector", 0), gd, n)
    is_dir = hr.dirichlet_mask(m)
    k = newmark_coefs(dt, beta, gamma)
    u, un, v, w = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    first = True
    for step in range(n_steps):
        un, v, w, t = newmark_advance(k, u, un, v, w, first)
        first = False
        s = force * f_unit
        b = Mm @ t + s
        b[is_dir] = 0.0
        r0 = None
        for it in range(max_its + 1):      # NonLinearSolver's loop: at most MaxNonLinIts solves, no error when they are used up
            K, f, _ = hr.assemble(m, u.reshape(-1, dim)[m["gid_rep"]], model, params)
            r = ((b - f) + s) - k["cuu"] * (Mm @ u)
            r[is_dir] = 0.0 - u[is_dir]
            nr = np.linalg.norm(r)
            r0 = nr if r0 is None else r0
            if nr < 1e-10 * r0 or it == max_its:
                break
            A, rhs = fo.set_dirichlet((k["cuu"] * Mm + K).tocsr(), r.copy(), is_dir, 0.0)
            u = u + fo.direct_solve(A, rhs)
    return u


TIGHT = dict(problem=(("relNonLinTol", "1.0e-10"),), solver=(("Convergence Tolerance", "1e-12"),))


def test_driver_matches_the_restatement_of_two_steps(fedd_lib, driver, tmp_path):
    r, out = _run(driver, tmp_path, _files(tmp_path, **TIGHT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    steps = _steps(r.stdout)
    assert len(steps) == 2, steps
    u = _solution(out)
    ref = restatement(4, 2, hr.STVK, hr.stvk_params(2.0e6, 0.4), 1.0, 0.01, 0.25, 0.5, -0.01, 2, fedd_lib)
    err = np.abs(u - ref).max() / np.abs(ref).max()
    print("driver %r; against the restatement %.2e of max|u| = %.3e" % (steps, err, np.abs(ref).max()))
    assert u.shape == ref.shape and err <= 1e-10


def test_driver_3d_neo_hooke_one_step(driver, tmp_path):
    edits = (("Dimension", "3"), ("H/h", "3"), ("Material model", "Neo-Hooke"), ("Final time", "0.01"))
    r, out = _run(driver, tmp_path, _files(tmp_path, problem=edits))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    steps = _steps(r.stdout)
    assert len(steps) == 1 and steps[0][-1] < 1e-4 and len(steps[0]) - 1 < 6, steps
    u = _solution(out)
    assert u.shape[0] == 3 * 4 ** 3 and np.abs(u).max() > 0.0 and np.all(np.isfinite(u))


@pytest.mark.parametrize("edits,names", [
    ((("Linearization", "NOX"),), ('"NOX"', "FixedPoint and Newton are")),
    ((("Linearization", "FixedPoint"),), ("Only Newton implemented for nonlinear material models", "Newton is built")),
    ((("Preconditioner Method", "Triangular"),), ('"Triangular"', "Monolithic is")),
    ((("Class", "Multistep"),), ('"Multistep"', '"Newmark"', "NonLinElasticity")),
])
def test_what_is_not_built_is_an_error_that_names_what_is(driver, tmp_path, edits, names):
    r, _ = _run(driver, tmp_path, _files(tmp_path, problem=edits))
    assert r.returncode == 1, r.stdout[-2000:]
    assert "exception:" in r.stderr and all(n in r.stderr for n in names), r.stderr[-2000:]


def test_a_two_by_two_time_definition_is_refused(driver, tmp_path):
    files = _files(tmp_path)
    txt = open(files[0]).read()
    anchor = '<ParameterList name="Timestepping Parameter">'
    assert txt.count(anchor) == 1
    open(files[0], "w").write(txt.replace(anchor, anchor + '\n        <Parameter name="Time Definition Size" type="int" value="2"/>'))
    r, _ = _run(driver, tmp_path, files)
    assert r.returncode == 1 and "1 x 1 time definition" in r.stderr and "2 x 2 definition was given" in r.stderr, r.stderr[-2000:]


def test_per_flag_material_that_differs_is_refused(driver, tmp_path):
    """E2 != E on a mesh that has elements with flag 2 ... the tetrahedron of tests/golden carries element flag 1, so the key
    that can be met there is E1; E2 takes the same code path (NonLinElasticity::material)"""
    tet = os.path.join(ROOT, "tests", "golden", "tetrahedron.mesh")
    edits = (("Dimension", "3"), ("Mesh Type", "unstructured"), ("Mesh 1 Name", tet), ("Material model", "Neo-Hooke"), ("E1", "5."))
    r, _ = _run(driver, tmp_path, _files(tmp_path, problem=edits))
    assert r.returncode == 1 and "\"E1\" differs from \"E\"" in r.stderr and "per-flag materials are not built" in r.stderr, r.stderr[-2000:]

"""The facade's BDF time loop (FEDD::TimeSteppingTools "BDF", TimeProblem on NavierStokes, NonLinearSolver::solve(TimeProblem&,
time), DAESolverInTime::advanceInTimeNonLinearMultistep; feddlib_amd/host/feddlib/fedd_time.hpp) through
examples/drivers/unsteadynavierstokes_main.cpp, the reference's unsteadyNavierStokes driver, on the settings files of
tests/golden/unsteadynavierstokes_xml (its README lists the edits: 3D benchmark cylinder, Multistep with BDF 2, Newton, three
steps of dt = 0.01), against the same three steps issued over the C ABI from Python (tests/test_gpu_time_navier_stokes.py).

For the comparison at the project's bar of 1e-10 max|x| the tolerances of the files (relNonLinTol 1e-4, GMRES 1e-6, 100
iterations) are tightened in a copy, as tests/test_gpu_time_facade.py does: two loops stopped at 1e-4 agree to 1e-4 at best."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_navier_stokes import _cylinder
from test_gpu_time_navier_stokes import Device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "unsteadynavierstokes_xml")
MESH = os.path.join(ROOT, "tests", "golden", "DFG3DCylinder_1k.mesh")
TIGHT = dict(problem=(('name="relNonLinTol" type="double" value="1.0e-4"', 'name="relNonLinTol" type="double" value="1.0e-10"'),
                      ('name="MaxNonLinIts" type="int" value="10"', 'name="MaxNonLinIts" type="int" value="20"')),
             solver=(('name="Convergence Tolerance" type="double" value="1e-6"', 'name="Convergence Tolerance" type="double" value="1e-13"'),
                     ('name="Maximum Iterations" type="int" value="100"', 'name="Maximum Iterations" type="int" value="1500"')))


def setting(text, name):
    return re.search(r'name="%s"\s+type="\w+"\s+value="([^"]*)"' % re.escape(name), text).group(1)


@pytest.fixture(scope="module")
def driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="unsteadynavierstokes")


def _files(tmp_path, problem=(), prec=(), solver=()):
    out = []
    for name, edits in (("parametersProblem.xml", (('value="DFG3DCylinder_1k.mesh"', 'value="%s"' % MESH),) + tuple(problem)),
                        ("parametersPrec.xml", prec), ("parametersSolver.xml", solver)):
        txt = open(os.path.join(XML, name)).read()
        for a, b in edits:
            assert a in txt, a
            txt = txt.replace(a, b)
        f = tmp_path / name
        f.write_text(txt)
        out.append(str(f))
    return out


def _run(driver, tmp_path, files):
    out = tmp_path / "sol.txt"
    r = subprocess.run([driver, "--problemfile=%s" % files[0], "--precfile=%s" % files[1], "--solverfile=%s" % files[2],
                        "--out=%s" % out], capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    return r, out


def test_fixture_files_are_the_settings_the_issue_names():
    txt = open(os.path.join(XML, "parametersProblem.xml")).read()
    assert setting(txt, "Class") == "Multistep" and setting(txt, "BDF") == "2" and setting(txt, "Linearization") == "Newton"
    assert setting(txt, "Dimension") == "3" and setting(txt, "BC Type") == "parabolic_benchmark"
    assert setting(txt, "Mesh 1 Name") == "DFG3DCylinder_1k.mesh" and os.path.exists(MESH)
    assert abs(float(setting(txt, "Final time")) - 3.0 * float(setting(txt, "dt"))) < 1e-15
    steady = open(os.path.join(ROOT, "tests", "golden", "navierstokes_xml", "parametersProblem.xml")).read()
    assert float(setting(txt, "Viscosity")) == float(setting(steady, "Viscosity"))
    assert float(setting(txt, "MaxVelocity")) == float(setting(steady, "MaxVelocity"))
    assert os.path.exists(os.path.join(XML, "README.md"))


def test_driver_runs_the_fixture_files_as_they_are(driver, tmp_path):
    """exit 0; the reference's iteration lines for each of the three steps, a falling residual in each; 2 combines; velocity and
    pressure records for t = 0 and the three steps"""
    r, out = _run(driver, tmp_path, _files(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = re.findall(r"### Newton iteration : (\d+)  relative nonlinear residual : (\S+)", r.stdout)
    steps, cur = [], None
    for k, v in lines:
        if int(k) == 0:
            cur = []
            steps.append(cur)
        cur.append(float(v))
    print("relative nonlinear residuals per step", steps)
    assert len(steps) == 3
    for rel in steps:
        assert len(rel) >= 2 and rel[0] == 1.0 and rel[-1] < 1e-4 and all(b < a for a, b in zip(rel, rel[1:]))
    assert len(re.findall(r"### Total Newton iteration : \d+ ", r.stdout)) == 3
    m = re.search(r"time steps (\d+) combines (\d+) nonlinear iterations per step((?: \d+)+)", r.stdout)
    assert m, r.stdout[-3000:]
    assert int(m.group(1)) == 3 and int(m.group(2)) == 2
    assert [int(v) for v in m.group(3).split()] == [len(rel) - 1 for rel in steps]
    x = np.loadtxt(out)
    assert np.all(np.isfinite(x))
    for name in ("u", "p"):
        assert (tmp_path / (name + ".xmf")).exists()
        assert all((tmp_path / ("%s.%s.%d.bin" % (name, name, k))).exists() for k in range(4))
        assert not (tmp_path / ("%s.%s.4.bin" % (name, name))).exists()


def test_driver_runs_the_fixed_point_loop(driver, tmp_path):
    """the second of the two loops NonLinearSolver::solve(TimeProblem&, time) restates: combineSystems and the boundary rows
    after the residual.  Exit 0, three steps of falling residuals, 2 combines, and more iterations than Newton needs"""
    r, out = _run(driver, tmp_path, _files(tmp_path, problem=(('name="Linearization" type="string" value="Newton"',
                                                                'name="Linearization" type="string" value="FixedPoint"'),)))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = re.findall(r"### Fixed Point iteration : (\d+)  relative nonlinear residual : (\S+)", r.stdout)
    steps = []
    for k, v in lines:
        if int(k) == 0:
            steps.append([])
        steps[-1].append(float(v))
    print("relative nonlinear residuals per step", steps)
    assert len(steps) == 3 and "### Newton iteration" not in r.stdout
    for rel in steps:
        assert len(rel) >= 2 and rel[0] == 1.0 and rel[-1] < 1e-4 and all(b < a for a, b in zip(rel, rel[1:]))
    assert len(re.findall(r"### Total FPI : \d+ ", r.stdout)) == 3
    m = re.search(r"time steps (\d+) combines (\d+) nonlinear iterations per step((?: \d+)+)", r.stdout)
    assert m and int(m.group(1)) == 3 and int(m.group(2)) == 2
    assert np.all(np.isfinite(np.loadtxt(out)))


def abi_sequence(fedd_lib, prob_text, tol, rtol):
    """DAESolverInTime::advanceInTimeNonLinearMultistep with NonLinearSolver's Newton loop over the C ABI: per step the residual
    relative to the step's first one, the solution zero at t = 0 (the boundary values arrive with the first update)"""
    nu, rho = float(setting(prob_text, "Viscosity")), float(setting(prob_text, "Density"))
    dt, t_end = float(setting(prob_text, "dt")), float(setting(prob_text, "Final time"))
    m1, mv, rows, vals = _cylinder(fedd_lib)
    vals = float(setting(prob_text, "MaxVelocity")) * vals
    c = fedd_lib.Context(device=0)
    try:
        d = Device(fedd_lib, c, m1, mv, rows, vals, nu=nu, rho=rho, dt=dt)
        x = np.zeros(d.n)
        t, step, its = 0.0, 0, []
        while t + 1e-10 < t_end:
            d.advance(step, x)
            hist = []
            for k in range(21):
                r = d.residual(x)
                hist.append(float(np.linalg.norm(r)))
                if hist[-1] / hist[0] < tol:
                    break
                d.system(fedd_lib.ADV_NEWTON, x)
                b = -r
                b[rows] = 0.0
                c.rhs_set(b)
                c.dirichlet_rows(rows, -r[rows])
                dx, _, rel = d.linear_solve(rtol, True)
                x = x + dx
            assert hist[-1] / hist[0] < tol
            its.append(len(hist) - 1)
            t += dt
            step += 1
        return x, its, d.combines
    finally:
        c.close()


def test_driver_solution_matches_the_abi_sequence(fedd_lib, driver, tmp_path):
    files = _files(tmp_path, **TIGHT)
    r, out = _run(driver, tmp_path, files)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"time steps (\d+) combines (\d+) nonlinear iterations per step((?: \d+)+)", r.stdout)
    assert m, r.stdout[-3000:]
    sol = np.loadtxt(out)
    x = np.zeros(int(sol[:, 0].max()) + 1)
    x[sol[:, 0].astype(int)] = sol[:, 1]
    xa, its, combines = abi_sequence(fedd_lib, open(files[0]).read(), 1e-10, 1e-13)
    err = np.abs(x - xa).max() / np.abs(xa).max()
    print("driver: steps", m.group(1), "combines", m.group(2), "iterations", m.group(3), "| ABI iterations", its, "combines", combines,
          "| vs C-ABI sequence %.2e" % err, "max|x| %.3e" % np.abs(xa).max())
    assert int(m.group(1)) == 3 and int(m.group(2)) == combines == 2
    assert x.shape == xa.shape and np.abs(xa).max() > 0.0
    assert err <= 1e-10
    # the last exported records are the final solution
    last_p = np.fromfile(str(tmp_path / "p.p.3.bin"), dtype="<f8")
    np.testing.assert_array_equal(last_p, x[x.shape[0] - last_p.shape[0]:])


@pytest.mark.parametrize("key,value,names", [("Class", "Singlestep", ('"Multistep"', '"Newmark"')), ("Class", "External", ('"Multistep"', '"Newmark"')),
                                             ("Linearization", "Extrapolation", ("FixedPoint", "Newton")),
                                             ("Linearization", "NOX", ("FixedPoint", "Newton")), ("BDF", "3", ("1 and 2",))])
def test_what_is_not_built_ends_with_an_error_that_names_what_is(driver, tmp_path, key, value, names):
    txt = open(os.path.join(XML, "parametersProblem.xml")).read()
    old = re.search(r'name="%s"\s+type="\w+"\s+value="[^"]*"' % key, txt).group(0)
    new = re.sub(r'value="[^"]*"', 'value="%s"' % value, old)
    assert txt.count(old) == 1 and new != old
    r, out = _run(driver, tmp_path, _files(tmp_path, problem=((old, new),)))
    assert r.returncode != 0, r.stdout[-2000:]
    assert "exception:" in r.stderr and value in r.stderr and all(n in r.stderr for n in names), r.stderr[-2000:]
    assert "### Newton iteration" not in r.stdout

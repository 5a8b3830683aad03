"""The facade's time loop (FEDD::TimeSteppingTools / TimeProblem / DAESolverInTime, feddlib_amd/host/feddlib/fedd_time.hpp) through
examples/drivers/unsteadylinelas_main.cpp, the reference's unsteadyLinElas driver, on the reference's own settings files
(tests/golden/unsteadylinelas_xml: 2D, P1, H/h = 10, dt = 0.025, final time 0.05 = two steps, Newmark beta 1/4 gamma 1/2,
two-level FROSch settings, Block GMRES), against the same two steps issued over the C ABI from Python.

The only edit to the settings: the solver's tolerance (1e-6 in the file) becomes 1e-13 and its iteration limit 1000, because the
comparison is at the project's bar of 1e-10 max|x| and two solves stopped at 1e-6 agree to 1e-6 at best.  The Python side
solves with CG and a one-level preconditioner: another solver and another preconditioner, the same systems."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "unsteadylinelas_xml")


def setting(text, name):
    return re.search(r'name="%s"\s+type="\w+"\s+value="([^"]*)"' % re.escape(name), text).group(1)


@pytest.fixture(scope="module")
def driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="unsteadylinelas")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("unsteady")
    sol = d / "parametersSolver.xml"
    txt = open(os.path.join(XML, "parametersSolver.xml")).read()
    assert 'name="Convergence Tolerance" type="double" value="1e-6"' in txt
    sol.write_text(txt.replace('name="Convergence Tolerance" type="double" value="1e-6"', 'name="Convergence Tolerance" type="double" value="1e-13"')
                      .replace('name="Maximum Iterations" type="int" value="100"', 'name="Maximum Iterations" type="int" value="1000"'))
    return d, os.path.join(XML, "parametersProblem.xml"), os.path.join(XML, "parametersPrec.xml"), str(sol)


def abi_sequence(fedd_lib, prob_text):
    """the loop of DAESolverInTime::advanceInTimeLinearNewmark over the C ABI, parameters from the settings file"""
    L = fedd_lib
    dim, M = int(setting(prob_text, "Dimension")), int(setting(prob_text, "H/h"))
    mu, nu = float(setting(prob_text, "Mu")), float(setting(prob_text, "Poisson Ratio"))
    rho, force = float(setting(prob_text, "Density")), float(setting(prob_text, "Volume force"))
    dt, t_end = float(setting(prob_text, "dt")), float(setting(prob_text, "Final time"))
    beta, gamma = float(setting(prob_text, "beta")), float(setting(prob_text, "gamma"))
    assert setting(prob_text, "Class") == "Newmark" and setting(prob_text, "Discretization") == "P1" and dim == 2
    E = mu * 2.0 * (1.0 + nu)
    lam = nu * E / ((1.0 + nu) * (1.0 - 2.0 * nu))
    c = L.Context(device=0)
    try:
        c.mesh_set_dict(L.structured_mesh(dim, 1, M))
        c.pattern_build(dim, L.BLOCK_FULL)
        c.assemble(L.FORM_LINELAS, [lam, mu])
        c.matrix_store(1)
        f = [0.0] * dim
        f[1] = force                                        # the driver's rhs2D: on while t <= 1
        c.assemble_rhs(f)
        load = c.rhs_get()
        c.pattern_build(dim, L.BLOCK_DIAG)
        c.assemble(L.FORM_MASS_VEC)
        c.matrix_scale(-1, rho)
        c.matrix_store(0)
        cm = 1.0 / (dt * dt * beta)
        t, steps = 0.0, 0
        while t + 1e-10 < t_end:
            fresh = not c.matrix_combine_current(0, cm, 1, 1.0)
            if fresh:
                c.matrix_combine(0, cm, 1, 1.0)
            if steps == 0:
                c.newmark_begin()
            c.newmark_advance(0, dt, beta, gamma, 1.0)
            c.rhs_axpy(1.0, load)
            if fresh:
                c.dirichlet([1], np.zeros(dim))
                c.schwarz_setup(1, L.COMBINE_FULL)
            else:
                c.dirichlet_rhs([1], np.zeros(dim))
            x, its, rel = c.cg_x0(None, None, rtol=1e-13, max_it=2000, use_prec=True)
            t += dt
            steps += 1
        return x, steps
    finally:
        c.close()


def test_driver_runs_the_reference_settings_and_matches_the_abi_sequence(fedd_lib, driver, files):
    d, prob, prec, sol = files
    out = d / "sol.txt"
    r = subprocess.run([driver, "--problemfile=%s" % prob, "--precfile=%s" % prec, "--solverfile=%s" % sol, "--out=%s" % out],
                       capture_output=True, text=True, timeout=300, cwd=str(d))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"time steps (\d+) combines (\d+) relres (\S+)", r.stdout)
    assert m, r.stdout[-3000:]
    data = np.loadtxt(out)
    x = np.zeros(int(data[:, 0].max()) + 1)
    x[data[:, 0].astype(int)] = data[:, 1]
    xa, steps = abi_sequence(fedd_lib, open(prob).read())
    err = np.abs(x - xa).max() / np.abs(xa).max()
    print("driver: steps", m.group(1), "combines", m.group(2), "relres", m.group(3), "| vs C-ABI sequence %.2e" % err, "max|x| %.3e" % np.abs(xa).max())
    assert int(m.group(1)) == steps == 2                    # as the reference's file has
    assert int(m.group(2)) == 1                             # one coefficient set: combined once, both setups once
    assert float(m.group(3)) <= 1e-13
    assert x.shape == xa.shape and np.abs(xa).max() > 0.0
    assert err <= 1e-10
    # "ParaViewExport" = true in the file: one record per exported step (t = 0 and the two steps)
    xmf = (d / "d_s.xmf").read_text()
    assert 'Name="d_s"' in xmf and all((d / ("d_s.d_s.%d.bin" % k)).exists() for k in range(3))
    last = np.fromfile(str(d / "d_s.d_s.2.bin"), dtype="<f8").reshape(-1, 3)[:, :2].ravel()
    np.testing.assert_array_equal(last, x)


@pytest.mark.parametrize("cls", ["Multistep", "Singlestep", "External"])
def test_other_classes_are_errors_that_name_newmark(driver, files, cls):
    d, prob, prec, sol = files
    p2 = d / ("problem_%s.xml" % cls)
    txt = open(prob).read()
    assert 'name="Class"                                 type="string"		value="Newmark"' in txt
    p2.write_text(txt.replace('type="string"		value="Newmark"', 'type="string"		value="%s"' % cls))
    r = subprocess.run([driver, "--problemfile=%s" % p2, "--precfile=%s" % prec, "--solverfile=%s" % sol, "--out=%s" % (d / "none.txt")],
                       capture_output=True, text=True, timeout=300, cwd=str(d))
    assert r.returncode != 0
    assert '"Newmark"' in r.stderr and cls in r.stderr, r.stderr[-2000:]

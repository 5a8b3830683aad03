""""Preconditioner Method" = "Diagonal" / "Triangular" through the facade and the drivers (LinearSolver::solve ->
setupBlockPreconditioner, feddlib_amd/host/feddlib/fedd_facade.hpp; PrecBlock2x2_def.hpp:114-164,
Preconditioner_def.hpp:979-1062): the Stokes driver on tests/golden/stokes_block_xml against its "Monolithic" run, the steady
Navier-Stokes driver on tests/golden/navierstokes_block_xml, and the message for the methods that are not built."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MESH = os.path.join(GOLD, "DFG3DCylinder_1k.mesh")
METHOD = 'name="Preconditioner Method" type="string" value="Triangular"'


@pytest.fixture(scope="module")
def stokes_driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="stokes")


@pytest.fixture(scope="module")
def ns_driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="navierstokes")


def _problem(tmp_path, fixture, method):
    txt = open(os.path.join(GOLD, fixture, "parametersProblem.xml")).read()
    assert METHOD in txt and 'value="DFG3DCylinder_1k.mesh"' in txt
    txt = txt.replace(METHOD, METHOD.replace("Triangular", method)).replace('value="DFG3DCylinder_1k.mesh"', 'value="%s"' % MESH)
    f = tmp_path / ("problem_%s.xml" % method)
    f.write_text(txt)
    return str(f)


def _run(driver, tmp_path, problem, prec, solver, tag):
    out = tmp_path / ("sol_%s.txt" % tag)
    r = subprocess.run([driver, "--problemfile=%s" % problem, "--precfile=%s" % prec, "--solverfile=%s" % solver, "--out=%s" % out],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    return r, out


def _solution(out):
    sol = np.loadtxt(out)
    x = np.zeros(int(sol[:, 0].max()) + 1)
    x[sol[:, 0].astype(int)] = sol[:, 1]
    return x


@pytest.fixture(scope="module")
def stokes_runs(stokes_driver, tmp_path_factory):
    """the three methods on the same problem, each run once"""
    tmp = tmp_path_factory.mktemp("stokes_block")
    solver = os.path.join(GOLD, "stokes_block_xml", "parametersSolver.xml")
    runs = {}
    for method in ("Monolithic", "Triangular", "Diagonal"):
        # Monolithic reads the monolithic file; for the block methods the driver itself picks parametersPrecBlock.xml beside it
        prec = os.path.join(GOLD, "stokes_xml", "parametersPrec.xml") if method == "Monolithic" else os.path.join(GOLD, "stokes_block_xml", "parametersPrec.xml")
        r, out = _run(stokes_driver, tmp, _problem(tmp, "stokes_block_xml", method), prec, solver, method)
        assert r.returncode == 0, method + "\n" + r.stdout[-3000:] + r.stderr[-3000:]
        m = re.search(r"iterations (\d+) relres (\S+)", r.stdout)
        assert m, r.stdout
        runs[method] = (_solution(out), int(m.group(1)), float(m.group(2)), r.stdout)
        print("Stokes driver, %s: %d iterations, relres %.2e" % (method, runs[method][1], runs[method][2]))
    return runs


def test_stokes_triangular_matches_monolithic(stokes_runs):
    """the tolerance of the Stokes driver comparison in tests/test_gpu_facade.py: 1e-8 of max|x|, both runs at 1e-12"""
    xm, _, relm, _ = stokes_runs["Monolithic"]
    xt, its, relt, log = stokes_runs["Triangular"]
    assert relm <= 1e-12 and relt <= 1e-12 and its > 1
    assert "block preconditioner Triangular: velocity block from slot 0" in log
    np.testing.assert_allclose(xt, xm, rtol=0, atol=1e-8 * np.abs(xm).max())


def test_stokes_diagonal_converges(stokes_runs):
    xm, _, _, _ = stokes_runs["Monolithic"]
    xd, its, rel, log = stokes_runs["Diagonal"]
    assert rel <= 1e-12 and its > 1 and "block preconditioner Diagonal" in log
    np.testing.assert_allclose(xd, xm, rtol=0, atol=1e-8 * np.abs(xm).max())


def test_navier_stokes_newton_with_the_triangular_preconditioner(ns_driver, tmp_path):
    """tests/golden/navierstokes_block_xml: the nonlinear loop ends under the XML's own relNonLinTol within its own MaxNonLinIts;
    the velocity child is imported from slot 4 in every iteration"""
    fx = os.path.join(GOLD, "navierstokes_block_xml")
    ptxt = open(os.path.join(fx, "parametersProblem.xml")).read()
    tol = float(re.search(r'name="relNonLinTol" type="double" value="(\S+)"', ptxt).group(1))
    max_its = int(re.search(r'name="MaxNonLinIts" type="int" value="(\d+)"', ptxt).group(1))
    r, out = _run(ns_driver, tmp_path, _problem(tmp_path, "navierstokes_block_xml", "Triangular"), os.path.join(fx, "parametersPrecBlock.xml"),
                  os.path.join(fx, "parametersSolver.xml"), "ns")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rel = [float(v) for v in re.findall(r"### Newton iteration : \d+  relative nonlinear residual : (\S+)", r.stdout)]
    print("relative nonlinear residuals", rel)
    assert len(rel) >= 2 and rel[0] == 1.0 and rel[-1] < tol and len(rel) - 1 < max_its
    assert r.stdout.count("block preconditioner Triangular: velocity block from slot 4") == len(rel) - 1
    assert np.all(np.isfinite(np.loadtxt(out)))


@pytest.mark.parametrize("method", ["Teko", "FaCSI"])
def test_methods_that_are_not_built_name_the_three_that_are(stokes_driver, tmp_path, method):
    fx = os.path.join(GOLD, "stokes_block_xml")
    r, _ = _run(stokes_driver, tmp_path, _problem(tmp_path, "stokes_block_xml", method), os.path.join(fx, "parametersPrecBlock.xml"),
                os.path.join(fx, "parametersSolver.xml"), method)
    assert r.returncode != 0
    assert '"Preconditioner Method" = "%s" is not built (Monolithic, Diagonal and Triangular are; Teko and FaCSI are not)' % method in r.stderr, r.stderr

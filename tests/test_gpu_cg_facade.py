""""Solver Type" = "Block CG" through the facade (LinearSolver::solve -> fedd_cg): the laplace driver in 2D and 3D against
its own "Block GMRES" run, and the two logic_errors (a combine that is not symmetric, a solver that is not built)."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "laplace_xml")


def run_driver(tmp_path, tag, dim, Hh, solver, combine):
    from feddlib_amd import build
    driver = build.build_driver(verbose=False)
    prob = tmp_path / ("p_%s.xml" % tag)
    prob.write_text(open(os.path.join(XML, "parametersProblem.xml")).read()
                    .replace('name="Dimension" type="int" value="2"', 'name="Dimension" type="int" value="%d"' % dim)
                    .replace('name="H/h" type="int" value="10"', 'name="H/h" type="int" value="%d"' % Hh))
    sol = tmp_path / ("s_%s.xml" % tag)
    sol.write_text(open(os.path.join(XML, "parametersSolver.xml")).read().replace("Block GMRES", solver))
    prec = tmp_path / ("c_%s.xml" % tag)
    prec.write_text(open(os.path.join(XML, "parametersPrec.xml")).read()
                    .replace('name="Combine Values in Overlap" type="string" value="Averaging"',
                             'name="Combine Values in Overlap" type="string" value="%s"' % combine))
    out = tmp_path / ("x_%s.txt" % tag)
    r = subprocess.run([driver, "--problemfile=%s" % prob, "--precfile=%s" % prec, "--solverfile=%s" % sol, "--out=%s" % out],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    return r, out


def solution(out):
    part = np.loadtxt(out)
    x = np.zeros(int(part[:, 0].max()) + 1)
    x[part[:, 0].astype(int)] = part[:, 1]
    return x


@pytest.mark.parametrize("dim,Hh", [(2, 60), (3, 14)])
def test_facade_block_cg_against_block_gmres(tmp_path, dim, Hh):
    """a few thousand dofs; exit status 0, reported residual <= the file's tolerance (1e-8), and the exported solution
    within 1e-8 max|x| of the GMRES run of the same driver (the file's tolerance is all the two runs share)"""
    rc, oc = run_driver(tmp_path, "cg", dim, Hh, "Block CG", "Full")
    assert rc.returncode == 0, rc.stdout + rc.stderr
    mt = re.search(r"iterations (\d+) relres (\S+)", rc.stdout)
    assert mt, rc.stdout
    assert int(mt.group(1)) > 0 and float(mt.group(2)) <= 1e-8
    rg, og = run_driver(tmp_path, "gm", dim, Hh, "Block GMRES", "Full")
    assert rg.returncode == 0, rg.stdout + rg.stderr
    xc, xg = solution(oc), solution(og)
    assert xc.shape[0] > 2000
    print("dim", dim, "CG", mt.group(0), "| diff %.2e" % (np.abs(xc - xg).max() / np.abs(xg).max()))
    np.testing.assert_allclose(xc, xg, rtol=0, atol=1e-8 * np.abs(xg).max())


def test_facade_cg_errors(tmp_path):
    r, _ = run_driver(tmp_path, "r", 2, 10, "Block CG", "Restricted")
    assert r.returncode != 0
    assert "not symmetric: use FEDD_COMBINE_FULL" in r.stdout + r.stderr
    r, _ = run_driver(tmp_path, "b", 2, 10, "BICGSTAB", "Full")
    assert r.returncode != 0
    assert 'Solver Type "BICGSTAB" is not built (Block GMRES, Block CG, Pseudo Block CG are)' in r.stdout + r.stderr

"""The C++ host facade for nonlinear elasticity (FEDD::NonLinElasticity / NonLinearSolver) through the g++-built driver
examples/drivers/nonlinelasticity_main.cpp, the reference's call sequence (feddlib/problems/tests/nonLinElasticity/main.cpp),
on the parameter files of tests/golden/nonlinelasticity_xml: 2D Saint Venant-Kirchhoff as shipped, 3D Neo-Hooke by override."""
import os
import re
import subprocess

import numpy as np
import pytest

import hyperelastic_ref as hr
from test_gpu_hyperelastic import gpu_newton, volume_rhs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "nonlinelasticity_xml")
TET = os.path.join(ROOT, "tests", "golden", "tetrahedron.mesh")


@pytest.fixture(scope="module")
def driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="nonlinelasticity")


def _files(tmp_path, problem=()):
    out = []
    for name, edits in (("parametersProblem.xml", problem), ("parametersPrec.xml", ()), ("parametersSolver.xml", ())):
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
                        "--out=%s" % out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    return r, out


def test_fixture_files_are_the_settings_the_issue_names():
    txt = open(os.path.join(XML, "parametersProblem.xml")).read()
    assert 'name="Linearization" type="string" value="Newton"' in txt
    for key, base in (("Mu1", "Mu"), ("Mu2", "Mu"), ("E1", "E"), ("E2", "E")):
        v = lambda k: float(re.search(r'name="%s" type="double" value="([^"]+)"' % k, txt).group(1))
        assert v(key) == v(base), key
    readme = open(os.path.join(XML, "README.md")).read()
    assert "Linearization" in readme and "Mu2" in readme and "E2" in readme


CASES = {"2d_stvk": ((), 2, 6, hr.STVK, hr.stvk_params(0.3571, 0.4)),
         "3d_neohooke": ((('name="Dimension" type="int" value="2"', 'name="Dimension" type="int" value="3"'),
                          ('name="H/h" type="int" value="6"', 'name="H/h" type="int" value="4"'),
                          ('value="Saint Venant-Kirchhoff"/>', 'value="Neo-Hooke"/>')), 3, 4, hr.NEOHOOKE, (1.0, 0.4))}


@pytest.mark.parametrize("case", sorted(CASES))
def test_driver_matches_the_abi_loop(fedd_lib, driver, tmp_path, case):
    """Same number of Newton iterations as the ABI-level loop of test_gpu_hyperelastic.py on that mesh with the files' settings
    (relNonLinTol 1e-8, GMRES to 1e-12 with 100 iterations / blocks, averaging), and the same solution within 1e-10 max|u|.  The
    reference's residual subtracts the source term twice (NonLinElasticity_def.hpp:61-62, 254-263), so the ABI loop takes twice
    the load vector."""
    edits, dim, M, model, params = CASES[case]
    r, out = _run(driver, tmp_path, _files(tmp_path, edits))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rel = [float(v) for v in re.findall(r"### Newton iteration : \d+  relative nonlinear residual : (\S+)", r.stdout)]
    total = int(re.search(r"### Total Newton iterations : (\d+) ", r.stdout).group(1))
    assert rel[0] == 1.0 and rel[-1] < 1e-8 and total == len(rel) - 1
    assert r.stdout.count("(Newton-Residual)") == len(rel) + 1 and (tmp_path / "displacement.xmf").exists()
    x = np.loadtxt(out)
    m = fedd_lib.structured_mesh(dim, 1, M)
    c = fedd_lib.Context(device=0)
    try:
        c.mesh_set_dict(m)
        rhs = 2.0 * volume_rhs(fedd_lib, c, m, -0.01)
        u, ratios, its = gpu_newton(fedd_lib, c, m, model, params, rhs, tol=1e-8, rtol=1e-12, gmres_its=100, restart=100,
                                    combine=fedd_lib.COMBINE_AVERAGING, strict=True)
    finally:
        c.close()
    print("%s: driver %r; ABI loop %r" % (case, rel, ratios))
    assert total == its
    got = np.zeros_like(u)
    got[x[:, 0].astype(np.int64)] = x[:, 1]
    assert np.abs(got - u).max() <= 1e-10 * np.abs(u).max()


def test_what_is_not_built_is_an_error_that_names_what_is(driver, tmp_path):
    r, _ = _run(driver, tmp_path, _files(tmp_path, (('name="Linearization" type="string" value="Newton"',
                                                      'name="Linearization" type="string" value="NOX"'),)))
    assert r.returncode == 1 and "\"NOX\" is not built (FixedPoint and Newton are)" in r.stderr
    # per-flag materials: the tetrahedron of tests/golden carries element flag 1
    flagged = (('name="Dimension" type="int" value="2"', 'name="Dimension" type="int" value="3"'),
               ('name="Mesh Type" type="string" value="structured"', 'name="Mesh Type" type="string" value="unstructured"'),
               ('value="testFoam.mesh"', 'value="%s"' % TET), ('value="Saint Venant-Kirchhoff"/>', 'value="Neo-Hooke"/>'),
               ('name="E1" type="double" value="1."', 'name="E1" type="double" value="5."'))
    r, _ = _run(driver, tmp_path, _files(tmp_path, flagged))
    assert r.returncode == 1 and "flag 1" in r.stderr and "\"E1\" differs from \"E\"" in r.stderr and "per-flag materials are not built" in r.stderr

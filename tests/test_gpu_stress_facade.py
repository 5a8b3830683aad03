""""Symmetric gradient" = true through the C++ facade: FE::assemblyStress in Stokes::assemble.  The Stokes
driver on tests/golden/stokes_symgrad_xml against a sparse direct solve of the system restated on the host (tests/stress_ref.py for
block (0,0), the oracle's B and B^T, the Dirichlet rows), with the monolithic and the Triangular preconditioner; and the message
of Navier-Stokes, steady and in the time loop, which keeps the vector Laplacian."""
import os
import re
import subprocess

import numpy as np
import pytest

import fedd_oracle as fo
import stress_ref as sr
from test_gpu_parity import oracle_mesh
from test_gpu_structured_p2 import stokes_bc, stokes_meshes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FX = os.path.join(GOLD, "stokes_symgrad_xml")
MESH = os.path.join(GOLD, "DFG3DCylinder_1k.mesh")
SYM_OFF = 'name="Symmetric gradient" type="bool" value="false"'
SYM_ON = 'name="Symmetric gradient" type="bool" value="true"'


def driver_of(which):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which=which)


@pytest.fixture(scope="module")
def stokes_driver(fedd_lib):
    return driver_of("stokes")


def edited(tmp_path, path, edits, name=None):
    txt = open(path).read()
    for a, b in edits:
        assert a in txt, a
        txt = txt.replace(a, b)
    p = tmp_path / (name or os.path.basename(path))
    p.write_text(txt)
    return str(p)


def run(driver, tmp_path, prob, prec, sol, tag="sol"):
    out = tmp_path / ("%s.txt" % tag)
    r = subprocess.run([driver, "--problemfile=%s" % prob, "--precfile=%s" % prec, "--solverfile=%s" % sol, "--out=%s" % out],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    return r, out


def solution(r, out):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"iterations (\d+) relres (\S+)", r.stdout)
    assert m, r.stdout
    sol = np.loadtxt(out)
    x = np.full(int(sol[:, 0].max()) + 1, np.nan)
    x[sol[:, 0].astype(int)] = sol[:, 1]
    assert not np.isnan(x).any()
    return x, int(m.group(1)), float(m.group(2))


@pytest.fixture(scope="module")
def host_solution(fedd_lib):
    """the fixture's problem restated on the host, in reference numbering: [A_stress B^T; B 0] with the driver's Dirichlet rows"""
    dim, M = 2, 4
    m1, mv = stokes_meshes(fedd_lib, dim, M)
    n_p, nv = m1["xyz"].shape[0], mv["xyz"].shape[0]
    n = dim * nv + n_p
    _, BT, B = fo.stokes_blocks(oracle_mesh(mv), oracle_mesh(m1), 1.0)
    A = sr.assemble(mv)                                 # viscosity 1
    L = sr.vector_laplacian(mv)
    assert abs(A - L).max() > 0.1 * abs(A).max()        # the two forms differ: the comparison below tells them apart
    nodes, vals, rows = stokes_bc(mv)
    is_dir = np.zeros(n, dtype=bool)
    is_dir[rows] = True
    g = np.zeros(n)
    g[rows] = vals.ravel()
    M_bc, rhs_bc = fo.set_dirichlet(fo.block_merge(A, BT, B), np.zeros(n), is_dir, g)
    xd = fo.direct_solve(M_bc, rhs_bc)
    perm = mv["perm"]                                   # perm[new] = reference id
    ref = np.zeros(n)
    ref[(dim * perm[:, None] + np.arange(dim)[None, :]).ravel()] = xd[:dim * nv]
    ref[dim * nv:] = xd[dim * nv:]
    return ref


def test_fixture_is_the_structured_set_with_the_symmetric_gradient():
    a = open(os.path.join(FX, "parametersProblem.xml")).read()
    b = open(os.path.join(GOLD, "stokes_structured_xml", "parametersProblem.xml")).read()
    assert SYM_ON in a and a.replace(SYM_ON, SYM_OFF) == b
    for f in ("parametersPrec.xml", "parametersSolver.xml"):
        assert open(os.path.join(FX, f)).read() == open(os.path.join(GOLD, "stokes_structured_xml", f)).read()


@pytest.mark.parametrize("method", ["Monolithic", "Triangular"])
def test_stokes_driver_matches_the_host_solve(stokes_driver, host_solution, tmp_path, method):
    """the tolerance of the Stokes driver comparison in tests/test_gpu_facade.py: 1e-8 of max|x|, the run at 1e-12.  Triangular
    sends the FULL velocity block through fedd_matrix_import."""
    sol = edited(tmp_path, os.path.join(FX, "parametersSolver.xml"),
                 [('name="Convergence Tolerance" type="double" value="1e-6"', 'name="Convergence Tolerance" type="double" value="1e-12"')])
    prob = edited(tmp_path, os.path.join(FX, "parametersProblem.xml"),
                  [('name="Preconditioner Method" type="string" value="Monolithic"', 'name="Preconditioner Method" type="string" value="%s"' % method)])
    r, out = run(stokes_driver, tmp_path, prob, os.path.join(FX, "parametersPrec.xml"), sol, method)
    x, its, rel = solution(r, out)
    print("Stokes driver, symmetric gradient, %s: %d iterations, relres %.2e, error %.2e"
          % (method, its, rel, np.abs(x - host_solution).max() / np.abs(host_solution).max()))
    assert rel <= 1e-12 and its > 1
    if method == "Triangular":
        assert "block preconditioner Triangular: velocity block from slot 0" in r.stdout
    assert x.shape == host_solution.shape
    np.testing.assert_allclose(x, host_solution, rtol=0, atol=1e-8 * np.abs(host_solution).max())


@pytest.mark.parametrize("which,fixture", [("navierstokes", "navierstokes_xml"), ("unsteadynavierstokes", "unsteadynavierstokes_xml")])
def test_navier_stokes_names_what_is_built(fedd_lib, tmp_path, which, fixture):
    """Navier-Stokes, steady and in the time loop, keeps the vector Laplacian: with the key set it ends before any iteration, and the
    message names the key and says where the stress form is taken"""
    fx = os.path.join(GOLD, fixture)
    prob = edited(tmp_path, os.path.join(fx, "parametersProblem.xml"), [(SYM_OFF, SYM_ON), ('value="DFG3DCylinder_1k.mesh"', 'value="%s"' % MESH)])
    r, _ = run(driver_of(which), tmp_path, prob, os.path.join(fx, "parametersPrec.xml"), os.path.join(fx, "parametersSolver.xml"), "ns")
    assert r.returncode != 0
    assert '"Symmetric gradient" = true' in r.stderr and "Stokes" in r.stderr and "vector Laplacian" in r.stderr, r.stderr[-2000:]
    assert "### Newton iteration" not in r.stdout

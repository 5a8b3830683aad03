"""Structured P2 domains through the C++ facade: Domain::buildMesh(..., "P2", ...) and the drivers' "structured" branch.  The facade
keeps the device order (vertices first) as the LOCAL order and the reference's lattice ids as the GLOBAL ids of its maps; the
drivers write by global id and the exporter writes at global positions, so what leaves the facade is in reference numbering.
Each result is compared with the same problem run at the ABI level (tests/test_gpu_structured_p2.py) and carried to reference
numbering with perm."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_structured_p2 import stokes_bc, stokes_meshes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOKES_XML = os.path.join(ROOT, "tests", "golden", "stokes_structured_xml")
LAPLACE_XML = os.path.join(ROOT, "tests", "golden", "laplace_xml")


@pytest.fixture(scope="module")
def stokes_driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="stokes")


@pytest.fixture(scope="module")
def laplace_driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="laplace")


def run(driver, tmp_path, prob, prec, sol, extra=()):
    out = tmp_path / "sol.txt"
    r = subprocess.run([driver, "--problemfile=%s" % prob, "--precfile=%s" % prec, "--solverfile=%s" % sol, "--out=%s" % out, *extra],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    return r, out


def solution(r, out):
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"iterations (\d+) relres (\S+)", r.stdout)
    assert m, r.stdout
    sol = np.loadtxt(out)
    x = np.full(int(sol[:, 0].max()) + 1, np.nan)
    x[sol[:, 0].astype(int)] = sol[:, 1]
    assert not np.isnan(x).any()
    return x, int(m.group(1)), float(m.group(2))


def tightened(tmp_path, path, edits):
    txt = open(path).read()
    for a, b in edits:
        assert a in txt, a
        txt = txt.replace(a, b)
    p = tmp_path / os.path.basename(path)
    p.write_text(txt)
    return p


def test_stokes_driver_on_the_structured_fixture(fedd_lib, stokes_driver, tmp_path):
    """tests/golden/stokes_structured_xml as it is but for the solver tolerance (1e-6 in the file cannot show 1e-10): 2D, P2 / P1,
    H/h = 4, one rank, monolithic Schwarz."""
    lib = fedd_lib
    ptxt = open(os.path.join(STOKES_XML, "parametersProblem.xml")).read()
    assert 'name="Mesh Type" type="string"   value="structured"' in ptxt and 'name="Dimension" type="int"   	value="2"' in ptxt
    sol = tightened(tmp_path, os.path.join(STOKES_XML, "parametersSolver.xml"),
                    [('name="Convergence Tolerance" type="double" value="1e-6"', 'name="Convergence Tolerance" type="double" value="1e-12"')])
    r, out = run(stokes_driver, tmp_path, os.path.join(STOKES_XML, "parametersProblem.xml"), os.path.join(STOKES_XML, "parametersPrec.xml"), sol)
    x, its, rel = solution(r, out)
    assert rel <= 1e-12 and its > 1
    # the ABI sequence on the vertices-first mesh
    dim, M = 2, 4
    m1, mv = stokes_meshes(lib, dim, M)
    n_p, nv = m1["xyz"].shape[0], mv["xyz"].shape[0]
    n = dim * nv + n_p
    nodes, vals, rows = stokes_bc(mv)
    c = lib.Context(device=0)
    try:
        c.mesh_set_dict(mv)
        c.pattern_build(dim, lib.BLOCK_DIAG)
        c.assemble(lib.FORM_LAPLACE_VEC)
        c.matrix_store(0)
        c.assemble_div(n_p, 1, 2)
        c.matrix_scale(1, -1.0)
        c.matrix_scale(2, -1.0)
        c.block_merge(0, 2, 1, -1)
        c.rhs_set(np.zeros(n))
        c.dirichlet_rows(rows, vals.ravel())
        c.schwarz_setup(overlap=1, combine=lib.COMBINE_RESTRICTED)
        xa, _, rela = c.gmres(None, rtol=1e-12, max_it=1500, restart=300, use_prec=True)
    finally:
        c.close()
    assert rela <= 1e-12
    perm = mv["perm"]                                   # perm[new] = reference id
    ref = np.zeros(n)
    ref[(dim * perm[:, None] + np.arange(dim)[None, :]).ravel()] = xa[:dim * nv]
    ref[dim * nv:] = xa[dim * nv:]                      # pressure dof k = P1 lattice node k in both numberings
    assert x.shape[0] == n
    np.testing.assert_allclose(x, ref, rtol=0, atol=1e-10 * np.abs(ref).max())
    # the exporter: velocity and pressure at their global (reference) positions, the points the reference lattice
    u = np.fromfile(str(tmp_path / "velocity.u.0.bin"), dtype="<f8").reshape(-1, 3)
    p = np.fromfile(str(tmp_path / "pressure.p.0.bin"), dtype="<f8")
    np.testing.assert_array_equal(u[:, :dim].ravel(), x[:dim * nv])
    np.testing.assert_array_equal(p, x[dim * nv:])
    pts = np.fromfile(str(tmp_path / "velocity.xyz.bin"), dtype="<f8").reshape(-1, 3)
    mref = lib.structured_mesh_p2(dim, 1, M)
    assert pts[:, :dim].tobytes() == mref["xyz"].tobytes()


def laplace_problem_file(tmp_path, hh):
    return tightened(tmp_path, os.path.join(LAPLACE_XML, "parametersProblem.xml"),
                     [('name="Discretization" type="string" value="P1"', 'name="Discretization" type="string" value="P2"'),
                      ('name="H/h" type="int" value="10"', 'name="H/h" type="int" value="%d"' % hh)])


def test_laplace_driver_with_p2_on_the_structured_square(fedd_lib, laplace_driver, tmp_path):
    lib = fedd_lib
    hh = 4
    prob = laplace_problem_file(tmp_path, hh)
    sol = tightened(tmp_path, os.path.join(LAPLACE_XML, "parametersSolver.xml"), [('value="1e-8"', 'value="1e-12"')])
    r, out = run(laplace_driver, tmp_path, prob, os.path.join(LAPLACE_XML, "parametersPrec.xml"), sol)
    x, its, rel = solution(r, out)
    assert rel <= 1e-12 and 0 < its <= 100
    m = lib.structured_mesh_p2(2, 1, hh)                # reference numbering: local = global on one rank
    c = lib.Context(device=0)
    try:
        c.mesh_set_dict(m)
        c.pattern_build(1, lib.BLOCK_SCALAR)
        c.assemble(lib.FORM_LAPLACE)
        c.assemble_rhs([1.0])
        c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
        c.schwarz_setup(1, lib.COMBINE_RESTRICTED)
        xa, _, rela = c.gmres(None, rtol=1e-13, max_it=400, restart=100, use_prec=True)
    finally:
        c.close()
    assert x.shape[0] == xa.shape[0] == (2 * hh + 1) ** 2
    np.testing.assert_allclose(x, xa, rtol=0, atol=1e-10 * np.abs(xa).max())


def test_structured_p2_on_four_ranks_is_refused(laplace_driver, tmp_path):
    prob = laplace_problem_file(tmp_path, 2)
    r, _ = run(laplace_driver, tmp_path, prob, os.path.join(LAPLACE_XML, "parametersPrec.xml"), os.path.join(LAPLACE_XML, "parametersSolver.xml"),
               extra=["--ranks-as-threads=4"])
    assert r.returncode != 0
    assert "one rank" in r.stdout + r.stderr

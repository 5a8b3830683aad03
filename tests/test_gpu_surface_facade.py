"""Surface loads and Neumann terms through the C++ facade: Problem::assembleSourceTerm with "Source Type" = "surface",
a "Neumann" entry of the BCBuilder, and the elasticity driver with a surface load from its problem file.  Before these
were built the first threw "only volume source terms are built" and the Neumann entry was ignored."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAPLACE_XML = os.path.join(ROOT, "tests", "golden", "laplace_xml")
LINELAS_XML = os.path.join(ROOT, "tests", "golden", "linelas_xml")
SURFACE_XML = os.path.join(ROOT, "tests", "golden", "linelas_surface_xml")
TOL = 1e-10


@pytest.fixture(scope="module")
def program(fedd_lib, tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx
    exe = tmp_path_factory.mktemp("surface_facade") / "surface_facade"
    lib_dir = os.path.dirname(fedd_lib.LIB_PATH)
    subprocess.run([gxx, "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "feddlib_amd", "host"),
                    os.path.join(ROOT, "tests", "cpp", "surface_facade.cpp"), "-o", str(exe), "-L", lib_dir, "-lfedd_hip",
                    "-Wl,-rpath," + lib_dir], check=True)
    return str(exe)


def run_driver(driver, tmp_path, problem_xml, prec_xml, solver_xml):
    """(solution by global dof id, iterations, relative residual) of one run of an example driver"""
    out = tmp_path / "sol.txt"
    r = subprocess.run([driver, "--problemfile=%s" % problem_xml, "--precfile=%s" % prec_xml, "--solverfile=%s" % solver_xml,
                        "--out=%s" % out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"iterations (\d+) relres (\S+)", r.stdout)
    assert m, r.stdout
    sol = np.loadtxt(out)
    x = np.zeros(int(sol[:, 0].max()) + 1)
    x[sol[:, 0].astype(int)] = sol[:, 1]
    return x, int(m.group(1)), float(m.group(2))


def tight_solver(tmp_path, src_dir):
    sol = tmp_path / "solver.xml"
    txt = open(os.path.join(src_dir, "parametersSolver.xml")).read()
    for old in ('"Convergence Tolerance" type="double" value="1e-8"', '"Convergence Tolerance" type="double" value="1e-6"'):
        txt = txt.replace(old, '"Convergence Tolerance" type="double" value="1e-12"')
    assert "1e-12" in txt
    sol.write_text(txt.replace('"Maximum Iterations" type="int" value="100"', '"Maximum Iterations" type="int" value="400"'))
    return str(sol)


def test_surface_source_term_equals_the_abi_call(fedd_lib, program, tmp_path):
    out = tmp_path / "source.txt"
    r = subprocess.run([program, "--mode=source", "--problemfile=%s" % os.path.join(SURFACE_XML, "parametersProblem.xml"),
                        "--precfile=%s" % os.path.join(LINELAS_XML, "parametersPrec.xml"),
                        "--solverfile=%s" % os.path.join(LINELAS_XML, "parametersSolver.xml"), "--out=%s" % out],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.loadtxt(out)
    # the program's load function: (force, -2 force, 0.25 flag) on flag 3, (0, 0, 0.25 flag) elsewhere; force 0.5
    m = fedd_lib.structured_mesh(3, 1, 4)
    surf, sflag = fedd_lib.structured_surfaces(3, 1, 4)
    c = fedd_lib.Context(device=0)
    try:
        c.mesh_set_dict(m)
        c.pattern_build(3, fedd_lib.BLOCK_FULL)
        c.surface_set(surf, sflag)
        c.assemble_surface([[0.0, 0.0, 0.25], [0.0, 0.0, 0.5], [0.5, -1.0, 0.75]], flags=[1, 2, 3])
        ref = c.rhs_get()
    finally:
        c.close()
    assert np.abs(ref).max() > 0
    err = np.abs(got - ref).max()
    assert err <= TOL * np.abs(ref).max(), "source term of the facade against fedd_assemble_surface: %.3e" % err


def test_neumann_entry_reproduces_the_laplace_patch_test(fedd_lib, program, tmp_path):
    prob = tmp_path / "problem.xml"
    prob.write_text(open(os.path.join(LAPLACE_XML, "parametersProblem.xml")).read()
                    .replace('name="Dimension" type="int" value="2"', 'name="Dimension" type="int" value="3"')
                    .replace('name="H/h" type="int" value="10"', 'name="H/h" type="int" value="4"'))
    prec = tmp_path / "prec.xml"
    prec.write_text(open(os.path.join(LAPLACE_XML, "parametersPrec.xml")).read()
                    .replace('name="Combine Values in Overlap" type="string" value="Averaging"',
                             'name="Combine Values in Overlap" type="string" value="Restricted"'))
    out = tmp_path / "u.txt"
    flux = 0.75
    r = subprocess.run([program, "--mode=neumann", "--flux=%r" % flux, "--problemfile=%s" % prob, "--precfile=%s" % prec,
                        "--solverfile=%s" % tight_solver(tmp_path, LAPLACE_XML), "--out=%s" % out],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    u = np.loadtxt(out)
    exact = flux * fedd_lib.structured_mesh(3, 1, 4)["xyz"][:, 0]
    err = np.abs(u - exact).max() / np.abs(exact).max()
    assert err <= 1e-9, "u = g x: relative error %.3e (%s)" % (err, r.stdout.strip().splitlines()[-1])


def test_elasticity_driver_honours_source_type(fedd_lib, tmp_path):
    """linelas driver, "Source Type" = "surface": traction (0.5, 0, 0) on x = 1, clamped on x = 0, against the same problem
    set up through the ABI"""
    from feddlib_amd import build
    driver = build.build_driver(verbose=False, which="linelas")
    x, its, rel = run_driver(driver, tmp_path, os.path.join(SURFACE_XML, "parametersProblem.xml"),
                                  os.path.join(LINELAS_XML, "parametersPrec.xml"), tight_solver(tmp_path, LINELAS_XML))
    assert rel <= 1e-12
    m = fedd_lib.structured_mesh(3, 1, 4)
    surf, sflag = fedd_lib.structured_surfaces(3, 1, 4)
    mu, nu = 1.0, 0.3
    c = fedd_lib.Context(device=0)
    try:
        c.mesh_set_dict(m)
        c.pattern_build(3, fedd_lib.BLOCK_FULL)
        c.surface_set(surf, sflag)
        c.assemble(fedd_lib.FORM_LINELAS, [2.0 * mu * nu / (1.0 - 2.0 * nu), mu])
        c.assemble_surface([[0.5, 0.0, 0.0]], flags=[3])
        c.dirichlet([2], [0.0, 0.0, 0.0])
        c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        ref, _, rel2 = c.gmres(None, rtol=1e-12, max_it=400, restart=200, use_prec=True)
    finally:
        c.close()
    assert rel2 <= 1e-12 and np.abs(ref).max() > 0
    err = np.abs(x - ref).max() / np.abs(ref).max()
    assert err <= 1e-9, "driver against the ABI: relative error %.3e" % err

"""The geometry driver (examples/drivers/geometry_main.cpp: Geometry -> Domain::moveMesh -> Laplace on the moved domain) on
tests/golden/geometry_xml, against the same sequence run through capi here: the extension of the boundary displacement, the
move by it, the Laplace problem on the moved mesh.

The two sides solve the same two systems with their own solver settings, so they are compared at a tight solver tolerance
(1e-13 in a copy of parametersSolver.xml, the fixture's own is 1e-6) and must agree to 1e-10 of the largest entry, the project's
parity bar.  The written coordinates are x_ref + d with the driver's own d, one addition per entry: bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "geometry_xml")
MU, NU, DISP, M = 2.0e6, 0.4, (0.02, 0.01), 10      # parametersProblem.xml: Mu, Poisson Ratio, Displacement X / Y, H/h


@pytest.fixture(scope="module")
def geometry_driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="geometry")


def by_id(path, width=1):
    a = np.loadtxt(path).reshape(-1, 1 + width)
    out = np.zeros((int(a[:, 0].max()) + 1, width))
    out[a[:, 0].astype(int)] = a[:, 1:]
    return out


def run(driver, tmp_path, problem=None, tight=True):
    solver = os.path.join(XML, "parametersSolver.xml")
    if tight:
        txt = open(solver).read()
        assert 'name="Convergence Tolerance" type="double" value="1e-6"' in txt
        txt = txt.replace('name="Convergence Tolerance" type="double" value="1e-6"', 'name="Convergence Tolerance" type="double" value="1e-13"') \
                 .replace('name="Maximum Iterations" type="int" value="100"', 'name="Maximum Iterations" type="int" value="400"') \
                 .replace('name="Num Blocks" type="int" value="100"', 'name="Num Blocks" type="int" value="400"')
        solver = str(tmp_path / "solver.xml")
        open(solver, "w").write(txt)
    return subprocess.run([driver, "--problemfile=%s" % (problem or os.path.join(XML, "parametersProblem.xml")),
                           "--precfile=%s" % os.path.join(XML, "parametersPrec.xml"), "--solverfile=%s" % solver,
                           "--out=%s" % (tmp_path / "geo")], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))


def test_fixture_says_what_the_test_assumes():
    txt = open(os.path.join(XML, "parametersProblem.xml")).read()
    for key, value in (("Model", "Elasticity"), ("Mesh Type", "structured"), ("Discretization", "P1"), ("Dimension", "2"),
                       ("H/h", str(M)), ("Moving Flag", "3")):
        assert re.search(r'name="%s"\s+type="\w+"\s+value="%s"' % (re.escape(key), re.escape(value)), txt), key
    assert float(re.search(r'name="Mu"\s+type="double"\s+value="([^"]+)"', txt).group(1)) == MU
    assert float(re.search(r'name="Poisson Ratio"\s+type="double"\s+value="([^"]+)"', txt).group(1)) == NU
    assert float(re.search(r'name="Displacement X"\s+type="double"\s+value="([^"]+)"', txt).group(1)) == DISP[0]
    assert float(re.search(r'name="Displacement Y"\s+type="double"\s+value="([^"]+)"', txt).group(1)) == DISP[1]


def test_driver_against_the_same_sequence_through_capi(fedd_lib, geometry_driver, tmp_path):
    lib = fedd_lib
    r = run(geometry_driver, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout[-1500:])
    d_drv, u_drv = by_id(tmp_path / "geo.d.txt")[:, 0], by_id(tmp_path / "geo.u.txt")[:, 0]
    xyz_drv = by_id(tmp_path / "geo.xyz.txt", 2)

    # ---- the same through capi ----
    m = lib.structured_mesh(2, 1, M)
    gid = m["gid_rep"]
    assert np.array_equal(m["gid_uni"], np.arange(gid.shape[0]))       # one rank: unique order = global ids
    E = MU * 2.0 * (1 + NU)
    lam = (NU * E) / ((1 + NU) * (1 - 2 * NU))
    c = lib.Context(device=0)
    try:
        c.mesh_set_dict(m)
        c.pattern_build(2, lib.BLOCK_FULL)
        c.assemble(lib.FORM_LINELAS, [lam, MU])
        c.dirichlet([1, 2, 3], [[0.0, 0.0], [0.0, 0.0], list(DISP)])
        c.schwarz_setup(1, lib.COMBINE_RESTRICTED)
        d, _, rel = c.gmres(rtol=1e-13, max_it=400, restart=400)
        # (the right-hand side holds the boundary values alone, |b| ~ 0.1 against |A| |d| ~ 1e5: b - A d cannot be formed to
        # 1e-13 |b|, and the solver says so; the bound on the solutions below is what is asserted)
        assert rel <= 1e-13 or c.gmres_status()["floor_reached"]
        d_rep = d.reshape(-1, 2)[gid]
        c.mesh_move(d_rep)
        info = c.mesh_move_info()
        c.pattern_build(1, lib.BLOCK_SCALAR)
        c.assemble(lib.FORM_LAPLACE)
        c.assemble_rhs([1.0])
        c.dirichlet([1, 2, 3])
        c.schwarz_setup(1, lib.COMBINE_RESTRICTED)
        u, _, rel = c.gmres(rtol=1e-13, max_it=400, restart=400)
        assert rel <= 1e-13
    finally:
        c.close()
    assert np.abs(d).max() >= max(DISP) and np.abs(u).max() > 0
    err_d = np.abs(d_drv - d).max() / np.abs(d).max()
    err_u = np.abs(u_drv - u).max() / np.abs(u).max()
    print("extension: max difference / max entry %.2e; Laplace on the moved mesh: %.2e" % (err_d, err_u))
    assert err_d <= 1e-10 and err_u <= 1e-10

    # ---- the written coordinates: x_ref + d with the driver's d, bit for bit ----
    x_ref = np.zeros_like(m["xyz"])
    x_ref[gid] = m["xyz"]
    want = x_ref + d_drv.reshape(-1, 2)
    assert np.array_equal(xyz_drv.view(np.uint64), want.view(np.uint64))
    assert np.abs(xyz_drv - x_ref).max() >= max(DISP)

    # ---- what the driver prints about the move ----
    k = re.search(r"n_moves (\d+) geometry_id (\d+) min_det_ratio (\S+)", r.stdout)
    assert k and int(k.group(1)) == 1 and int(k.group(2)) == 1
    assert abs(float(k.group(3)) - info["min_det_ratio"]) <= 1e-8 and 0.3 < float(k.group(3)) <= 1.5
    s = re.search(r"symbolic launches before move (\d+) after move (\d+)", r.stdout)
    assert s and int(s.group(1)) >= 1 and s.group(1) == s.group(2), r.stdout


@pytest.mark.parametrize("how", ["Laplace", "absent"])
def test_laplace_model_is_an_error_that_names_elasticity(geometry_driver, tmp_path, how):
    txt = open(os.path.join(XML, "parametersProblem.xml")).read()
    line = re.search(r'.*name="Model".*\n', txt).group(0)
    txt = txt.replace(line, line.replace('value="Elasticity"', 'value="Laplace"') if how == "Laplace" else "")
    prob = tmp_path / "problem.xml"
    prob.write_text(txt)
    r = run(geometry_driver, tmp_path, problem=str(prob), tight=False)
    assert r.returncode != 0
    assert '"Elasticity"' in r.stderr and "Laplace" in r.stderr, r.stderr

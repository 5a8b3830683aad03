"""The geometry driver with --interface-flag on tests/golden/geometry_laplace_xml ("Model" absent: the reference's default, the
scaled Laplacian) against the same sequence run through capi here: the distances to the interface, the extension of the boundary
displacement with FORM_LAPLACE_XDIM, the move by it, the Laplace problem on the moved mesh.

As in test_gpu_geometry_facade.py the two sides solve with their own solver settings, so they are compared at a tight solver
tolerance (1e-13 in a copy of parametersSolver.xml) and must agree to 1e-10 of the largest entry, the project's parity bar; the
written coordinates are x_ref + d with the driver's own d, one addition per entry: bit for bit.  The facade's errors come from a
small program of the tests (tests/cpp/interface_facade.cpp)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import interface_ref as ir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "geometry_laplace_xml")
DIST, COEF, DISP, M, FLAG = 0.25, 100.0, (0.02, 0.01), 10, 3      # parametersProblem.xml; FLAG: --interface-flag


@pytest.fixture(scope="module")
def geometry_driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="geometry")


@pytest.fixture(scope="module")
def program(fedd_lib, tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx
    exe = tmp_path_factory.mktemp("interface_facade") / "interface_facade"
    lib_dir = os.path.dirname(fedd_lib.LIB_PATH)
    subprocess.run([gxx, "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "feddlib_amd", "host"),
                    os.path.join(ROOT, "tests", "cpp", "interface_facade.cpp"), "-o", str(exe), "-L", lib_dir, "-lfedd_hip",
                    "-Wl,-rpath," + lib_dir], check=True)
    return str(exe)


def by_id(path, width=1):
    a = np.loadtxt(path).reshape(-1, 1 + width)
    out = np.zeros((int(a[:, 0].max()) + 1, width))
    out[a[:, 0].astype(int)] = a[:, 1:]
    return out


def run(driver, tmp_path, extra=(), tight=True):
    solver = os.path.join(XML, "parametersSolver.xml")
    if tight:
        txt = open(solver).read()
        assert 'name="Convergence Tolerance" type="double" value="1e-6"' in txt
        txt = txt.replace('name="Convergence Tolerance" type="double" value="1e-6"', 'name="Convergence Tolerance" type="double" value="1e-13"') \
                 .replace('name="Maximum Iterations" type="int" value="100"', 'name="Maximum Iterations" type="int" value="400"') \
                 .replace('name="Num Blocks" type="int" value="100"', 'name="Num Blocks" type="int" value="400"')
        solver = str(tmp_path / "solver.xml")
        open(solver, "w").write(txt)
    return subprocess.run([driver, "--problemfile=%s" % os.path.join(XML, "parametersProblem.xml"),
                           "--precfile=%s" % os.path.join(XML, "parametersPrec.xml"), "--solverfile=%s" % solver,
                           "--out=%s" % (tmp_path / "geo")] + list(extra), capture_output=True, text=True, timeout=300, cwd=str(tmp_path))


def test_fixture_says_what_the_test_assumes(fedd_lib):
    txt = open(os.path.join(XML, "parametersProblem.xml")).read()
    assert 'name="Model"' not in txt
    for key, value in (("Mesh Type", "structured"), ("Discretization", "P1"), ("Dimension", "2"), ("H/h", str(M)), ("Moving Flag", "3")):
        assert re.search(r'name="%s"\s+type="\w+"\s+value="%s"' % (re.escape(key), re.escape(value)), txt), key
    assert float(re.search(r'name="Distance Laplace"\s+type="double"\s+value="([^"]+)"', txt).group(1)) == DIST
    assert float(re.search(r'name="Coefficient Laplace"\s+type="double"\s+value="([^"]+)"', txt).group(1)) == COEF
    assert float(re.search(r'name="Displacement X"\s+type="double"\s+value="([^"]+)"', txt).group(1)) == DISP[0]
    assert float(re.search(r'name="Displacement Y"\s+type="double"\s+value="([^"]+)"', txt).group(1)) == DISP[1]
    # some but not all elements of the test mesh are scaled
    m = fedd_lib.structured_mesh(2, 1, M)
    f = ir.coefficients(m, ir.distances_to_flags(m, FLAG), DIST, COEF)
    assert 0 < np.count_nonzero(f == COEF) < f.shape[0]


def test_driver_against_the_same_sequence_through_capi(fedd_lib, geometry_driver, tmp_path):
    lib = fedd_lib
    r = run(geometry_driver, tmp_path, extra=["--interface-flag=%d" % FLAG])
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout[-1500:])
    d_drv, u_drv = by_id(tmp_path / "geo.d.txt")[:, 0], by_id(tmp_path / "geo.u.txt")[:, 0]
    xyz_drv = by_id(tmp_path / "geo.xyz.txt", 2)

    m = lib.structured_mesh(2, 1, M)
    gid = m["gid_rep"]
    assert np.array_equal(m["gid_uni"], np.arange(gid.shape[0]))       # one rank: unique order = global ids
    c = lib.Context(device=0)
    try:
        c.mesh_set_dict(m)
        n_if = c.interface_distance([FLAG])
        c.pattern_build(2, lib.BLOCK_DIAG)
        c.assemble(lib.FORM_LAPLACE_XDIM, [DIST, COEF])
        f = c.laplace_scale()
        c.dirichlet([1, 2, 3], [[0.0, 0.0], [0.0, 0.0], list(DISP)])
        c.schwarz_setup(1, lib.COMBINE_RESTRICTED)
        d, _, rel = c.gmres(rtol=1e-13, max_it=400, restart=400)
        assert rel <= 1e-13 or c.gmres_status()["floor_reached"]
        c.mesh_move(d.reshape(-1, 2)[gid])
        assert c.interface_distance_info()["have"]
        c.pattern_build(1, lib.BLOCK_SCALAR)
        c.assemble(lib.FORM_LAPLACE)
        c.assemble_rhs([1.0])
        c.dirichlet([1, 2, 3])
        c.schwarz_setup(1, lib.COMBINE_RESTRICTED)
        u, _, rel = c.gmres(rtol=1e-13, max_it=400, restart=400)
        assert rel <= 1e-13
    finally:
        c.close()
    assert 0 < np.count_nonzero(f == COEF) < f.shape[0]
    k = re.search(r"interface nodes (\d+)", r.stdout)
    assert k and int(k.group(1)) == n_if == np.count_nonzero(m["flag_uni"] == FLAG)
    assert np.abs(d).max() >= max(DISP) and np.abs(u).max() > 0
    err_d = np.abs(d_drv - d).max() / np.abs(d).max()
    err_u = np.abs(u_drv - u).max() / np.abs(u).max()
    print("extension: max difference / max entry %.2e; Laplace on the moved mesh: %.2e" % (err_d, err_u))
    assert err_d <= 1e-10 and err_u <= 1e-10

    x_ref = np.zeros_like(m["xyz"])
    x_ref[gid] = m["xyz"]
    want = x_ref + d_drv.reshape(-1, 2)
    assert np.array_equal(xyz_drv.view(np.uint64), want.view(np.uint64))
    assert np.abs(xyz_drv - x_ref).max() >= max(DISP)
    s = re.search(r"symbolic launches before move (\d+) after move (\d+)", r.stdout)
    assert s and int(s.group(1)) >= 1 and s.group(1) == s.group(2), r.stdout       # the move and the assembly after it: no symbolic work


def test_without_the_option_the_default_model_is_still_an_error(geometry_driver, tmp_path):
    r = run(geometry_driver, tmp_path, tight=False)
    assert r.returncode != 0
    assert '"Elasticity"' in r.stderr and "Laplace" in r.stderr and "identifyInterfaceParallelAndDistance" in r.stderr, r.stderr
    r = run(geometry_driver, tmp_path, extra=["--interface-flag=x"], tight=False)
    assert r.returncode == 2 and "wants an integer" in r.stderr


def test_domains_with_different_interface_counts_are_refused(program, tmp_path):
    r = subprocess.run([program, "--mode=mismatch"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DetermineInterfaceInParallel failed. ThisMesh and OtherMesh seem to have different numbers of interface nodes." in r.stdout
    assert "has distances 0" in r.stdout            # nothing was computed


def test_a_foreign_function_is_refused(program, tmp_path):
    r = subprocess.run([program, "--mode=foreign"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "func is not HeuristicScaling" in r.stdout and "what is built" in r.stdout
    assert "HeuristicScaling accepted" in r.stdout


def test_errors_without_distances(program, tmp_path):
    r = subprocess.run([program, "--mode=nodist"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"caught assembly: .*identifyInterfaceParallelAndDistance", r.stdout)
    assert re.search(r"caught calculate: .*identifyInterfaceParallelAndDistance", r.stdout)
    assert re.search(r"caught get: .*no distances", r.stdout)


def test_distances_of_the_facade_are_the_restatement(fedd_lib, program, tmp_path):
    r = subprocess.run([program, "--mode=distances"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    rows = np.array([[float(t) for t in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("dist ")])
    assert rows.shape == (25, 4)
    xyz, d = rows[:, 1:3], rows[:, 3]
    side = xyz[xyz[:, 0] == 0.0]
    assert side.shape[0] == 5
    ref = ir.distances(xyz, side)                   # flag 2 is the whole side x = 0
    assert np.array_equal(d.view(np.uint64), ref.view(np.uint64))
    assert np.array_equal(d.view(np.uint64), np.ascontiguousarray(xyz[:, 0]).view(np.uint64))

"""The ALE Navier-Stokes driver (examples/drivers/alenavierstokes_main.cpp: Domain::moveMesh, a mesh velocity from two
displacements, FE::assemblyAdditionalConvection, the fixed-point loop on NavierStokes::calculateNonLinResidualVecWithMeshVelo)
on tests/golden/alenavierstokes_xml, against the same sequence run through capi here, and the four errors of the facade.

Both sides iterate the same fixed-point map to a relative nonlinear residual of 1e-12 with linear solves at 1e-13 (the
fixture's values), each with its own preconditioner, and must agree to 1e-10 of the largest entry, the project's parity bar
for a driver against capi."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_structured_p2 import stokes_bc, stokes_meshes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "alenavierstokes_xml")
DIM, M, NU, RHO, UMAX, A_OLD, A_NEW, DT, TOL, MAX_ITS = 2, 4, 0.1, 1.5, 1.0, 0.03, 0.05, 0.1, 1e-12, 40


@pytest.fixture(scope="module")
def driver(fedd_lib):
    from feddlib_amd import build
    return build.build_driver(verbose=False, which="alenavierstokes")


def run(driver, tmp_path, *extra):
    return subprocess.run([driver, "--problemfile=%s" % os.path.join(XML, "parametersProblem.xml"),
                           "--precfile=%s" % os.path.join(XML, "parametersPrec.xml"),
                           "--solverfile=%s" % os.path.join(XML, "parametersSolver.xml"), "--out=%s" % (tmp_path / "sol.txt"), *extra],
                          capture_output=True, text=True, timeout=300, cwd=str(tmp_path))


def displacement(x, a):
    """the driver's: a * prod_j sin(pi x_j) * cos(2.1 x_{k+1} + 0.7 k), exactly zero on the boundary"""
    dim = x.shape[1]
    bubble = np.prod(np.sin(np.pi * x), axis=1)
    d = a * np.stack([bubble * np.cos(2.1 * x[:, (k + 1) % dim] + 0.7 * k) for k in range(dim)], axis=1)
    d[np.any((x == 0.0) | (x == 1.0), axis=1)] = 0.0
    return d


def test_fixture_says_what_the_test_assumes():
    txt = open(os.path.join(XML, "parametersProblem.xml")).read()
    for key, value in (("Dimension", DIM), ("H/h", M), ("Viscosity", NU), ("Density", RHO), ("MaxVelocity", UMAX),
                       ("Mesh Amplitude Old", A_OLD), ("Mesh Amplitude New", A_NEW), ("Mesh Time Step", DT), ("relNonLinTol", TOL),
                       ("MaxNonLinIts", MAX_ITS)):
        got = re.search(r'name="%s"\s+type="\w+"\s+value="([^"]+)"' % re.escape(key), txt)
        assert got and float(got.group(1)) == float(value), key
    assert 'name="Convergence Tolerance" type="double" value="1e-13"' in open(os.path.join(XML, "parametersSolver.xml")).read()


def test_driver_against_the_same_sequence_through_capi(fedd_lib, driver, tmp_path):
    lib = fedd_lib
    r = run(driver, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout[-1200:])
    got = re.search(r"nonlinear iterations (\d+) residual (\S+)", r.stdout)
    assert got and float(got.group(2)) < TOL and int(got.group(1)) >= 3
    sol = np.loadtxt(tmp_path / "sol.txt")
    x = np.full(int(sol[:, 0].max()) + 1, np.nan)
    x[sol[:, 0].astype(int)] = sol[:, 1]
    assert not np.isnan(x).any()

    # ---- the same through capi, on the vertices-first mesh ----
    m1, mv = stokes_meshes(lib, DIM, M)
    n_p, nv = m1["xyz"].shape[0], mv["xyz"].shape[0]
    n = DIM * nv + n_p
    nodes, vals, rows = stokes_bc(mv, lambda y: 4.0 * UMAX * y * (1.0 - y))
    vals = vals.ravel()
    d_old, d_new = displacement(mv["xyz"], A_OLD), displacement(mv["xyz"], A_NEW)
    c = lib.Context(device=0)
    try:
        c.mesh_set_dict(mv)
        c.mesh_move(d_new)
        c.mesh_velocity_diff(d_new, d_old, DT)
        c.pattern_build(DIM, lib.BLOCK_DIAG)
        c.assemble(lib.FORM_LAPLACE_VEC)
        c.matrix_scale(-1, NU * RHO)
        c.matrix_store(0)
        c.assemble_div(n_p, 1, 2)
        c.matrix_scale(1, -1.0)
        c.matrix_scale(2, -1.0)
        xa = np.zeros(n)
        r0 = None
        for it in range(MAX_ITS + 1):
            c.velocity_set(xa[:DIM * nv])
            c.assemble_advection_ale(lib.ALE_FIXEDPOINT, RHO, 0, 4)
            c.block_merge(4, 2, 1, -1)
            res = -c.spmv(xa)                                   # "reverse": rhs - K(x) x, the Dirichlet rows g - x
            res[rows] = vals - xa[rows]
            rn = float(np.linalg.norm(res))
            r0 = rn if r0 is None else r0
            if rn / r0 < TOL:
                break
            b = res.copy()
            b[rows] = 0.0
            c.rhs_set(b)
            c.dirichlet_rows(rows, res[rows])
            c.schwarz_setup(overlap=1, combine=lib.COMBINE_RESTRICTED)
            dx, _, rel = c.gmres(None, rtol=1e-13, max_it=1500, restart=300, use_prec=True)
            xa += dx
        assert rn / r0 < TOL and it >= 3
        # the ALE terms matter for this input: the fixed-mesh matrix at the same state is another matrix
        c.assemble_advection(lib.ADV_N, RHO, 0, 3)
        c.assemble_advection_ale(lib.ALE_FIXEDPOINT, RHO, 0, 4)
        assert abs(c.matrix_get(3) - c.matrix_get(4)).max() > 1e-3 * abs(c.matrix_get(4)).max()
    finally:
        c.close()
    perm = mv["perm"]                                           # perm[new] = reference id
    ref = np.zeros(n)
    ref[(DIM * perm[:, None] + np.arange(DIM)[None, :]).ravel()] = xa[:DIM * nv]
    ref[DIM * nv:] = xa[DIM * nv:]
    assert x.shape[0] == n
    err = np.abs(x - ref).max() / np.abs(ref).max()
    print("driver %s iterations, capi %d; max difference / max entry %.3e" % (got.group(1), it, err))
    assert err <= 1e-10


@pytest.mark.parametrize("what,message", [
    ("wrongP", "is not the matrix FE::assemblyAdditionalConvection returned last"),
    ("wrongScale", "must be scaled by exactly -density"),
    ("wrongDiff", "u_minus_w is not u - w"),
    ("newton", "Newton method not implemented in reAssembleFSI"),
])
def test_facade_errors(driver, tmp_path, what, message):
    r = run(driver, tmp_path, "--provoke=%s" % what)
    assert r.returncode == 1, r.stdout + r.stderr
    assert message in r.stderr, r.stderr
    assert "A + density N(u - w) - density P(w)" in r.stderr or what in ("wrongDiff", "newton")

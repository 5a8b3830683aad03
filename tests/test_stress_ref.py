"""The numpy restatement of FE::assemblyStress (tests/stress_ref.py) has the properties of the form, and the product declares the
entry, refuses a host-only context by name, and no longer refuses "Symmetric gradient" = true in the facade.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import stress_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "stokes_symgrad_xml")
CASES = [(2, "p1", 3), (2, "p2", 3), (3, "p1", 2), (3, "p2", 2)]
_cache = {}


def mesh(lib, dim, fe, M):
    key = (dim, fe, M)
    if key not in _cache:
        m = sr.jitter(lib.structured_mesh(dim, 1, M))
        _cache[key] = lib.p2_of_p1(m, volume_id=0) if fe == "p2" else m
    return _cache[key]


@pytest.mark.parametrize("dim,fe,M", CASES)
def test_closed_form_is_the_element_loop(fedd_lib, dim, fe, M):
    m = mesh(fedd_lib, dim, fe, M)
    c = np.random.default_rng(2).uniform(0.5, 2.0, (m["conn"].shape[0], sr.rule(m)[1].shape[0]))
    A, B = sr.assemble(m, c, loops=True), sr.assemble(m, c)
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    assert abs(A - B).max() <= 1e-14 * abs(A).max()
    # FULL pattern: every row of a node has dim entries per coupled node
    assert np.all(np.diff(A.indptr) % dim == 0)


@pytest.mark.parametrize("dim,fe,M", CASES)
def test_annihilates_rotations_and_the_vector_laplacian_does_not(fedd_lib, dim, fe, M):
    m = mesh(fedd_lib, dim, fe, M)
    K, L, R = sr.assemble(m), sr.vector_laplacian(m), sr.rotations(m)
    assert R.shape[1] == (1 if dim == 2 else 3)
    for k in range(R.shape[1]):
        r = R[:, k]
        assert np.abs(K @ r).max() <= 1e-13 * np.abs(K).sum(axis=1).max() * np.abs(r).max()
        assert np.abs(L @ r).max() >= 1e-3 * np.abs(L).max() * np.abs(r).max()      # so the check tells the two forms apart
    # both annihilate translations
    for d in range(dim):
        t = np.zeros(K.shape[0]); t[d::dim] = 1.0
        assert np.abs(K @ t).max() <= 1e-13 * np.abs(K).sum(axis=1).max()


@pytest.mark.parametrize("dim,fe,M", CASES)
def test_symmetric_and_linear_in_c(fedd_lib, dim, fe, M):
    m = mesh(fedd_lib, dim, fe, M)
    rng = np.random.default_rng(4)
    shape = (m["conn"].shape[0], sr.rule(m)[1].shape[0])
    c1, c2 = rng.uniform(0.5, 2.0, shape), rng.uniform(0.5, 2.0, shape)
    K1, K2, K12 = sr.assemble(m, c1), sr.assemble(m, c2), sr.assemble(m, 2.0 * c1 + 3.0 * c2)
    assert abs(K1 - K1.T).max() <= 1e-14 * abs(K1).max()
    assert abs(K12 - (2.0 * K1 + 3.0 * K2)).max() <= 1e-13 * abs(K12).max()
    assert abs(sr.assemble(m, np.ones(shape)) - sr.assemble(m)).max() == 0.0


def test_quadrature_points_are_the_affine_images(fedd_lib):
    m = mesh(fedd_lib, 3, "p2", 2)
    x = sr.quadrature_points(m)
    xi = sr.rule(m)[0]
    X = m["xyz"][m["conn"][:, :4]]
    lam = np.concatenate([1.0 - xi.sum(axis=1, keepdims=True), xi], axis=1)         # barycentric
    assert np.abs(x - np.einsum("kv,evd->ekd", lam, X)).max() <= 1e-15


def test_header_declares_the_entry_and_capi_binds_it(fedd_lib):
    hdr = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    assert re.search(r"int fedd_assemble_stress\(fedd_ctx\* ctx, const double\* coeff_q, int64_t n_coeff\);", hdr)
    assert re.search(r"FEDD_FORM_STRESS\s+= 6", hdr)
    assert "fedd_assemble_stress" in fedd_lib.SIGNATURES and fedd_lib.FORM_STRESS == 6
    assert hasattr(fedd_lib.lib(), "fedd_assemble_stress")


def test_host_only_context_names_what_it_needs(fedd_lib):
    c = fedd_lib.Context(device=-1)
    try:
        c.mesh_set_dict(fedd_lib.structured_mesh(2, 1, 2))
        with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
            c.assemble_stress()
        with pytest.raises(fedd_lib.FeddError, match="needs a GPU context"):
            c.assemble_stress(np.ones((8, 1)))
    finally:
        c.close()


def test_facade_takes_the_symmetric_gradient(fedd_lib, tmp_path):
    """The facade has FE::assemblyStress, compiles into the drivers, and Stokes no longer refuses the key.  Run on a host-only
    context (LOCAL_RANK = -1) with "Symmetric gradient" = true, the Stokes driver ends at its first device call, naming the GPU it
    needs, not at a "not built" refusal."""
    from feddlib_amd import build
    src = open(os.path.join(ROOT, "feddlib_amd", "host", "feddlib", "fedd_facade.hpp")).read()
    assert "void assemblyStress(int dim, std::string FEType, MatrixPtr_Type& A, CoeffFunc_Type func, int* parameters, bool callFillComplete" in src
    assert "assemblyStress is not built" not in src and "(symmetric gradient) is not built" not in src
    stokes = src[src.index("class Stokes : public Problem"):src.index("class NonLinearProblem : public Problem")]
    assert "Symmetric gradient" in stokes and "feFactory_->assemblyStress(" in stokes       # Stokes::assemble takes the key ...
    assert not re.search(r'TEUCHOS_TEST_FOR_EXCEPTION\([^;]*Symmetric gradient', stokes)      # ... and does not refuse it
    build.build_driver(verbose=False, which="navierstokes")
    drv = build.build_driver(verbose=False, which="stokes")
    r = subprocess.run([drv, "--problemfile=%s" % os.path.join(FX, "parametersProblem.xml"), "--precfile=%s" % os.path.join(FX, "parametersPrec.xml"),
                        "--solverfile=%s" % os.path.join(FX, "parametersSolver.xml"), "--out=%s" % (tmp_path / "x.txt")],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=dict(os.environ, LOCAL_RANK="-1"))
    assert r.returncode != 0
    assert "not built" not in r.stdout + r.stderr
    assert "needs a GPU context" in r.stdout + r.stderr

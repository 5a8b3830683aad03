"""The stress form of the velocity block on the GPU (fedd_assemble_stress, FEDD_FORM_STRESS) against the numpy restatement of
tests/stress_ref.py, the elasticity form that is already built, the properties of the form (rigid-body null space, symmetry,
linearity in c), reproducibility, its errors, and what the call does to the solver state."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import fedd_oracle as fo
import stress_ref as sr
from test_gpu_parity import csr_global

pytestmark = pytest.mark.gpu
RTOL = 1e-10        # the project's parity bar

# 4 x 4 (x 4) cells, interior nodes moved by a seeded +-0.2 h; p2_cube4: 384 tetrahedra, 729 nodes, vertex nodes of full valence
# whose FULL row holds more node blocks than a wave has lanes.  p2_box322: 3 x 2 x 2 cells, 72 elements; p*_box333: 162 elements,
# no multiple of the four waves (elements) of a workgroup, so the last workgroup is a partial one.
MESHES = ["p1_square4", "p2_square4", "p1_cube4", "p2_cube4", "p2_box322", "p1_box333", "p2_box333"]
_cache = {}


def mesh(lib, which):
    if which not in _cache:
        fe, shape = which.split("_")
        if shape.startswith("square"):
            dim, cells = 2, [4, 4]
        elif shape.startswith("cube"):
            dim, cells = 3, [4, 4, 4]
        else:
            dim, cells = 3, [int(ch) for ch in shape[3:]]
        m = sr.jitter(lib.structured_mesh(dim, 1, cells))
        if fe == "p2":      # the mid nodes of the boundary take their flags from the surface elements
            m["surf"], m["surf_flag"] = lib.structured_surfaces(dim, 1, cells)
            m = lib.p2_of_p1(m, volume_id=0)
        _cache[which] = m
    return _cache[which]


def coeff(m, seed=5):
    nq = sr.rule(m)[1].shape[0]
    return np.random.default_rng(seed).uniform(0.5, 2.0, (m["conn"].shape[0], nq))


@pytest.fixture(scope="module")
def reference():
    """restatement results, computed once per (mesh, coefficient) and shared; never modified"""
    cache = {}

    def get(lib, which, with_c):
        key = (which, with_c)
        if key not in cache:
            m = mesh(lib, which)
            cache[key] = sr.assemble(m, coeff(m) if with_c else None)
        return cache[key]
    return get


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def setup(lib, ctx, m):
    ctx.mesh_set_dict(m)
    ctx.pattern_build(m["dim"], lib.BLOCK_FULL)


def system(ctx, m):
    return csr_global(ctx, m["dim"] * int(m["n_global"]))[0]


def assert_close(A, B):
    A = A.tocsr(); B = B.tocsr()
    A.sort_indices(); B.sort_indices()
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)      # structural zeros included
    scale = np.abs(B).max(axis=1).toarray().ravel()
    assert scale.min() > 0.0
    err = (np.abs(A.data - B.data) / np.repeat(scale, np.diff(B.indptr))).max()
    assert err <= RTOL, err
    return err


def test_meshes_are_what_the_cases_need(fedd_lib):
    m = mesh(fedd_lib, "p2_cube4")
    assert m["conn"].shape == (384, 10) and int(m["n_global"]) == 729
    K = sr.assemble(mesh(fedd_lib, "p1_cube4"))
    assert np.diff(K.indptr).max() // 3 <= 64           # P1: a row of node blocks fits a wave ...
    nodes_per_row = np.diff(sp.csr_matrix(sr.assemble(m)).indptr).max() // 3
    assert nodes_per_row > 64                            # ... P2: the full-valence vertex does not
    assert mesh(fedd_lib, "p2_box322")["conn"].shape[0] == 72 and mesh(fedd_lib, "p2_box333")["conn"].shape[0] % 4 == 2


@pytest.mark.parametrize("which", MESHES)
def test_matches_the_restatement(fedd_lib, ctx, reference, which):
    m = mesh(fedd_lib, which)
    setup(fedd_lib, ctx, m)
    pattern = system(ctx, m)                            # fedd_pattern_build(dim, FULL), values zero
    K1 = reference(fedd_lib, which, False)
    assert np.array_equal(pattern.indptr, K1.indptr) and np.array_equal(pattern.indices, K1.indices)
    ctx.assemble_stress()
    e0 = assert_close(system(ctx, m), K1)
    ctx.assemble_stress(np.ones_like(coeff(m)))
    e1 = assert_close(system(ctx, m), K1)
    ctx.assemble_stress(coeff(m))
    e2 = assert_close(system(ctx, m), reference(fedd_lib, which, True))
    ctx.assemble(fedd_lib.FORM_STRESS)                  # the same call with c = 1
    e3 = assert_close(system(ctx, m), K1)
    print("%s: c = 1 %.2e, ones %.2e, c_q %.2e, fedd_assemble %.2e of the row maximum" % (which, e0, e1, e2, e3))


@pytest.mark.parametrize("which", MESHES)
def test_equals_the_elasticity_form_with_mu_1_lambda_0(fedd_lib, ctx, which):
    """FE::assemblyLinElasXDim (FE_def.hpp:2739-3040) is 2 mu eps(u) : eps(v) + lambda div u div v; with mu = 1, lambda = 0 that
    is grad v : (grad u + grad u^T) on the same rule and the same pattern."""
    m = mesh(fedd_lib, which)
    setup(fedd_lib, ctx, m)
    ctx.assemble(fedd_lib.FORM_LINELAS, [0.0, 1.0])     # params = {lambda, mu}
    E = system(ctx, m)
    ctx.assemble_stress()
    assert_close(system(ctx, m), E)


@pytest.mark.parametrize("which", MESHES)
def test_null_space_and_symmetry(fedd_lib, ctx, which):
    m = mesh(fedd_lib, which)
    setup(fedd_lib, ctx, m)
    for c_q in (None, coeff(m)):
        ctx.assemble_stress(c_q)
        K = system(ctx, m)
        R = sr.rotations(m)
        norm = np.abs(K).sum(axis=1).max()              # ||K||_inf
        for k in range(R.shape[1]):
            assert np.abs(K @ R[:, k]).max() <= RTOL * norm * np.abs(R[:, k]).max()
        assert abs(K - K.T).max() <= RTOL * np.abs(K).max()


@pytest.mark.parametrize("which", MESHES)
def test_reproducible_and_exactly_linear_in_c(fedd_lib, ctx, which):
    m = mesh(fedd_lib, which)
    setup(fedd_lib, ctx, m)
    c_q = coeff(m)
    ctx.assemble_stress(c_q)
    a = ctx.csr_get()[2].copy()
    ctx.assemble_stress()
    ctx.assemble_stress(c_q)
    b = ctx.csr_get()[2].copy()
    assert np.array_equal(a, b)                         # equal bits
    ctx.assemble_stress(2.0 * c_q)
    assert np.array_equal(ctx.csr_get()[2], 2.0 * a)    # a power of two commutes with every rounding


def test_errors_name_themselves(fedd_lib, ctx):
    m = mesh(fedd_lib, "p2_square4")
    ctx.mesh_set_dict(m)
    with pytest.raises(fedd_lib.FeddError, match="fedd_assemble_stress: no pattern"):
        ctx.assemble_stress()
    ctx.pattern_build(2, fedd_lib.BLOCK_DIAG)
    with pytest.raises(fedd_lib.FeddError, match="fedd_assemble_stress: assemblyStress needs a FULL pattern with dim dofs per node"):
        ctx.assemble_stress()
    ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    with pytest.raises(fedd_lib.FeddError, match="fedd_assemble_stress: assemblyStress needs a FULL pattern with dim dofs per node"):
        ctx.assemble_stress()
    with pytest.raises(fedd_lib.FeddError, match="assemblyStress needs a FULL pattern"):
        ctx.assemble(fedd_lib.FORM_STRESS)
    ctx.pattern_build(2, fedd_lib.BLOCK_FULL)
    c_q = coeff(m)
    with pytest.raises(fedd_lib.FeddError, match=r"fedd_assemble_stress: n_coeff = %d, but the mesh has 32 elements x 3 quadrature "
                                                 r"points = 96" % (c_q.size - 1)):
        ctx.assemble_stress(c_q.ravel()[:-1])
    ctx.assemble_stress(c_q)                            # and the context still works


def test_solver_state_after_the_call(fedd_lib, ctx, reference):
    """the call is a system-matrix write like every assemble: the Schwarz setup is dropped; a new setup and GMRES solve the
    Dirichlet-constrained stress system, compared with a sparse direct solve as test_gpu_parity.py compares its solves"""
    lib = fedd_lib
    which = "p2_cube4"
    m = mesh(lib, which)
    setup(lib, ctx, m)
    dim = 3
    n = dim * int(m["n_global"])

    def constrain():
        ctx.assemble_rhs([0.3, -1.0, 0.5])
        ctx.dirichlet([1, 2, 3], [0.0] * 9)             # every flagged boundary node (the structured cube's faces, edges, corners)

    ctx.assemble_stress(coeff(m))
    constrain()
    ctx.schwarz_set_target(27, 1.0)
    ctx.schwarz_setup(overlap=1, combine=lib.COMBINE_RESTRICTED)
    r = np.random.default_rng(3).standard_normal(n)
    assert np.isfinite(ctx.schwarz_apply(r)).all()
    ctx.assemble_stress(coeff(m))
    with pytest.raises(lib.FeddError, match="fedd_schwarz_apply: no preconditioner"):
        ctx.schwarz_apply(r)
    constrain()
    ctx.schwarz_setup(overlap=1, combine=lib.COMBINE_RESTRICTED)
    x, its, rel = ctx.gmres(None, rtol=1e-13, max_it=600, restart=200, use_prec=True)
    assert rel <= 1e-13
    A, row_gid = csr_global(ctx, n)
    rhs = np.zeros(n)
    rhs[row_gid] = ctx.rhs_get()
    # the device's constrained rows are unit rows; the restatement's matrix gets the same treatment on the host
    flags = np.zeros(int(m["n_global"]), dtype=np.int32)
    flags[m["gid_uni"]] = m["flag_uni"]
    is_dir = fo.dirichlet_rows(flags, (1, 2, 3), dofs=dim)
    assert is_dir.any() and not is_dir.all()
    K_bc, rhs_bc = fo.set_dirichlet(reference(lib, which, True), np.where(is_dir, 0.0, rhs), is_dir, 0.0)
    assert abs(A - K_bc).max() <= RTOL * abs(K_bc).max()
    xd = np.zeros(n)
    xd[:] = spla.spsolve(K_bc.tocsc(), rhs_bc)
    xg = np.zeros(n)
    xg[row_gid] = x
    np.testing.assert_allclose(xg, xd, rtol=0, atol=RTOL * np.abs(xd).max())

"""fedd_fsi_merge / fedd_fsi_interface_rhs / fedd_fsi_info (include/fedd_hip.h "FSI coupling", feddlib_amd/csrc/fsi.hip) against
the matrix tests/fsi_ref.py builds from the children's fedd_csr_get and the matched table: identical pattern, child values bit
for bit, coupling values exactly 1, -1, -(1.0 / dt).  Fluid: P2 / P1 Stokes on 4 x 4 cells with inflow and wall Dirichlet rows
(the walls include the two corner nodes of the interface); structure: P2 linear elasticity on 4 x 4 cells, clamped at x = 2."""
import numpy as np
import pytest

import fsi_pair
import fsi_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pr(fedd_lib):
    p = fsi_pair.Pair(fedd_lib)
    yield p
    p.close()


def assert_same_csr(got, ref):
    for a, b in zip(got, ref):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_coupled_matrix_and_vectors(pr):
    pr.cpl.fsi_merge(pr.fluid, pr.struct, pr.DT)
    ref, fdof, sdof = pr.host_matrix()
    assert_same_csr(fsi_pair.csr_tuple(pr.cpl), ref)
    info = pr.cpl.fsi_info()
    assert (info["n_u"], info["n_p"], info["n_s"], info["n_l"]) == (pr.n_u, pr.n_p, pr.n_s, pr.n_l)
    assert info["offsets"].tolist() == [0, pr.n_u, pr.n_f, pr.n_f + pr.n_s] and not info["last_values_only"]
    assert pr.n_pairs == 9 and pr.n_l == 18
    # coupling values and the Dirichlet rows: the interface corners are wall nodes of the fluid
    A = fsi_pair.scipy_matrix(fsi_pair.csr_tuple(pr.cpl))
    off = pr.n_f + pr.n_s
    dir_f, dir_s = pr.dirichlet_marks()
    c1t = A[:pr.n_f, off:]
    assert set(c1t.data.tolist()) == {1.0} and c1t.nnz == pr.n_l - int(dir_f[fdof].sum()) and dir_f[fdof].sum() == 4
    assert c1t[np.nonzero(dir_f)[0], :].nnz == 0
    c3t = A[pr.n_f:off, off:]
    assert set(c3t.data.tolist()) == {-1.0} and c3t.nnz == pr.n_l and c3t[np.nonzero(dir_s)[0], :].nnz == 0
    lam = A[off:, :]
    assert lam.nnz == 2 * pr.n_l and set(lam.data.tolist()) == {1.0, -(1.0 / pr.DT)}
    for r in np.nonzero(dir_f)[0]:
        row = A[r, :]
        assert row.data[row.indices == r].tolist() == [1.0] and np.count_nonzero(row.data) == 1
    # the right-hand side is carried over, the lambda part zero; the solution zeroed
    b = pr.cpl.rhs_get()
    assert np.array_equal(b[:pr.n_f], pr.fluid.rhs_get()) and np.array_equal(b[pr.n_f:off], pr.struct.rhs_get())
    assert np.abs(b[pr.n_f:off]).max() > 0 and np.abs(b[:pr.n_f]).max() > 0 and not b[off:].any()
    assert not pr.cpl.solution_get().any()
    # SpMV of the coupled context agrees with the host matrix
    x = np.random.default_rng(1).standard_normal(A.shape[0])
    assert np.abs(pr.cpl.spmv(x) - A @ x).max() <= 1e-12 * np.abs(A @ x).max()


def test_interface_rhs_is_exact(pr):
    pr.cpl.fsi_merge(pr.fluid, pr.struct, pr.DT)
    _, fdof, sdof = pr.host_matrix()
    d_old = np.random.default_rng(2).standard_normal(pr.n_s)
    pr.cpl.fsi_interface_rhs(d_old)
    off = pr.n_f + pr.n_s
    assert np.array_equal(pr.cpl.rhs_get()[off:], fsi_ref.interface_rhs(sdof, d_old, pr.DT))


def test_masked_dofs_carry_the_dummy_diagonal(pr):
    mask = np.ones(pr.n_l, dtype=np.uint8)
    mask[[2, 3, 11]] = 0
    pr.cpl.fsi_merge(pr.fluid, pr.struct, pr.DT, mask)
    ref, fdof, sdof = pr.host_matrix(mask)
    assert_same_csr(fsi_pair.csr_tuple(pr.cpl), ref)
    A = fsi_pair.scipy_matrix(ref)
    off = pr.n_f + pr.n_s
    for k in (2, 3, 11):
        assert A[off + k, :].indices.tolist() == [off + k] and A[off + k, :].data.tolist() == [1.0]
        assert A[:, off + k].nnz == 1
    d_old = np.arange(pr.n_s, dtype=np.float64) + 1.0
    pr.cpl.fsi_interface_rhs(d_old)
    got = pr.cpl.rhs_get()[off:]
    assert np.array_equal(got, fsi_ref.interface_rhs(sdof, d_old, pr.DT)) and not got[[2, 3, 11]].any()
    pr.cpl.fsi_merge(pr.fluid, pr.struct, pr.DT)          # another mask: the pattern is built again
    assert not pr.cpl.fsi_info()["last_values_only"]
    assert_same_csr(fsi_pair.csr_tuple(pr.cpl), pr.host_matrix()[0])


def test_second_merge_moves_values_only(fedd_lib, pr):
    pr.cpl.fsi_merge(pr.fluid, pr.struct, pr.DT)
    n0 = pr.cpl.fsi_info()["n_values_only"]
    pr.struct.matrix_scale(-1, 1.5)
    pr.cpl.fsi_merge(pr.fluid, pr.struct, 2.0 * pr.DT)
    info = pr.cpl.fsi_info()
    assert info["last_values_only"] and info["n_values_only"] == n0 + 1
    got = fsi_pair.csr_tuple(pr.cpl)
    ref, _, _ = pr.host_matrix(dt=2.0 * pr.DT)
    assert_same_csr(got, ref)
    fresh = fedd_lib.Context(device=0)
    try:
        fresh.fsi_merge(pr.fluid, pr.struct, 2.0 * pr.DT)
        assert not fresh.fsi_info()["last_values_only"]
        assert_same_csr(got, fsi_pair.csr_tuple(fresh))
        assert np.array_equal(pr.cpl.rhs_get(), fresh.rhs_get())
    finally:
        fresh.close()
    # a Dirichlet row more on a child changes the coupling pattern: the next merge builds it again, and says so
    pr.struct.dirichlet_nodes(pr.i_s[4:5], np.zeros((1, pr.DIM)))
    pr.cpl.fsi_merge(pr.fluid, pr.struct, pr.DT)
    assert not pr.cpl.fsi_info()["last_values_only"]
    A = fsi_pair.scipy_matrix(fsi_pair.csr_tuple(pr.cpl))
    off = pr.n_f + pr.n_s
    assert A[pr.n_f + pr.DIM * pr.i_s[4], off:].nnz == 0
    pr.structure_system()       # back to the module's structure system
    pr.cpl.fsi_merge(pr.fluid, pr.struct, pr.DT)
    assert_same_csr(fsi_pair.csr_tuple(pr.cpl), pr.host_matrix()[0])


def test_errors(fedd_lib, pr):
    lib = fedd_lib
    other = lib.Context(device=0)
    try:
        with pytest.raises(lib.FeddError, match="no matched interface between exactly these two contexts"):
            pr.cpl.fsi_merge(pr.struct, pr.fluid, pr.DT)
        other.mesh_set_dict(pr.ms)
        with pytest.raises(lib.FeddError, match="no matched interface between exactly these two contexts"):
            pr.cpl.fsi_merge(pr.fluid, other, pr.DT)
        with pytest.raises(lib.FeddError, match="carries a mesh"):
            other.fsi_merge(pr.fluid, pr.struct, pr.DT)
        with pytest.raises(lib.FeddError, match="dt must be positive"):
            pr.cpl.fsi_merge(pr.fluid, pr.struct, 0.0)
    finally:
        other.close()
    # the entries that need a mesh refuse the coupled context by name
    pr.cpl.fsi_merge(pr.fluid, pr.struct, pr.DT)
    for call in (lambda: pr.cpl.schwarz_setup(), lambda: pr.cpl.dirichlet([1], [0.0]), lambda: pr.cpl.dirichlet_rhs([1], [0.0]),
                 lambda: pr.cpl.dirichlet_nodes(np.zeros(1, dtype=np.int32), np.zeros(1))):
        with pytest.raises(lib.FeddError, match="carries no mesh"):
            call()
    # a child without a system, an unmerged fluid
    f2, s2, c2 = lib.Context(device=0), lib.Context(device=0), lib.Context(device=0)
    try:
        f2.mesh_set_dict(pr.mf)
        s2.mesh_set_dict(pr.ms)
        f2.interface_match(s2, [fsi_pair.FLAG])
        with pytest.raises(lib.FeddError, match="the fluid child holds no system"):
            c2.fsi_merge(f2, s2, pr.DT)
        f2.pattern_build(pr.DIM, lib.BLOCK_DIAG)
        f2.assemble(lib.FORM_LAPLACE_VEC)
        with pytest.raises(lib.FeddError, match="the structure child holds no system"):
            c2.fsi_merge(f2, s2, pr.DT)
        s2.pattern_build(pr.DIM, lib.BLOCK_FULL)
        s2.assemble(lib.FORM_LINELAS, [1.0, 1.0])
        with pytest.raises(lib.FeddError, match="unmerged fluid"):
            c2.fsi_merge(f2, s2, pr.DT)
    finally:
        for c in (c2, f2, s2):
            c.close()

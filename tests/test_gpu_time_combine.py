"""fedd_matrix_combine and fedd_matrix_apply (timestep.hip) against numpy / scipy on the read-back blocks.

Combine: fedd_csr_get after the combine equals (cm * M) + (ca * A), M scattered into A's pattern with 0.0 where it has no
entry, BIT FOR BIT (two separately rounded products, then one sum: numpy does the same, nothing is fused on either side);
rowptr / colind are A's; a second combine with other coefficients keeps the Schwarz structure stage.
Apply: against scipy's product of the read-back block to 1e-14 * ||M||_inf * ||x||_inf -- a few rounding errors of a row sum of
at most 81 terms (81 * 2^-53 = 9e-15 bounds the sum of any order) -- and two calls agree bitwise."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

DT, BETA = 0.025, 0.25
CM = 1.0 / ((DT * DT) * BETA)

MESHES = ["3d_p1_4", "2d_p1_5", "2d_p2_4", "3d_p1_12"]
_MESH = {}


def mesh(fedd_lib, name):
    if name not in _MESH:
        if name == "3d_p1_4":
            _MESH[name] = fedd_lib.structured_mesh(3, 1, 4)
        elif name == "3d_p1_12":
            _MESH[name] = fedd_lib.structured_mesh(3, 1, 12)
        elif name == "2d_p1_5":
            _MESH[name] = fedd_lib.structured_mesh(2, 1, 5)
        else:
            _MESH[name] = fedd_lib.p2_of_p1(fedd_lib.structured_mesh(2, 1, 4), volume_id=10)
    return _MESH[name]


def store(fedd_lib, c, dofs, mode, form, params, slot, scale=None):
    c.pattern_build(dofs, mode)
    c.assemble(form, params)
    if scale is not None:
        c.matrix_scale(-1, scale)
    c.matrix_store(slot)


def pairing(fedd_lib, c, dim, pair, a_last):
    """slot 0 <- M, slot 1 <- A; a_last: A is stored last, so the system slot already holds its pattern"""
    L = fedd_lib
    lam_mu = [2.0e6, 0.5e6]
    if pair == "scalar":
        jobs = [(1, L.BLOCK_SCALAR, L.FORM_MASS, None, 0), (1, L.BLOCK_SCALAR, L.FORM_LAPLACE, None, 1)]
    elif pair == "diag_diag":
        jobs = [(dim, L.BLOCK_DIAG, L.FORM_MASS_VEC, None, 0), (dim, L.BLOCK_DIAG, L.FORM_LAPLACE_VEC, None, 1)]
    else:
        jobs = [(dim, L.BLOCK_DIAG, L.FORM_MASS_VEC, None, 0), (dim, L.BLOCK_FULL, L.FORM_LINELAS, lam_mu, 1)]
    for j in (jobs if a_last else jobs[::-1]):
        store(L, c, *j, scale=1000.0 if j[4] == 0 else None)


def scatter(M, A):
    """M's values at the positions of A's stored entries (0.0 where M has none)"""
    M = M.tocsr(); A = A.tocsr()
    nc = A.shape[1]
    ka = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr)) * nc + A.indices
    km = np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr)) * nc + M.indices
    assert np.all(np.diff(ka) > 0) and np.all(np.diff(km) > 0)          # rows ascending, columns ascending within a row
    pos = np.searchsorted(ka, km)
    assert np.array_equal(ka[pos], km), "M has an entry outside A's pattern"
    out = np.zeros(A.nnz)
    out[pos] = M.data
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("a_last", [True, False])
@pytest.mark.parametrize("pair", ["scalar", "diag_diag", "diag_full"])
@pytest.mark.parametrize("name", MESHES)
def test_combine_bit_for_bit(fedd_lib, name, pair, a_last):
    m = mesh(fedd_lib, name)
    c = fedd_lib.Context(device=0)
    try:
        c.mesh_set_dict(m)
        pairing(fedd_lib, c, m["dim"], pair, a_last)
        M, A = c.matrix_get(0), c.matrix_get(1)
        mfull = scatter(M, A)
        if pair == "diag_full":
            assert A.nnz == M.nnz * m["dim"] and np.count_nonzero(mfull == 0.0) >= A.nnz - M.nnz
        gen0 = None
        for k, (cm, ca) in enumerate([(CM, 1.0), (1.0 / ((0.0125 * 0.0125) * 0.3), 0.75)]):
            c.matrix_combine(0, cm, 1, ca)
            assert c.matrix_combine_current(0, cm, 1, ca) and not c.matrix_combine_current(0, cm, 1, ca + 1.0)
            rowptr, col, val, _ = c.csr_get()
            assert np.array_equal(rowptr, A.indptr) and np.array_equal(col, A.indices)
            expect = (cm * mfull) + (ca * A.data)
            nz = int(np.count_nonzero(val == 0.0))
            print(name, pair, "a_last", a_last, "combine", k, "nnz", A.nnz, "stored zeros", nz,
                  "differing entries", int(np.count_nonzero(bits(val) != bits(expect))))
            assert np.array_equal(bits(val), bits(expect))
            assert nz == int(np.count_nonzero(expect == 0.0))           # the structural zeros are there, as zeros
            # the Schwarz structure stage survives the second combine
            flags = [2]
            c.dirichlet(flags, np.zeros(len(flags) * c.dofs))
            c.schwarz_setup(1, fedd_lib.COMBINE_FULL)
            info = c.schwarz_reuse_info()
            if k == 0:
                gen0 = info["n_reused"]
            else:
                assert info["last_reused"] and info["n_reused"] == gen0 + 1, info
        # a write to a slot ends "current"
        c.matrix_scale(0, 2.0)
        assert not c.matrix_combine_current(0, cm, 1, ca)
    finally:
        c.close()


def test_combine_keeps_rhs_and_solution_resets_dirichlet(fedd_lib):
    m = mesh(fedd_lib, "3d_p1_4")
    c = fedd_lib.Context(device=0)
    try:
        c.mesh_set_dict(m)
        pairing(fedd_lib, c, 3, "diag_full", True)
        n = c.csr_sizes()[0]
        rng = np.random.default_rng(11)
        b, x = rng.standard_normal(n), rng.standard_normal(n)
        c.rhs_set(b)
        c.solution_set(x)
        c.dirichlet([2], np.zeros(3))
        c.matrix_combine(0, CM, 1, 1.0)
        assert np.array_equal(c.solution_get(), x)
        got = c.rhs_get()
        flag2 = np.repeat(m["flag_uni"] == 2, 3)
        assert np.array_equal(got[~flag2], b[~flag2]) and np.all(got[flag2] == 0.0)   # (what fedd_dirichlet wrote stays too)
        # the Dirichlet rows are real rows again
        A = c.matrix_get(1)
        rowptr, col, val, _ = c.csr_get()
        expect = (CM * scatter(c.matrix_get(0), A)) + (1.0 * A.data)
        assert np.array_equal(bits(val), bits(expect))
        # rhs_axpy: rhs + (alpha * f), one product and one sum
        f = rng.standard_normal(n)
        c.rhs_axpy(-0.7, f)
        assert np.array_equal(bits(c.rhs_get()), bits(got + (-0.7 * f)))
        # dirichlet_rhs touches the flagged rows of the right-hand side only
        c.dirichlet([2], np.zeros(3))
        before = c.csr_get()[2]
        c.rhs_set(b)
        c.dirichlet_rhs([2], [1.0, 2.0, 3.0])
        got = c.rhs_get()
        assert np.array_equal(got[~flag2], b[~flag2]) and np.array_equal(got[flag2].reshape(-1, 3), np.tile([1.0, 2.0, 3.0], (flag2.sum() // 3, 1)))
        assert np.array_equal(bits(c.csr_get()[2]), bits(before))
    finally:
        c.close()


@pytest.mark.parametrize("name", MESHES)
def test_block_apply(fedd_lib, name):
    m = mesh(fedd_lib, name)
    dim = m["dim"]
    L = fedd_lib
    c = L.Context(device=0)
    try:
        c.mesh_set_dict(m)
        store(L, c, 1, L.BLOCK_SCALAR, L.FORM_MASS, None, 2)
        store(L, c, dim, L.BLOCK_DIAG, L.FORM_MASS_VEC, None, 0, scale=1000.0)
        store(L, c, dim, L.BLOCK_FULL, L.FORM_LINELAS, [2.0e6, 0.5e6], 1)
        rng = np.random.default_rng(5)
        for slot in (2, 0, 1):
            M = c.matrix_get(slot)
            x = rng.standard_normal(M.shape[1])
            y = c.matrix_apply(slot, x)
            ref = M @ x
            norm_inf = np.abs(M).sum(axis=1).max()
            tol = 1e-14 * norm_inf * np.abs(x).max()
            err = np.abs(y - ref).max()
            print(name, "slot", slot, "rows", M.shape[0], "longest row", int(np.diff(M.indptr).max()), "err %.3e tol %.3e" % (err, tol))
            assert int(np.diff(M.indptr).max()) <= 81 or name == "2d_p2_4"
            assert err <= tol
            assert np.array_equal(bits(c.matrix_apply(slot, x)), bits(y))
            ya = c.matrix_apply(slot, x, alpha=-2.5)
            assert np.array_equal(bits(ya), bits(-2.5 * y))             # alpha multiplies the finished row sum
    finally:
        c.close()

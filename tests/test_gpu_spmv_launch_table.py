"""Every row of the SpMV's launch tables (spmv.hip: SPMV_WIN, SPMV_PAT, SPMV_CLS, SPMV_LPR, CS_REUSE) is reached by a case.

    table row                                   reached by
    SPMV_WIN[NT=0][NU 4, 6, 8] c32 | c16        test_gpu_edge_cases.test_spmv_sixteen_bit_columns_give_the_same_bits
    SPMV_WIN[NT=0][NU 5, 7]    c32 | c16        test_window_rows below
    SPMV_WIN[NT=1][NU 4 ... 8] c32 | c16        test_window_rows below
    SPMV_WIN[NT=0 | 1][8] c32, parity CSR       test_gpu_launch_shapes (spmv_nt 0 / 1 on the public product), test_window_rows
    SPMV_PAT[NT=0][NU 2 ... 8] lu8              test_gpu_edge_cases.test_spmv_column_patterns_give_the_same_bits (scalar systems)
    SPMV_PAT[NT=0][NU 2 ... 8] lu16             test_pattern_rows below (2D two-dof elasticity: 14 entries per row)
    SPMV_PAT[NT=1][NU 2 ... 8] lu8 | lu16       test_pattern_rows below
    SPMV_CLS (4, 8) | (4, 16) | (2, 48)         test_gpu_edge_cases.test_spmv_row_classes_give_the_same_bits: scalar Laplace (7 / 5
                                                entries per row) | 2D two-dof elasticity (14) | 3D elasticity (45)
    SPMV_CLS_LDS (4, 8) | (4, 16) | (2, 48)     test_gpu_spmv_cls_lds: per stride, listed and flagged blocks in one launch.  Within
                                                (4, 8), cls_row takes a wave of 64 rows by its kind (test_gpu_spmv_cls_waves,
                                                bit for bit against a host product; the lattices are named there):
      (a) one pattern, 7 entries, x from lanes    lattice A (every block listed), B (cap forced low: flagged blocks), E (default gates)
      (b) one pattern, 5 entries, x from lanes    lattice C; lattices A and B without Dirichlet rows (an edge along x)
      (c) one pattern, middle offsets no run      lattice D (7 entries); lattices A and B without Dirichlet rows (5: the other x-edges)
      (d) one length of 7 / 5, several patterns   lattice D (7 entries)
      (e) one pattern, 6 or 4 entries             lattices A, B without Dirichlet rows and E (6: a face); C without Dirichlet rows (4)
    SPMV_LPR 4 | 8 | 16 | 32 | 64               test_lane_group_rows below, one system per bracket of the average row length
                                                (test_gpu_edge_cases.test_spmv_kernels_agree reaches 8 and 16 without saying so)
    CS_REUSE[REFRESH=0 | 1]                     test_gpu_spmv_reuse (streams built with | without the class stage)

The window, pattern and class kernels form the same products in the same order as the per-entry kernel with spmv_nt 0: bit for
bit against it, on the same context.  The lane-group kernel sums a row in another order: against fo.spmv on the matrix read back
from the device, within len_i 2^-52 (|A| |x|)_i per row, which bounds the difference of ANY two summation orders of len_i
products (each order is within (len_i - 1) u (|A| |x|)_i of the exact sum, u = 2^-53, to first order; scipy's order and a
reversed and a strided-tree order of the same products stay below 0.25 of the bound on these systems, checked with numpy)."""
import numpy as np
import pytest
import scipy.sparse as sp

import fedd_oracle as fo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def system(L, c, kind, dim, M):
    """assembles on c; returns a random x of the system's length"""
    m = L.structured_mesh(dim, 1, M)
    if kind == "linelas_p2":
        m = L.p2_of_p1(m, volume_id=0)
    c.mesh_set_dict(m)
    if kind == "laplace":
        c.pattern_build(1, L.BLOCK_SCALAR)
        c.assemble(L.FORM_LAPLACE)
        c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    else:
        c.pattern_build(dim, L.BLOCK_FULL)
        c.assemble(L.FORM_LINELAS, [1.5, 1.0])
        if kind == "linelas":
            c.dirichlet([2], np.zeros(dim))
    return np.random.default_rng(dim * 100 + M).standard_normal(c.csr_sizes()[0])


def restore(c):
    for key, v in (("spmv_nt", -1), ("spmv_pattern", 1), ("spmv_classes", 1), ("spmv_col16", 1), ("spmv_win_nu", 0), ("spmv_pat_nu", 0),
                   ("spmv_compact", 1), ("spmv_kind", 0), ("spmv_exact_public", 1)):
        c.set_option(key, v)


@pytest.mark.parametrize("kind,dim,M", [("laplace", 3, 20), ("linelas", 3, 10)])
def test_window_rows(fedd_lib, ctx, kind, dim, M):
    """k_spmv_win<NT, NU, C16> on the compacted stream for NT 0 / 1, NU 4 ... 8 and both column widths, and on the parity CSR"""
    x = system(fedd_lib, ctx, kind, dim, M)
    try:
        ctx.set_option("spmv_exact_public", 0)      # fedd_spmv = the solver's stream in this test
        ctx.set_option("spmv_pattern", 0)
        ctx.set_option("spmv_nt", 0)
        ctx.set_option("spmv_col16", 0)
        y0 = ctx.spmv(x)
        assert ctx.spmv_info()["column_index_bytes"] == 4 and ctx.spmv_info()["column_patterns"] == 0
        for nt in (0, 1):
            ctx.set_option("spmv_nt", nt)
            for c16 in (0, 1):
                ctx.set_option("spmv_col16", c16)
                for nu in (4, 5, 6, 7, 8):
                    ctx.set_option("spmv_win_nu", nu)
                    y = ctx.spmv(x)
                    info = ctx.spmv_info()
                    assert info["column_index_bytes"] == (2 if c16 else 4) and info["column_patterns"] == 0, (nt, c16, nu, info)
                    assert np.array_equal(y, y0), (nt, c16, nu)
        # the parity CSR through the same kernel (NU 8, 32-bit columns) at drop tolerance 0: the same entries but the exact zeros
        ctx.set_option("spmv_drop_tol", 0.0)
        ctx.set_option("spmv_nt", 0)
        ye = ctx.spmv(x)
        ctx.set_option("spmv_compact", 0)
        for nt in (0, 1):
            ctx.set_option("spmv_nt", nt)
            assert np.array_equal(ctx.spmv(x), ye), nt
            assert ctx.spmv_info()["nnz_streamed"] == ctx.spmv_info()["nnz_pattern"]
    finally:
        ctx.set_option("spmv_drop_tol", 2.0 ** -52)
        restore(ctx)


@pytest.mark.parametrize("kind,dim,M,lu", [("laplace", 3, 20, 8), ("linelas", 2, 40, 16)])
def test_pattern_rows(fedd_lib, ctx, kind, dim, M, lu):
    """k_spmv_pat<NT, NU, LU> for NT 0 / 1 and NU 2 ... 8: LU 8 where no row has more than 8 entries (3D scalar Laplace: 7),
    SPAT_LK = 16 above (2D elasticity with full node blocks: 2 x 7)"""
    x = system(fedd_lib, ctx, kind, dim, M)
    rowptr, _, val, _ = ctx.csr_get()
    try:
        ctx.set_option("spmv_exact_public", 0)
        ctx.set_option("spmv_classes", 0)
        ctx.set_option("spmv_pattern", 0)
        ctx.set_option("spmv_nt", 0)
        y0 = ctx.spmv(x)
        assert ctx.spmv_info()["column_patterns"] == 0
        ctx.set_option("spmv_pattern", 2)
        for nt in (0, 1):
            ctx.set_option("spmv_nt", nt)
            for nu in (2, 3, 4, 5, 6, 7, 8):
                ctx.set_option("spmv_pat_nu", nu)
                y = ctx.spmv(x)
                info = ctx.spmv_info()
                # the pattern kernel ran: a dictionary without classes, and no column index is streamed
                assert info["column_patterns"] >= 1 and info["row_classes"] == 0 and info["column_index_bytes"] == 0, (nt, nu, info)
                assert np.array_equal(y, y0), (nt, nu)
        # the unroll follows the longest pattern of the compacted stream (entries above one ulp of their row's largest).  No row
        # is longer than 8: LU 8; most rows are longer (and at most a quarter of the rows is without a pattern): SPAT_LK
        row_of = np.repeat(np.arange(x.shape[0]), np.diff(rowptr))
        rowmax = np.zeros(x.shape[0])
        np.maximum.at(rowmax, row_of, np.abs(val))
        kept = np.bincount(row_of[np.abs(val) > 2.0 ** -52 * rowmax[row_of]], minlength=x.shape[0])
        if lu == 8:
            assert kept.max() <= 8, kept.max()
        else:
            assert kept.max() <= 16 and np.count_nonzero(kept > 8) > 0.75 * x.shape[0], np.bincount(kept)
    finally:
        restore(ctx)


# (system, dim, cells per direction, lane group the average row length selects)
LPR_CASES = [("laplace", 2, 1, 4), ("laplace", 2, 6, 8), ("linelas", 2, 6, 16), ("linelas", 3, 4, 32), ("linelas_p2", 3, 2, 64)]


@pytest.mark.parametrize("kind,dim,M,lpr", LPR_CASES)
def test_lane_group_rows(fedd_lib, ctx, kind, dim, M, lpr):
    """k_spmv<LPR> (spmv_kind 1): one system per bracket of nnz / n_rows -- <= 4, <= 10, <= 24, <= 48, above"""
    x = system(fedd_lib, ctx, kind, dim, M)
    n, n_cols, nnz = ctx.csr_sizes()
    avg = nnz / n
    bracket = 4 if avg <= 4.0 else 8 if avg <= 10.0 else 16 if avg <= 24.0 else 32 if avg <= 48.0 else 64
    print("avg row length %.2f -> k_spmv<%d>" % (avg, bracket))
    assert bracket == lpr, (avg, bracket)
    rowptr, col, val, _ = ctx.csr_get()
    A = sp.csr_matrix((val, col, rowptr), shape=(n, n_cols))
    yo = fo.spmv(A, x)
    bound = np.diff(rowptr) * 2.0 ** -52 * (abs(A) @ np.abs(x))
    try:
        ctx.set_option("spmv_kind", 1)
        y = ctx.spmv(x)
    finally:
        restore(ctx)
    worst = float(np.max(np.abs(y - yo) - bound))
    print("largest |y - y_ref| %.3e, largest excess over the row bound %.3e" % (np.abs(y - yo).max(), worst))
    assert np.all(np.abs(y - yo) <= bound)
    assert np.abs(yo).max() > 0


def test_setting_a_deciding_option_drops_the_stream(fedd_lib, ctx):
    """The stream records the kernel it takes at its build; the queries and the dispatch no longer re-test "spmv_pattern" and
    "spmv_classes".  That is sound because setting either drops the stream and its key at once: the queries stop reporting the
    dropped stream before any product, and the next product builds (not keeps) a stream on the other path."""
    x = system(fedd_lib, ctx, "laplace", 3, 20)
    try:
        ctx.set_option("spmv_exact_public", 0)
        ctx.set_option("spmv_pattern", 2)
        y0 = ctx.spmv(x)
        info = ctx.spmv_info()
        assert info["row_classes"] >= 1 and info["column_patterns"] >= 1, info
        kept = ctx.spmv_reuse_info()["n_reused"]
        ctx.set_option("spmv_classes", 0)
        info = ctx.spmv_info()
        assert info["row_classes"] == 0 and info["column_patterns"] == 0, info      # dropped: nothing is reported as in use
        assert np.array_equal(ctx.spmv(x), y0)
        info = ctx.spmv_info()
        assert info["row_classes"] == 0 and info["column_patterns"] >= 1 and info["column_index_bytes"] == 0, info
        ctx.set_option("spmv_pattern", 0)
        assert ctx.spmv_info()["column_patterns"] == 0
        assert np.array_equal(ctx.spmv(x), y0)
        info = ctx.spmv_info()
        assert info["column_patterns"] == 0 and info["column_index_bytes"] == 2, info
        assert ctx.spmv_reuse_info() == {"last_reused": False, "n_reused": kept}        # both were builds: the key went too
    finally:
        restore(ctx)

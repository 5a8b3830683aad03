"""Option spmv_cls_lds: the class SpMV with its block's class values in LDS and unit-stride x from the neighbouring lanes
(k_spmv_cls_lds) gives the y of k_spmv_cls bit for bit -- on the smallest grids that build row classes by default (65 536 rows),
for the three strides of the class table, with every block on the LDS path and with the cap forced low (flagged blocks and
blocks with a list in one launch), and through a preconditioned s-step solve."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (name, dim, cells per side, dofs per node, rows, table stride, rows per block of the kernel that takes the stride)
CASES = [("laplace3d", 3, 41, 1, 74088, 8, 1024),       # lines of 42 nodes: every wave mixes interior and Dirichlet rows
         ("laplace2d", 2, 256, 1, 66049, 8, 1024),      # 5-entry rows
         ("linelas3d", 3, 27, 3, 65856, 48, 512)]       # 3 x 15 entries per row: the widest stride
LOW_CAPS = (48, 24, 12, 6, 3, 1)


@pytest.fixture(scope="module")
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def system(fedd_lib, ctx, dim, M, dofs):
    ctx.mesh_set_dict(fedd_lib.structured_mesh(dim, 1, M))
    if dofs == 1:
        ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
        ctx.assemble(fedd_lib.FORM_LAPLACE)
        ctx.assemble_rhs([1.0])
        ctx.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    else:
        ctx.pattern_build(dofs, fedd_lib.BLOCK_FULL)
        ctx.assemble(fedd_lib.FORM_LINELAS, [1.5e6, 1.0e6])
        ctx.assemble_rhs([0.0, 1.0, 0.0][:dofs])
        ctx.dirichlet([2], np.zeros(dofs))
    return ctx.csr_sizes()[0]


def product(ctx, x, lds, cap=0):
    ctx.set_option("spmv_cls_lds", lds)
    ctx.set_option("spmv_cls_lds_cap", cap)
    return ctx.spmv(x), ctx.spmv_info()


@pytest.mark.parametrize("name,dim,M,dofs,rows,stride,per_block", CASES, ids=[c[0] for c in CASES])
def test_lds_path_gives_the_bits_of_the_table_path(fedd_lib, ctx, name, dim, M, dofs, rows, stride, per_block):
    nr = system(fedd_lib, ctx, dim, M, dofs)
    assert nr == rows and nr % 1024 != 0 and nr % per_block != 0      # (the last block is a partial one)
    nblk = -(-nr // per_block)
    x = np.random.default_rng(1909).standard_normal(nr)
    ctx.set_option("spmv_exact_public", 0)      # fedd_spmv = the solver's stream
    try:
        y0, info0 = product(ctx, x, 0)
        assert info0["row_classes"] >= 1 and info0["rows_in_classes"] >= 0.9 * nr, info0
        assert info0["class_blocks_lds"] == 0 and info0["class_blocks_fallback"] == 0, info0
        y1, info1 = product(ctx, x, 1)
        print("%s: %d rows, %d blocks; lds 0: %s; lds 1: %s" % (name, nr, nblk, info0, info1))
        assert info1["row_classes"] == info0["row_classes"] and info1["rows_in_classes"] == info0["rows_in_classes"]
        assert info1["class_blocks_lds"] >= 1 and info1["class_blocks_lds"] + info1["class_blocks_fallback"] == nblk, info1
        assert np.array_equal(y1, y0)
        # the cap forced low: flagged blocks and blocks with a list in one launch (a block of one class -- a boundary face --
        # keeps its list down to a cap of one)
        mixed = 0
        for cap in LOW_CAPS:
            yc, infoc = product(ctx, x, 1, cap)
            print("%s: cap %d: %d blocks with a list, %d flagged" % (name, cap, infoc["class_blocks_lds"], infoc["class_blocks_fallback"]))
            assert infoc["class_blocks_lds"] + infoc["class_blocks_fallback"] == nblk, (cap, infoc)
            assert infoc["class_blocks_lds"] <= info1["class_blocks_lds"], (cap, infoc, info1)
            assert np.array_equal(yc, y0), cap
            mixed += 1 if infoc["class_blocks_lds"] >= 1 and infoc["class_blocks_fallback"] >= 1 else 0
        if info1["row_classes"] > 2:
            assert mixed >= 1
        else:
            # (256 cells per side: h is a power of two, the arithmetic exact, and the two classes -- interior, Dirichlet -- are in
            # every block of four grid lines: no cap separates the blocks; at one class per list every block is flagged)
            assert infoc["class_blocks_lds"] == 0 and infoc["class_blocks_fallback"] == nblk, infoc
        # the default cap again: the lists are rebuilt for it
        y2, info2 = product(ctx, x, 1)
        assert np.array_equal(y2, y0) and info2 == info1
    finally:
        ctx.set_option("spmv_cls_lds", 1)
        ctx.set_option("spmv_cls_lds_cap", 0)
        ctx.set_option("spmv_exact_public", 1)


def test_a_preconditioned_s_step_solve_is_the_same_solve(fedd_lib, ctx):
    """more than 16 iterations with s = 16: the shifted epilogue of the Newton basis runs on both kernels"""
    nr = system(fedd_lib, ctx, 3, 41, 1)
    ctx.schwarz_set_target(27, 1.0)
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    ctx.set_option("gmres_s", 16)
    try:
        sol = {}
        for lds in (0, 1):
            ctx.set_option("spmv_cls_lds", lds)
            xs, its, rel = ctx.gmres(None, rtol=1e-10, max_it=400, restart=100, use_prec=True)
            sol[lds] = (xs, its, rel, ctx.gmres_info(), ctx.spmv_info())
            print("spmv_cls_lds %d: %d iterations, relres %.3e, %s" % (lds, its, rel, sol[lds][3]))
        assert sol[1][4]["class_blocks_lds"] >= 1 and sol[0][4]["class_blocks_lds"] == 0
        assert sol[0][1] == sol[1][1] > 16 and sol[0][2] == sol[1][2]
        assert sol[0][3] == sol[1][3] and sol[0][3]["blocks"] >= 2
        assert np.array_equal(sol[0][0], sol[1][0]) and sol[0][0].shape == (nr,)
    finally:
        ctx.set_option("spmv_cls_lds", 1)
        ctx.set_option("gmres_s", 0)

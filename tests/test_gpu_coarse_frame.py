"""The shapes of the GDSW setup that the other small tests do not reach, against the oracle's CoarseGDSW + RAS at the tolerances of
test_gpu_two_level.py: the stacked Galerkin product with more than one chunk of rows per cell, and the column kernels in 2D at
both their widths (one column, sixteen with a partly filled last batch)."""
import functools

import numpy as np
import pytest

import fedd_oracle as fo
from test_gpu_parity import oracle_mesh

pytestmark = pytest.mark.gpu


def coarse_and_apply(fedd_lib, c, kind, block, rot=0):
    """(cells per direction, K0^-1, one two-level apply of a seeded r) with the extensions solved to 1e-13"""
    c.set_option("gdsw_block", block)
    c.set_option("gdsw_rotations", rot)
    c.set_option("gdsw_tol", 1e-13)
    c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED, two_level=1,
                    coarse_kind=fedd_lib.COARSE_RGDSW if kind == "rgdsw" else fedd_lib.COARSE_GDSW)
    g, Kinv = c.schwarz_coarse()
    r = np.random.default_rng(5).standard_normal(c.csr_sizes()[0])
    return g, Kinv, c.schwarz_apply(r), r


def check_stacked_ran(Kinv, z, Kinv0, z0):
    """gdsw_block 1 stacks only under the defaults (s-step GMRES, subdomains that multi_rhs_ok takes) and the context does not say
    which path ran.  A stacked solve rounds differently from sixteen single ones: results equal to the last bit mean that
    block 1 fell back to the one-column path.  Beyond that the two widths agree at the 1e-10 of
    test_extension_solves_sixteen_columns_at_a_time."""
    assert not (np.array_equal(Kinv, Kinv0) and np.array_equal(z, z0)), "gdsw_block 1 ran the one-column path"
    np.testing.assert_allclose(Kinv, Kinv0, rtol=0, atol=1e-10 * np.abs(Kinv0).max())
    np.testing.assert_allclose(z, z0, rtol=0, atol=1e-10 * np.abs(z0).max())


def check_against_oracle(Kinv, z, r, co, ras):
    assert Kinv.shape == (co.n0, co.n0)
    np.testing.assert_allclose(Kinv, co.K0inv, rtol=0, atol=1e-10 * np.abs(co.K0inv).max())
    zo = ras.apply(r) + co.apply(r)
    np.testing.assert_allclose(z, zo, rtol=0, atol=1e-10 * np.abs(zo).max())


@pytest.mark.parametrize("kind", ["gdsw", "rgdsw"])
def test_stacked_galerkin_product_in_two_chunks(fedd_lib, kind):
    """The stacked product splits the rows of a cell into nch = min(64, max(1, (n_rows / ncell + 2047) / 2048)) chunks (integer
    division).  3D Laplace on 26^3 nodes with 2^3 cells: 17576 / 8 = 2197 rows per cell, nch = (2197 + 2047) / 2048 = 2, and a
    chunk is the rows' half rounded up to a multiple of 4, so the second one is ragged.  The context does not expose nch: the
    test asserts the arithmetic it rests on, and that the stacked path ran (check_stacked_ran).  (RGDSW has one coarse node
    here, n0 = 1: it pins the chunked restriction of its 8 slots, little of the scatter.)"""
    c = fedd_lib.Context(device=0)
    try:
        m = fedd_lib.structured_mesh(3, 1, 25)
        c.mesh_set_dict(m)
        c.pattern_build(1, fedd_lib.BLOCK_SCALAR)
        c.assemble(fedd_lib.FORM_LAPLACE)
        c.assemble_rhs([1.0])
        c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
        c.schwarz_set_target(27, 1.0)
        c.schwarz_set_coarse(8)
        g, Kinv, z, r = coarse_and_apply(fedd_lib, c, kind, block=1)
        n_rows, ncell = r.shape[0], int(np.prod(g[:3]))
        assert ncell == 8 and n_rows // ncell > 2048 and (n_rows // ncell + 2047) // 2048 == 2, (n_rows, ncell)
        A_bc, _, _, _, flags = fo.laplace_problem(oracle_mesh(m), bc_flags=(1, 2, 3))
        co = fo.CoarseGDSW(A_bc, m["conn"], m["xyz"], np.isin(flags, (1, 2, 3)), 1, cells_target=8, reduced=kind == "rgdsw")
        np.testing.assert_array_equal(g[:3], co.g)
        node_bin, nb, _ = fo.schwarz_bins(m["xyz"], 27)
        check_against_oracle(Kinv, z, r, co, fo.RAS(A_bc, node_bin, nb))
        _, Kinv0, z0, _ = coarse_and_apply(fedd_lib, c, kind, block=0)
        check_stacked_ran(Kinv, z, Kinv0, z0)
    finally:
        c.close()


# ---- 2D elasticity, M = 24, 16 cells: the oracle once per (kind, rotations), the device once per (kind, rotations, block) ----
MU, NU = 2.0e6, 0.4


@functools.lru_cache(maxsize=None)
def elasticity_2d_oracle(kind, rot):
    m = fo.build_mesh_structured(2, 1, 24)
    A_bc, _, _, _, flags = fo.linelas_problem(m, MU, NU, f=(0.0, 1.0))
    co = fo.CoarseGDSW(A_bc, m.conn, m.xyz, fo.dirichlet_rows(flags, (2,), dofs=2), 2, cells_target=16, reduced=kind == "rgdsw",
                       rotations=bool(rot))
    node_bin, nb, _ = fo.schwarz_bins(m.xyz, 9)
    return co, fo.RAS(A_bc, node_bin, nb, dofs=2)


@pytest.fixture(scope="module")
def elasticity_2d_device(fedd_lib):
    """(kind, rot, block) -> coarse_and_apply of that setup, computed once per module"""
    @functools.lru_cache(maxsize=None)
    def get(kind, rot, block):
        c = fedd_lib.Context(device=0)
        try:
            m = fedd_lib.structured_mesh(2, 1, 24)
            c.mesh_set_dict(m)
            c.pattern_build(2, fedd_lib.BLOCK_FULL)
            c.assemble(fedd_lib.FORM_LINELAS, [2.0 * MU * NU / (1.0 - 2.0 * NU), MU])
            c.assemble_rhs([0.0, 1.0])
            c.dirichlet([2], [0.0, 0.0])
            c.schwarz_set_target(9, 1.0)
            c.schwarz_set_coarse(16)
            return coarse_and_apply(fedd_lib, c, kind, block, rot)
        finally:
            c.close()
    return get


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("kind", ["gdsw", "rgdsw"])
def test_columns_one_by_one_in_2d(elasticity_2d_device, kind, rot):
    """gdsw_block 0: every column kernel at NR = 1 with DIM = 2 (extensions and Galerkin product a column per sweep)"""
    co, ras = elasticity_2d_oracle(kind, rot)
    g, Kinv, z, r = elasticity_2d_device(kind, rot, 0)
    np.testing.assert_array_equal(g[:2], co.g)
    check_against_oracle(Kinv, z, r, co, ras)


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("kind", ["gdsw", "rgdsw"])
def test_sixteen_columns_with_a_partly_filled_batch_in_2d(elasticity_2d_device, kind, rot):
    """gdsw_block 1 on the same systems: the column kernels at NR = 16 with DIM = 2.  GDSW has 8 classes x 2 (3) functions = 16 (24,
    in two batches of 12) extension columns and 25 colours x 2 (3) = 50 (75) product columns, RGDSW 4 x 2 (3) and 9 x 2 (3): the
    last batch is never full.  And the stacked path ran and agrees with the one-column path (check_stacked_ran)."""
    co, ras = elasticity_2d_oracle(kind, rot)
    g, Kinv, z, r = elasticity_2d_device(kind, rot, 1)
    check_against_oracle(Kinv, z, r, co, ras)
    _, Kinv0, z0, _ = elasticity_2d_device(kind, rot, 0)
    check_stacked_ran(Kinv, z, Kinv0, z0)

"""The lane-group row walk over a stored CSR (feddlib_amd/csrc/stored_rows.hpp) where no other bit-for-bit test reaches it,
and the child link that the block preconditioner and FaCSI share.

Which (kernel, G) the other tests pin bit for bit -- G = 8 while the longest row has at most 32 entries, else 16:
    k_block_apply<8>            test_gpu_time_multistep.py against block_apply_rowwalk (DIAG mass, rows of at most 15)
    k_block_apply<16>           none: HERE, against block_apply_rowwalk
    k_newton_residual<8 | 16>   test_gpu_newton_newmark.py against fedd_matrix_apply, with and without source (2D FULL rows of 14,
                                3D P1 FULL rows of up to 45); the mass term alone HERE
    k_bt_sub<8>                 test_gpu_blockprec.py against fedd_matrix_apply; B^T rows of P2 / P1 do not exceed 32 on the
                                meshes at hand, so k_bt_sub<16> has no case
    k_facsi_rows<16>            test_gpu_fsi_facsi.py to 1e-10 only (the structure's 2D P2 FULL rows have up to 38 entries): HERE
                                bit for bit; k_facsi_rows<8> needs a pair whose every row has at most 32 entries and has no case
Shapes: 2D P1 FULL on structured_mesh(2, 1, 2) -- 18 rows of at most 14 entries, G = 8, one pass of the trip loop; 3D P2 FULL on
one cell of the structured cube -- 81 rows (odd: the last workgroup of 6 has dead lane groups), the longest with 81 entries,
G = 16, two passes of the trip loop of 64 with one entry in the last trip."""
import numpy as np
import pytest

import fsi_pair
import hyperelastic_ref as hr
from test_gpu_hyperelastic import model_id, own_dofs, smooth_displacement
from test_gpu_time_multistep import block_apply_rowwalk

pytestmark = pytest.mark.gpu

SLOT_MD, SLOT_A, SLOT_MF = 0, 1, 2
CASES = {"2d_p1_full": (8, 14, 18), "3d_p2_full": (16, 81, 81)}      # G, longest row, rows


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_state = {}


def stored(lib, which):
    """(context, mesh) with slot 0: DIAG mass, slot 1: linear elasticity (FULL), slot 2: the mass on the FULL pattern"""
    if which not in _state:
        m = lib.structured_mesh(2, 1, 2) if which == "2d_p1_full" else lib.p2_of_p1(lib.structured_mesh(3, 1, 1), volume_id=0)
        c = lib.Context(device=0)
        c.mesh_set_dict(m)
        c.pattern_build(m["dim"], lib.BLOCK_DIAG)
        c.assemble(lib.FORM_MASS_VEC)
        c.matrix_store(SLOT_MD)
        c.pattern_build(m["dim"], lib.BLOCK_FULL)
        c.assemble(lib.FORM_LINELAS, [2.0, 0.5])
        c.matrix_store(SLOT_A)
        c.matrix_combine(SLOT_MD, 1.0, SLOT_A, 0.0)
        c.matrix_store(SLOT_MF)
        _state[which] = (c, m)
    return _state[which]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c, _ in _state.values():
        c.close()
    _state.clear()


@pytest.mark.parametrize("which", sorted(CASES))
def test_block_apply_equals_the_row_walk_bit_for_bit(fedd_lib, which):
    c, m = stored(fedd_lib, which)
    G, longest, n = CASES[which]
    rng = np.random.default_rng(11)
    for slot in (SLOT_A, SLOT_MF):
        M = c.matrix_get(slot)
        lens = np.diff(M.indptr)
        assert (M.shape[0], int(lens.max())) == (n, longest) and (8 if lens.max() <= 32 else 16) == G
        x = rng.standard_normal(n)
        y = c.matrix_apply(slot, x)
        ref = block_apply_rowwalk(M, x)
        assert np.array_equal(bits(y), bits(ref))
        assert np.array_equal(bits(c.matrix_apply(slot, x, alpha=-2.5)), bits(-2.5 * ref))      # alpha meets the finished sum


@pytest.mark.parametrize("which", sorted(CASES))
def test_mass_term_of_the_newton_residual_is_matrix_apply(fedd_lib, which):
    """b = 0, f = 0 (a material without stiffness), no source, no boundary condition: r = -(cm M u_k), the bits of
    fedd_matrix_apply(slot_m, cm, u_k) -- and of the host's row walk"""
    lib = fedd_lib
    c, m = stored(lib, which)
    own = own_dofs(m)
    n = own.shape[0]
    cm = 1.0 / ((0.01 * 0.01) * 0.25)
    u = smooth_displacement(m).ravel()[own]
    c.solution_set(u)
    c.rhs_set(np.zeros(n))
    c.newton_begin()
    c.assemble_hyperelastic(model_id(lib, hr.STVK), [0.0, 0.0], lib.HYPER_FORCE)
    assert not c.hyperelastic_force_get().any()
    nr = c.newton_residual(SLOT_MF, cm)
    r = c.rhs_get()
    c.newton_end()
    mm = c.matrix_apply(SLOT_MF, u, cm)
    assert np.array_equal(bits(r), bits(-mm))
    assert np.array_equal(bits(mm), bits(cm * block_apply_rowwalk(c.matrix_get(SLOT_MF), u)))
    assert abs(nr - np.linalg.norm(r)) <= n * 2.0 ** -52 * np.linalg.norm(r)


def masked(A, keep):
    """A with the values outside the columns `keep` set to 0.0 in place: every entry keeps its position in its row"""
    B = A.copy()
    B.data = np.where(keep[B.indices], B.data, 0.0)
    return B


def test_facsi_rows_bit_for_bit(fedd_lib):
    """y_l = (x_u[fdof] - sB) - sF with the two sums walked as k_facsi_rows<16> walks them: an entry's lane and trip follow from
    its position in the whole row of the coupled matrix, whichever sum it belongs to"""
    p = fsi_pair.Pair(fedd_lib)
    try:
        p.cpl.fsi_merge(p.fluid, p.struct, p.DT)
        _, fdof, sdof = p.host_matrix()
        p.facsi_children()
        p.cpl.fsi_prec_attach(p.fluid, p.struct)
        A = fsi_pair.scipy_matrix(fsi_pair.csr_tuple(p.cpl))
        assert np.diff(A.indptr).max() > 32 and (fdof >= 0).all()
        n, off_l = A.shape[0], p.n_f + p.n_s
        x = np.random.default_rng(31).standard_normal(n)
        y = p.cpl.schwarz_apply(x)
        y_d = p.struct.schwarz_apply(x[p.n_f:off_l])
        t = x[:p.n_f].copy()
        t[fdof] = x[off_l:] - (-(1.0 / p.DT)) * y_d[sdof]
        y_f = p.fluid.schwarz_apply(t)
        assert np.array_equal(bits(y[:p.n_f]), bits(y_f)) and np.array_equal(bits(y[p.n_f:off_l]), bits(y_d))
        col = np.arange(n)
        y_ext = np.concatenate([y_f, np.zeros(n - p.n_f)])
        sF = block_apply_rowwalk(masked(A, col < p.n_u), y_ext)[fdof]
        sB = block_apply_rowwalk(masked(A, (col >= p.n_u) & (col < p.n_f)), y_ext)[fdof]
        assert np.array_equal(bits(y[off_l:]), bits((x[fdof] - sB) - sF))
    finally:
        p.close()


def test_a_child_of_two_parents_of_both_kinds(fedd_lib):
    """the fluid context is the fluid child of a FaCSI preconditioner and the velocity child of another parent's block
    preconditioner: a detach lets go of that parent alone, a destroy of the child detaches both"""
    lib = fedd_lib
    p = fsi_pair.Pair(lib)
    par, schur = lib.Context(device=0), lib.Context(device=0)
    try:
        p.cpl.fsi_merge(p.fluid, p.struct, p.DT)
        p.facsi_children()
        p.cpl.fsi_prec_attach(p.fluid, p.struct)
        par.mesh_set_dict(p.mf)                     # a merged system of its own on the fluid's mesh
        par.pattern_build(p.DIM, lib.BLOCK_DIAG)
        par.assemble(lib.FORM_LAPLACE_VEC)
        par.matrix_store(0)
        par.assemble_div(p.n_p1, 1, 2)
        par.block_merge(0, 2, 1, -1)
        x = np.ones(p.n_f + p.n_s + p.n_l)
        y = p.cpl.schwarz_apply(x)
        for _ in range(2):
            par.block_prec_attach(lib.BLOCKPREC_DIAGONAL, p.fluid, schur)
            assert par.block_prec_info()["kind"] == lib.BLOCKPREC_DIAGONAL and p.cpl.fsi_prec_info()["attached"]
            par.block_prec_detach()                 # the other parent keeps the child
            assert par.block_prec_info()["kind"] == 0 and p.cpl.fsi_prec_info()["attached"]
            assert np.array_equal(p.cpl.schwarz_apply(x), y)
        par.block_prec_attach(lib.BLOCKPREC_DIAGONAL, p.fluid, schur)
        p.fluid.close()
        assert par.block_prec_info()["kind"] == 0 and not p.cpl.fsi_prec_info()["attached"]
        for parent, v in ((par, np.ones(p.n_f)), (p.cpl, x)):
            with pytest.raises(lib.FeddError, match="no preconditioner"):
                parent.schwarz_apply(v)
            with pytest.raises(lib.FeddError, match="preconditioner requested"):
                parent.gmres(v, max_it=5, use_prec=True)
    finally:
        schur.close()
        par.close()
        p.close()

"""The shared row walk of the gather kernels (csrc/gather_lists.hpp gather_walk; k_p2_gather, k_stress_gather, k_adv_gather,
k_hyper_gather) and the one list builder (gather_lists_ensure, k_p2_lists) in the shapes in which they can go wrong, as checked
preconditions of the mesh: the P2 cube of 3 x 3 x 3 cells (test_gpu_stress.py's p2_box333: 162 tetrahedra, 343 nodes), whose
interior vertices have more node-level nonzeros than a wave has lanes -- the second trip of the slot loop and the carry of the
running count in k_p2_lists -- and whose other nodes have fewer.  Every consumer is compared with the independent path the
suite already uses for it, at that test's tolerance, over every stored value: the last slot of the last node, the one place
where the walk takes the end of a list from the node's source count instead of the next start, is the last of them."""
import numpy as np
import pytest

import hyperelastic_ref as hr
import stress_ref as sr
from ale_ref import AleRestatement, on_pattern
from test_gpu_parity import assert_matrix_close
from test_gpu_stress import assert_close as assert_stress_close
from test_gpu_stress import coeff, mesh, system
from test_navier_stokes_abi import Restatement, smooth_velocity

pytestmark = pytest.mark.gpu
WHICH = "p2_box333"
CM = 1.0 / ((0.01 * 0.01) * 0.25)       # the Newmark coefficient of test_gpu_newton_newmark.py
STVK = hr.stvk_params(0.3571, 0.4)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def m(fedd_lib):
    return mesh(fedd_lib, WHICH)


def node_slots(ctx, dofs_rows, per_slot):
    """node-level nonzeros of every node from the stored CSR: the length of the node's first row over the entries per slot"""
    rowptr = ctx.csr_get()[0]
    return np.diff(rowptr)[::dofs_rows] // per_slot


def assert_shape(slots):
    assert slots.max() > 64, "no node takes a second trip of the slot loop: %d slots at most" % slots.max()
    assert slots.min() < 64
    assert slots[-1] > 0                # the last node has a last slot


def all_values(ctx):
    """the stored values, all of them: their number is the last row pointer"""
    rowptr, _, val, _ = ctx.csr_get()
    assert val.shape[0] == rowptr[-1] > 0
    return val.copy()


def test_p2_scalar_rows_equal_the_pair_kernels_bit_for_bit(fedd_lib, ctx, m):
    lib, dim = fedd_lib, m["dim"]
    ctx.mesh_set_dict(m)
    for form, dofs, mode in ((lib.FORM_LAPLACE, 1, lib.BLOCK_SCALAR), (lib.FORM_MASS, 1, lib.BLOCK_SCALAR),
                             (lib.FORM_LAPLACE_VEC, dim, lib.BLOCK_DIAG), (lib.FORM_MASS_VEC, dim, lib.BLOCK_DIAG)):
        ctx.pattern_build(dofs, mode)
        assert_shape(node_slots(ctx, dofs, 1))
        ctx.assemble(form)
        assert ctx.mesh_setup_info()["tiles_state"] == 1        # the lists were built and fit
        got = all_values(ctx)
        try:
            ctx.set_option("asm_p2_elem", 0)
            ctx.assemble(form)
            want = all_values(ctx)
        finally:
            ctx.set_option("asm_p2_elem", 1)
        assert got.shape == want.shape and np.abs(want).max() > 0.0
        assert np.array_equal(bits(got), bits(want)), (form, int(np.count_nonzero(bits(got) != bits(want))))


def test_stress_rows_match_the_restatement(fedd_lib, ctx, m):
    lib, dim = fedd_lib, m["dim"]
    ctx.mesh_set_dict(m)
    ctx.pattern_build(dim, lib.BLOCK_FULL)
    assert_shape(node_slots(ctx, dim, dim))
    for c_q in (None, coeff(m)):
        K = sr.assemble(m, c_q)
        ctx.assemble_stress(c_q)
        A = system(ctx, m)
        assert A.nnz == K.nnz       # with the pattern equality of assert_close: no stored value is left out of the comparison
        assert_stress_close(A, K)


def test_advection_rows_match_the_restatements(fedd_lib, ctx, m):
    lib = fedd_lib
    u = smooth_velocity(m["xyz"])
    w = 0.5 * smooth_velocity(m["xyz"][:, ::-1])
    ctx.mesh_set_dict(m)
    ctx.velocity_set(u)
    ctx.mesh_velocity_set(w)
    R = AleRestatement(lib, m)
    bn, bw = R.blocks_N(u.ravel()), R.blocks_W(u.ravel())
    cases = [(False, lib.ADV_N, R.assemble(bn)), (False, lib.ADV_W, R.assemble(bw)), (False, lib.ADV_NEWTON, R.assemble(bn + bw)),
             (True, lib.ALE_P, R.ale("P", u, w)), (True, lib.ALE_FIXEDPOINT, R.ale("FixedPoint", u, w)),
             (True, lib.ALE_NEWTON, R.ale("Newton", u, w))]
    # slot_add: slot 0 a DIAG matrix (the vector Laplacian), slot 3 a FULL one (N + W)
    ctx.pattern_build(m["dim"], lib.BLOCK_DIAG)
    ctx.assemble(lib.FORM_LAPLACE_VEC)
    ctx.matrix_store(0)
    ctx.assemble_advection(lib.ADV_NEWTON, 1.0, -1, 3)
    adds = {-1: None, 0: ctx.matrix_get(0), 3: ctx.matrix_get(3)}
    for ale, kind, ref in cases:
        for slot_add, M in adds.items():
            (ctx.assemble_advection_ale if ale else ctx.assemble_advection)(kind, 1.9, slot_add, 4)
            A = ctx.matrix_get(4)
            assert_shape(np.diff(A.indptr)[::m["dim"]] // m["dim"])
            want = ref.copy()
            want.data = 1.9 * ref.data
            want = want if M is None else on_pattern([want, M], ref.shape)
            assert A.nnz == want.nnz        # with the pattern equality below: no stored value is left out of the comparison
            assert_matrix_close(A, want)


@pytest.mark.parametrize("slot_m", [0, 2], ids=["diag_mass", "full_mass"])
def test_time_tangent_equals_store_and_combine_bit_for_bit(fedd_lib, ctx, m, slot_m):
    lib, dim = fedd_lib, m["dim"]
    ctx.mesh_set_dict(m)
    ctx.pattern_build(dim, lib.BLOCK_DIAG)
    ctx.assemble(lib.FORM_MASS_VEC)
    ctx.matrix_store(0)
    ctx.matrix_scale(0, 1.7)
    ctx.pattern_build(dim, lib.BLOCK_FULL)
    assert_shape(node_slots(ctx, dim, dim))
    ctx.assemble(lib.FORM_LINELAS, list(STVK))
    ctx.matrix_store(1)
    ctx.matrix_combine(0, 1.0, 1, 0.0)
    ctx.matrix_store(2)                 # the mass on the FULL pattern
    ctx.velocity_set(0.02 * smooth_velocity(m["xyz"]))
    ctx.assemble_hyperelastic(lib.HYPER_STVK, STVK, lib.HYPER_TANGENT)
    ctx.matrix_store(3)
    ctx.matrix_combine(slot_m, CM, 3, 1.0)
    want = all_values(ctx)
    ctx.assemble_hyperelastic(lib.HYPER_STVK, STVK, lib.HYPER_TANGENT)      # other values in between
    assert not np.array_equal(all_values(ctx), want)
    ctx.assemble_hyperelastic_time(lib.HYPER_STVK, STVK, slot_m, CM, what=lib.HYPER_TANGENT)
    got = all_values(ctx)
    assert got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), int(np.count_nonzero(bits(got) != bits(want)))


def test_lists_are_kept_by_a_move_and_dropped_by_a_new_mesh(fedd_lib, ctx, m):
    """a repeated call after fedd_mesh_move gives the bits of a fresh context on the moved mesh (the lists follow the
    connectivity, not the coordinates), and after a fedd_mesh_set of another mesh the bits of a fresh context on that one (one
    reset for the three sets of lists): the P2 scalar consumer and a FULL one"""
    lib, dim = fedd_lib, m["dim"]
    x = m["xyz"]
    d = 0.05 * np.prod(np.sin(np.pi * x), axis=1)[:, None] * np.cos(2.1 * x[:, ::-1] + 0.7)
    d[np.any((x == 0.0) | (x == 1.0), axis=1)] = 0.0
    assert np.abs(d).max() > 0.01
    other = mesh(lib, "p2_box322")

    def run(c):
        c.pattern_build(1, lib.BLOCK_SCALAR)
        c.assemble(lib.FORM_LAPLACE)
        a = all_values(c)
        c.pattern_build(dim, lib.BLOCK_FULL)
        c.assemble_stress()
        return a, all_values(c)

    def fresh(mm):
        c = lib.Context(device=0)
        try:
            c.mesh_set_dict(mm)
            return run(c)
        finally:
            c.close()

    moved = dict(m)
    moved["xyz"] = x + d
    ctx.mesh_set_dict(m)
    first = run(ctx)                    # the lists of both consumers exist
    ctx.mesh_move(d)
    for got, want, ref in zip(run(ctx), fresh(moved), first):
        assert np.array_equal(bits(got), bits(want))
        assert not np.array_equal(got, ref)
    ctx.mesh_set_dict(other)
    for got, want in zip(run(ctx), fresh(other)):
        assert np.array_equal(bits(got), bits(want))

"""Option "asm_kind": every dispatch of the matrix assembly that can be selected (assemble.hip launch_assemble: 0 = the default,
here with "asm_tiles" 0 so that it is the pair kernels; 2 = the pair sweep always; 3 = slot-addressed where it fits) gives the
oracle's matrix, and a value that names no dispatch is rejected and changes nothing."""
import os

import numpy as np
import pytest

import fedd_oracle as fo
from test_gpu_parity import assert_matrix_close, csr_global, oracle_mesh

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

LAM_MU = [1.5, 1.0]
KINDS = ((0, 0), (2, 1), (3, 1))        # (asm_kind, asm_tiles)
FORMS = ("laplace", "laplace_vec", "mass", "linelas", "div", "divt")


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def _mesh(fedd_lib, name):
    """(velocity / matrix mesh, pressure mesh): the smallest meshes of the suite with boundary rows, interior rows and, on the
    cylinder, irregular degree; the P2 mesh for the P2 instantiations of the kernels"""
    if name == "square":
        m = fedd_lib.structured_mesh(2, 1, 5)
        return m, m
    if name == "cube":
        m = fedd_lib.structured_mesh(3, 1, 4)
        return m, m
    m1 = fedd_lib.read_mesh(os.path.join(GOLD, "DFG3DCylinder_1k.mesh"), 3)
    return (m1, m1) if name == "cylinder" else (fedd_lib.p2_of_p1(m1, volume_id=0), m1)


# "cylinder_p2_rows": the P2 mesh with "asm_p2_elem" 0.  At its default the P2 scalar forms leave launch_assemble through
# k_elem_matrix + k_p2_gather under every kind; with 0 their rows come from the P2 instantiations of the pair / slot kernels.
MESHES = ["square", "cube", "cylinder", "cylinder_p2", "cylinder_p2_rows"]


def _oracle(mv, mp):
    om, omp = oracle_mesh(mv), oracle_mesh(mp)
    A_vec, BT, B = fo.stokes_blocks(om, omp, 1.0)       # (nu = 1: the vector Laplacian itself; B and B^T come scaled by -1)
    return {"laplace": fo.assembly_laplace(om), "laplace_vec": A_vec, "mass": fo.assembly_mass(om, "Scalar"),
            "linelas": fo.assembly_linelas(om, *LAM_MU), "div": -B, "divt": -BT}


def _assemble_all(fedd_lib, ctx, mv, mp):
    """every form of the list on the mesh set in ctx: {form: (matrix in global ids, its values as stored)}"""
    dim, ng = mv["dim"], mv["n_global"]
    out = {}
    for form, fid, dofs, mode, params in (("laplace", fedd_lib.FORM_LAPLACE, 1, fedd_lib.BLOCK_SCALAR, None),
                                          ("laplace_vec", fedd_lib.FORM_LAPLACE_VEC, dim, fedd_lib.BLOCK_DIAG, None),
                                          ("mass", fedd_lib.FORM_MASS, 1, fedd_lib.BLOCK_SCALAR, None),
                                          ("linelas", fedd_lib.FORM_LINELAS, dim, fedd_lib.BLOCK_FULL, LAM_MU)):
        ctx.pattern_build(dofs, mode)
        ctx.assemble(fid, params)
        out[form] = (csr_global(ctx, dofs * ng)[0], ctx.csr_get()[2].copy())
    ctx.assemble_div(mp["xyz"].shape[0], 1, 2)
    for form, slot in (("div", 1), ("divt", 2)):
        M = ctx.matrix_get(slot)
        out[form] = (M, M.data.copy())
    return out


@pytest.mark.parametrize("name", MESHES)
def test_every_kind_assembles_the_oracles_matrices(fedd_lib, ctx, name):
    """Laplace, vector Laplace (DIAG), mass, elasticity (FULL) and B / B^T under each kind: the oracle's matrix to the project's
    tolerance, bitwise reproducible over two runs, and -- the pair sweep and the slot-addressed kernel add the contributions of a
    slot in the same (adjacency, then local column) order -- the same bits under every kind."""
    mv, mp = _mesh(fedd_lib, name)
    ref = _oracle(mv, mp)
    ctx.mesh_set_dict(mv)
    vals = {}
    try:
        ctx.set_option("asm_p2_elem", 0 if name.endswith("_rows") else 1)
        for kind, tiles in KINDS:
            ctx.set_option("asm_kind", kind)
            ctx.set_option("asm_tiles", tiles)
            first = _assemble_all(fedd_lib, ctx, mv, mp)
            again = _assemble_all(fedd_lib, ctx, mv, mp)
            for form in FORMS:
                assert_matrix_close(first[form][0], ref[form])
                assert np.array_equal(first[form][1], again[form][1]), (name, kind, form)
                vals[(kind, form)] = first[form][1]
        for form in FORMS:
            for kind in (2, 3):
                assert np.array_equal(vals[(kind, form)], vals[(0, form)]), (name, kind, form)
    finally:
        ctx.set_option("asm_kind", 0)
        ctx.set_option("asm_tiles", 1)
        ctx.set_option("asm_p2_elem", 1)


def test_values_that_name_no_kind_are_rejected(fedd_lib, ctx):
    """asm_kind 1 (the lane-per-row kernel) and 4 (a second name for "asm_tiles") are gone, any other integer never named a
    dispatch; "asm_u" and "asm_dbg" are unknown keys.  A rejected value leaves the stored one alone: the assembly afterwards is
    the default path's, bit for bit."""
    m = fedd_lib.structured_mesh(3, 1, 4)
    ctx.mesh_set_dict(m)

    def default_matrices():
        out = []
        for fid, dofs, mode, params in ((fedd_lib.FORM_LAPLACE, 1, fedd_lib.BLOCK_SCALAR, None),
                                        (fedd_lib.FORM_MASS, 1, fedd_lib.BLOCK_SCALAR, None),
                                        (fedd_lib.FORM_LINELAS, 3, fedd_lib.BLOCK_FULL, LAM_MU)):
            ctx.pattern_build(dofs, mode)
            ctx.assemble(fid, params)
            out.append(ctx.csr_get()[2].copy())
        return out

    before = default_matrices()
    for v in (1, 4, 5, -1):
        with pytest.raises(fedd_lib.FeddError, match="asm_kind"):
            ctx.set_option("asm_kind", v)
    for key in ("asm_u", "asm_dbg"):
        for v in (0, 1, 2, 64):
            with pytest.raises(fedd_lib.FeddError, match="unknown key '%s'" % key):
                ctx.set_option(key, v)
    for key, bad in (("asm_tiles", (2, -1)), ("asm_tiles_host", (2, -1)), ("asm_p2_elem", (3, -1))):
        for v in bad:
            with pytest.raises(fedd_lib.FeddError, match=key):
                ctx.set_option(key, v)
    after = default_matrices()
    for b, a in zip(before, after):
        assert np.array_equal(b, a)
    assert ctx.mesh_setup_info()["tiles_state"] == 1        # (the default path of this mesh is the tile kernel)

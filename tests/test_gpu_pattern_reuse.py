"""fedd_pattern_build keeps the pattern arrays when it repeats the build they came from (option "pattern_reuse", default 1):
same mesh, dofs per node, block mode and "pat_hash", nothing wrote the pattern since.  It then only zeroes values and vectors.
Nothing in the arithmetic changes, so every comparison is bit for bit against a FRESH context with pattern_reuse = 0 and
spmv_reuse = 0, which builds everything every time.  40^3 cells is the smallest grid on which the SpMV dictionary and the row
classes, which sit behind the same steps, are built at all (68 921 rows; the classes need 65 536)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = 40
LAM, MU = 1.0 * 2 * 0.3 / (1 - 2 * 0.3), 1.0


def _scalar(c, capi):
    c.pattern_build(1, capi.BLOCK_SCALAR)
    c.assemble(capi.FORM_LAPLACE)
    c.assemble_rhs([1.0])
    c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])


def _vector(c, capi, mode):
    c.pattern_build(3, mode)
    if mode == capi.BLOCK_FULL:
        c.assemble(capi.FORM_LINELAS, [LAM, MU])
    else:
        c.assemble(capi.FORM_LAPLACE_VEC)
    c.assemble_rhs([0.0, 1.0, 0.0])
    c.dirichlet([2], [0.0, 0.0, 0.0])


def _observe(c, capi, max_it=300):
    """what a step is judged by: the assembled system and the preconditioned solve (at most max_it iterations: the iterates
    repeat bit for bit, converged or not)"""
    rowptr, col, val, _ = c.csr_get()
    out = dict(rowptr=rowptr, col=col, val=val, rhs=c.rhs_get())
    c.schwarz_set_target(0, 1.0)
    c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
    x, its, _ = c.gmres(None, rtol=1e-10, max_it=max_it, restart=100, use_prec=True)
    out.update(x=x, its=its)
    return out


def _assert_same(got, ref):
    for k in ("rowptr", "col", "val", "rhs", "x"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["its"] == ref["its"]


def _fresh(capi, mesh, problem, max_it=300, options=()):
    c = capi.Context(device=0)
    try:
        c.set_option("pattern_reuse", 0)
        c.set_option("spmv_reuse", 0)
        for k, v in options:
            c.set_option(k, v)
        c.mesh_set_dict(mesh)
        problem(c)
        out = _observe(c, capi, max_it)
        assert c.pattern_reuse_info() == {"last_reused": False, "n_reused": 0}
        assert c.spmv_reuse_info() == {"last_reused": False, "n_reused": 0}
        return out
    finally:
        c.close()


@pytest.fixture(scope="module")
def cube(fedd_lib):
    return fedd_lib.structured_mesh(3, 1, M)


@pytest.fixture(scope="module")
def ref_scalar(fedd_lib, cube):
    return _fresh(fedd_lib, cube, lambda c: _scalar(c, fedd_lib))


@pytest.fixture(scope="module")
def ref_vector(fedd_lib, cube):
    capi = fedd_lib
    return {mode: _fresh(capi, cube, lambda c: _vector(c, capi, mode), max_it=25) for mode in (capi.BLOCK_DIAG, capi.BLOCK_FULL)}


def test_three_bench_style_steps(fedd_lib, cube, ref_scalar):
    capi = fedd_lib
    c = capi.Context(device=0)
    try:
        c.mesh_set_dict(cube)
        for k in range(3):
            _scalar(c, capi)
            assert c.pattern_reuse_info() == {"last_reused": k > 0, "n_reused": k}
            _assert_same(_observe(c, capi), ref_scalar)
            assert c.schwarz_reuse_info() == {"last_reused": k > 0, "n_reused": k}
        # the A/B switch: the same context builds again, and computes the same
        c.set_option("pattern_reuse", 0)
        _scalar(c, capi)
        assert c.pattern_reuse_info() == {"last_reused": False, "n_reused": 2}
        _assert_same(_observe(c, capi), ref_scalar)
        assert c.schwarz_reuse_info() == {"last_reused": True, "n_reused": 3}      # (the pattern generation stands all the same)
    finally:
        c.close()


@pytest.mark.parametrize("what", ["dofs", "block_mode", "mesh_set", "assemble_div", "block_merge", "pat_hash"])
def test_pattern_is_built_again(fedd_lib, cube, ref_scalar, ref_vector, what):
    capi = fedd_lib
    n_nodes = cube["xyz"].shape[0]
    c = capi.Context(device=0)
    try:
        c.mesh_set_dict(cube)
        if what == "dofs":
            _scalar(c, capi)
            second, ref = (lambda: _vector(c, capi, capi.BLOCK_FULL)), ref_vector[capi.BLOCK_FULL]
        elif what == "block_mode":
            _vector(c, capi, capi.BLOCK_DIAG)
            second, ref = (lambda: _vector(c, capi, capi.BLOCK_FULL)), ref_vector[capi.BLOCK_FULL]
        elif what == "mesh_set":
            _scalar(c, capi)
            c.mesh_set_dict(cube)           # the same arrays: the mesh generation moves all the same
            second, ref = (lambda: _scalar(c, capi)), ref_scalar
        elif what in ("assemble_div", "block_merge"):
            # (P1 / P1 blocks on the cube: what matters here is who wrote the system slot)
            _vector(c, capi, capi.BLOCK_DIAG)
            c.matrix_store(0)
            c.assemble_div(n_nodes, 1, 2)   # leaves its scratch node pattern in the system slot
            if what == "block_merge":
                c.block_merge(0, 2, 1, -1)
            second, ref = (lambda: _vector(c, capi, capi.BLOCK_DIAG)), ref_vector[capi.BLOCK_DIAG]
        else:
            _scalar(c, capi)
            c.set_option("pat_hash", 0)     # the ordered-insertion kernel writes the same lists; it has to run to say so
            second, ref = (lambda: _scalar(c, capi)), ref_scalar
        before = c.pattern_reuse_info()["n_reused"]
        second()
        assert c.pattern_reuse_info() == {"last_reused": False, "n_reused": before}
        _assert_same(_observe(c, capi, max_it=300 if ref is ref_scalar else 25), ref)
        # ... and the build after that one repeats it
        second()
        assert c.pattern_reuse_info() == {"last_reused": True, "n_reused": before + 1}
        _assert_same(_observe(c, capi, max_it=300 if ref is ref_scalar else 25), ref)
    finally:
        c.close()


def test_p2_mesh_repeats(fedd_lib):
    """P2 tetrahedra take k_node_pattern (ordered insertion, lists longer than the hashed kernel holds)"""
    capi = fedd_lib
    mesh = capi.p2_of_p1(capi.structured_mesh(3, 1, 8), volume_id=0)
    ref = _fresh(capi, mesh, lambda c: _scalar(c, capi), max_it=25)
    c = capi.Context(device=0)
    try:
        c.mesh_set_dict(mesh)
        for k in range(2):
            _scalar(c, capi)
            assert c.pattern_reuse_info() == {"last_reused": k == 1, "n_reused": k}
            _assert_same(_observe(c, capi, max_it=25), ref)
    finally:
        c.close()


def test_full_node_blocks_repeat(fedd_lib, cube, ref_vector):
    capi = fedd_lib
    c = capi.Context(device=0)
    try:
        c.mesh_set_dict(cube)
        for k in range(2):
            _vector(c, capi, capi.BLOCK_FULL)
            assert c.pattern_reuse_info() == {"last_reused": k == 1, "n_reused": k}
            _assert_same(_observe(c, capi, max_it=25), ref_vector[capi.BLOCK_FULL])
    finally:
        c.close()

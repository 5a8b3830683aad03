"""Option "setup_fused" (default 1): the Schwarz setup's walk over the finished rows also makes the check of the kept SpMV
stream, and fedd_assemble_rhs keeps |det B| of the elements while the geometry stands.  Nothing in the arithmetic changes, so
every comparison is bit for bit between the same sequence of calls with the option at 0 and at 1, each on a context of its own.
Every sequence assembles at least twice: the first step builds the stream and the determinants, the later ones are the ones that
keep them.  fedd_setup_fused_info says what was kept, so a stale result that was used anyway shows even where the bits agree.

(The zero-fill of the values a repeated fedd_pattern_build makes is not skipped by this option; the sequence that switches from
the tile assembly to the accumulating kernels is pinned here all the same.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAM, MU = 1.5, 1.0


def _laplace(c, capi, extra_rows=()):
    c.pattern_build(1, capi.BLOCK_SCALAR)
    c.assemble(capi.FORM_LAPLACE)
    c.assemble_rhs([1.0])
    c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    if len(extra_rows):
        c.dirichlet_rows(extra_rows, np.zeros(len(extra_rows)))


def _elasticity(c, capi):
    c.pattern_build(3, capi.BLOCK_FULL)
    c.assemble(capi.FORM_LINELAS, [LAM, MU])
    c.assemble_rhs([0.0, 1.0, 0.0])
    c.dirichlet([2], [0.0, 0.0, 0.0])


def _setup(c, capi):
    c.schwarz_set_target(27, 1.0)
    c.schwarz_setup(1, capi.COMBINE_RESTRICTED)


def _outputs(c, solve=True, schwarz=True):
    """matrix, right-hand side, Schwarz sizes and classes (after a schwarz_setup), the solve, the stream and a product through it"""
    out = dict(val=c.csr_get()[2], rhs=c.rhs_get())
    if schwarz:
        out.update(schwarz=c.schwarz_info())
    n = c.csr_sizes()[0]
    x = np.random.default_rng(11).standard_normal(n)
    if solve:       # (the solve's first product is the one that keeps or builds the stream)
        sol, its, _ = c.gmres(None, rtol=1e-10, max_it=300, restart=100, use_prec=True)
        out.update(x=sol, its=its)
    c.spmv_device(1)
    out.update(y=c.spmv(x), spmv=c.spmv_info(), reuse=c.spmv_reuse_info())
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def _context(capi, mesh, fused):
    c = capi.Context(device=0)
    c.set_option("spmv_exact_public", 0)        # products through the solver's stream
    c.set_option("setup_fused", fused)
    c.mesh_set_dict(mesh)
    return c


def _both(capi, mesh, sequence):
    """the sequence with the option at 0 and at 1: ([outputs of every step] , fedd_setup_fused_info) each"""
    res = []
    for fused in (0, 1):
        c = _context(capi, mesh, fused)
        try:
            res.append((sequence(c), c.setup_fused_info()))
        finally:
            c.close()
    (out0, info0), (out1, info1) = res
    assert info0 == {"n_walks": 0, "n_checks_used": 0, "n_absdet_kept": 0}
    assert len(out0) == len(out1)
    for a, b in zip(out0, out1):
        _same(a, b)
    return out1, info1


def _steps(capi, problem, n=3):
    def sequence(c):
        outs = []
        for _ in range(n):
            problem(c, capi)
            _setup(c, capi)
            outs.append(_outputs(c))
        return outs
    return sequence


@pytest.mark.parametrize("cells", [13, (12, 13, 14), 40], ids=["13x13x13", "12x13x14", "40x40x40"])
def test_laplace_steps(fedd_lib, cells):
    """13^3 and 12 x 13 x 14 cells (a ragged last row block): streams without row classes, whose check writes the new values.
    40^3 cells is the smallest grid on which the classes are built: there the check compares the values and writes nothing"""
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, cells if isinstance(cells, int) else list(cells))
    outs, info = _both(capi, mesh, _steps(capi, _laplace))
    assert (outs[0]["spmv"]["row_classes"] > 0) == (cells == 40)
    # steps 2 and 3 found a stream to check and determinants to keep
    assert info == {"n_walks": 2, "n_checks_used": 2, "n_absdet_kept": 2}
    assert [o["reuse"]["n_reused"] for o in outs] == [0, 1, 2]
    _same(outs[0], {**outs[2], "reuse": outs[0]["reuse"]})


def test_elasticity_steps(fedd_lib):
    """three dofs per node, BLOCK_FULL: rows of up to 81 entries, longer than the walk holds in registers and than a column
    pattern takes"""
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, 9)
    outs, info = _both(capi, mesh, _steps(capi, _elasticity))
    assert info == {"n_walks": 2, "n_checks_used": 2, "n_absdet_kept": 2}
    assert [o["reuse"]["n_reused"] for o in outs] == [0, 1, 2]


def test_a_matrix_written_after_the_setup_makes_the_check_stale(fedd_lib):
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, 13)

    def sequence(c):
        outs = []
        _laplace(c, capi)
        _setup(c, capi)
        outs.append(_outputs(c))
        _laplace(c, capi)
        _setup(c, capi)             # (the walk checks the stream against these rows ...)
        c.matrix_scale(-1, 2.0)     # ... which are not the rows the next product sees
        outs.append(_outputs(c, solve=False, schwarz=False))
        _laplace(c, capi)
        _setup(c, capi)             # (walked again: the stream of the scaled matrix against the unscaled rows)
        c.matrix_scale(-1, 2.0)
        _setup(c, capi)             # (... and again, on the rows the product sees: this check is the one that is used)
        outs.append(_outputs(c))
        return outs

    outs, info = _both(capi, mesh, sequence)
    assert info["n_walks"] == 3 and info["n_checks_used"] == 1
    assert np.array_equal(outs[1]["y"], 2.0 * outs[0]["y"]) and np.array_equal(outs[1]["y"], outs[2]["y"])


def test_a_value_difference_alone_rebuilds_a_classed_stream(fedd_lib):
    """40^3 cells: the stream has row classes, so the walk compares the values and writes nothing.  The second matrix is the
    first one times two -- same graph, same kept entries, same columns: only the value comparison can tell that the stream is
    not this matrix' stream.  A walk that missed it would leave the product of the first matrix"""
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, 40)

    def sequence(c):
        outs = []
        for alpha in (None, 2.0, 2.0):
            _laplace(c, capi)
            if alpha:
                c.matrix_scale(-1, alpha)
            _setup(c, capi)
            outs.append(_outputs(c, solve=False))
        return outs

    outs, info = _both(capi, mesh, sequence)
    assert outs[0]["spmv"]["row_classes"] > 0
    assert info["n_walks"] == 2 and info["n_checks_used"] == 2
    assert [o["reuse"] for o in outs] == [{"last_reused": False, "n_reused": 0}, {"last_reused": False, "n_reused": 0},
                                          {"last_reused": True, "n_reused": 1}]
    assert np.array_equal(outs[1]["y"], 2.0 * outs[0]["y"]) and np.array_equal(outs[2]["y"], outs[1]["y"])


def test_a_moved_mesh_and_another_mesh_get_their_own_determinants(fedd_lib):
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, 13)
    other = capi.structured_mesh(3, 1, [12, 13, 14])
    xyz = np.asarray(mesh["xyz"], dtype=np.float64)
    disp = 0.02 * np.sin(np.pi * xyz[:, [1, 2, 0]]) * np.sin(np.pi * xyz)      # zero on the boundary, smooth, no inverted element

    def sequence(c):
        outs = []

        def rhs():
            c.pattern_build(1, capi.BLOCK_SCALAR)
            c.assemble_rhs([1.0])
            outs.append(dict(rhs=c.rhs_get()))

        rhs()
        rhs()                       # kept
        c.mesh_move(disp)
        rhs()                       # computed on the moved coordinates
        rhs()                       # kept
        c.mesh_move(None)
        rhs()                       # computed: the coordinates of the first call again, but another geometry_id
        c.mesh_set_dict(other)
        rhs()                       # computed on the other mesh
        rhs()                       # kept
        return outs

    outs, info = _both(capi, mesh, sequence)
    assert info["n_absdet_kept"] == 3
    assert np.array_equal(outs[0]["rhs"], outs[1]["rhs"]) and np.array_equal(outs[0]["rhs"], outs[4]["rhs"])
    assert not np.array_equal(outs[0]["rhs"], outs[2]["rhs"]) and np.array_equal(outs[2]["rhs"], outs[3]["rhs"])
    assert outs[5]["rhs"].shape != outs[0]["rhs"].shape


def test_an_accumulating_assembly_after_an_overwriting_one(fedd_lib):
    """the tile assembly stores into the values, the kernels of asm_tiles 0 add into zeroed ones.  The option does not skip the
    zero-fill of a repeated fedd_pattern_build, so this passes without it too: it stands guard for a change that does"""
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, 13)

    def sequence(c):
        outs = []
        for tiles in (1, 0, 1, 0):
            c.set_option("asm_tiles", tiles)
            _laplace(c, capi)
            _setup(c, capi)
            outs.append(_outputs(c, solve=False))
        return outs

    _both(capi, mesh, sequence)


def test_a_changed_row_rebuilds_the_stream(fedd_lib):
    """one more unit row in the second step: the walk's check reports the mismatch and the stream is built, as without the option"""
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, 13)
    flags = np.asarray(mesh["flag_uni"])
    row = int(np.flatnonzero(flags == 0)[len(flags) // 4])      # an interior node

    def sequence(c):
        outs = []
        for extra in ((), (row,), (row,)):
            _laplace(c, capi, extra_rows=np.array(extra, dtype=np.int32))
            _setup(c, capi)
            outs.append(_outputs(c))
        return outs

    outs, info = _both(capi, mesh, sequence)
    assert info["n_walks"] == 2 and info["n_checks_used"] == 2
    assert [o["reuse"] for o in outs] == [{"last_reused": False, "n_reused": 0}, {"last_reused": False, "n_reused": 0},
                                          {"last_reused": True, "n_reused": 1}]
    assert not np.array_equal(outs[0]["y"], outs[1]["y"]) and np.array_equal(outs[1]["y"], outs[2]["y"])

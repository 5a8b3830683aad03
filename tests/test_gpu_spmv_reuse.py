"""The solver's SpMV stream is kept from one matrix to the next while pattern, sizes and SpMV options stand (option "spmv_reuse",
default 1): one pass over the assembled rows verifies it (row classes in use: values too, nothing written) or writes the new
values to their places (no classes).  Every comparison is bit for bit against a FRESH context with pattern_reuse = 0 and
spmv_reuse = 0.  40^3 cells is the smallest grid on which the dictionary and the row classes are built at all."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = 40          # 68 921 rows: the classes need 65 536
ME = 24         # elasticity: 46 875 rows, dictionary forced by "spmv_pattern" 2
LAM = 1.0 * 2 * 0.3 / (1 - 2 * 0.3)


def _laplace(c, capi, flags=(1, 2, 3)):
    c.pattern_build(1, capi.BLOCK_SCALAR)
    c.assemble(capi.FORM_LAPLACE)
    c.assemble_rhs([1.0])
    c.dirichlet(list(flags), [0.0] * len(flags))


def _elasticity(c, capi, mu):
    c.pattern_build(3, capi.BLOCK_FULL)
    c.assemble(capi.FORM_LINELAS, [LAM, mu])
    c.assemble_rhs([0.0, 1.0, 0.0])
    c.dirichlet([2], [0.0, 0.0, 0.0])


def _product(c):
    """y = A x through the solver's stream (spmv_exact_public = 0), x seeded; the first product after a matrix changed is what
    builds, verifies or refreshes the stream"""
    n = c.csr_sizes()[0]
    x = np.random.default_rng(11).standard_normal(n)
    c.spmv_device(1)
    return dict(y=c.spmv(x), info=c.spmv_info())


def _solve(c, capi):
    c.schwarz_set_target(27, 1.0)
    c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
    x, its, _ = c.gmres(None, rtol=1e-10, max_it=300, restart=100, use_prec=True)
    return dict(x=x, its=its)


def _context(capi, mesh, options=(), fresh=False):
    c = capi.Context(device=0)
    c.set_option("spmv_exact_public", 0)
    if fresh:
        c.set_option("pattern_reuse", 0)
        c.set_option("spmv_reuse", 0)
    for k, v in options:
        c.set_option(k, v)
    c.mesh_set_dict(mesh)
    return c


def _fresh(capi, mesh, problem, options=(), solve=False):
    c = _context(capi, mesh, options, fresh=True)
    try:
        problem(c)
        out = _product(c)
        if solve:
            out.update(_solve(c, capi))
        assert c.spmv_reuse_info() == {"last_reused": False, "n_reused": 0}
        return out
    finally:
        c.close()


def _assert_same(got, ref):
    assert got["info"] == ref["info"]           # field by field: stream length, patterns, classes, column bytes
    assert np.array_equal(got["y"], ref["y"])
    if "x" in ref:
        assert got["its"] == ref["its"]
        assert np.array_equal(got["x"], ref["x"])


def _jittered(mesh, h):
    """the interior nodes of the corner block of 24 x 24 x 25 nodes moved by up to 0.2 h (seeded): their rows and their neighbours'
    rows (25 x 25 x 26 = 16 250) repeat nobody's values.  A row that repeats nobody is a class of its own and the table holds
    16 384 classes, filled in hash order: with the classes of the lattice part (about a thousand) some 5 % of all classes,
    hence of the rows, find no place, and the others keep the classes in use.  (A smaller block leaves every row in a class; from
    18 200 classes on, 10 % of the rows would be outside and the classes off.)"""
    m = dict(mesh)
    xyz = np.array(mesh["xyz"], dtype=np.float64, copy=True)
    pick = (np.asarray(mesh["flag_rep"]) == 0) & np.all(xyz < np.array([24.5, 24.5, 25.5]) * h, axis=1)
    xyz[pick] += np.random.default_rng(17).uniform(-0.2 * h, 0.2 * h, size=xyz[pick].shape)
    m["xyz"] = xyz
    return m


@pytest.fixture(scope="module", params=["lattice", "jittered"])
def grid(request, fedd_lib):
    """the mesh and the fresh context's results for the two Laplace problems the tests below reassemble"""
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, M)
    if request.param == "jittered":
        mesh = _jittered(mesh, 1.0 / M)
    ref = _fresh(capi, mesh, lambda c: _laplace(c, capi), solve=True)
    ref1 = _fresh(capi, mesh, lambda c: _laplace(c, capi, flags=(1,)))
    n = mesh["xyz"].shape[0]
    info = ref["info"]
    print("%s: %d rows, %d classes, %d rows in classes, %d patterns" % (request.param, n, info["row_classes"], info["rows_in_classes"],
                                                                    info["column_patterns"]))
    # preconditions: the classes are in use (they cover at least 90 % of the rows), and the jitter left rows outside them
    assert info["row_classes"] > 0 and info["rows_in_classes"] * 100 >= 90 * n
    if request.param == "jittered":
        assert info["rows_in_classes"] < n
    return dict(mesh=mesh, ref=ref, ref1=ref1)


def test_same_operator_reassembled(fedd_lib, grid):
    capi = fedd_lib
    c = _context(capi, grid["mesh"])
    try:
        for k in range(3):
            _laplace(c, capi)
            got = _product(c)
            assert c.spmv_reuse_info() == {"last_reused": k > 0, "n_reused": k}
            if k == 2:
                got.update(_solve(c, capi))
                _assert_same(got, grid["ref"])
            else:
                _assert_same(got, {k_: grid["ref"][k_] for k_ in ("y", "info")})
        # the A/B switch
        c.set_option("spmv_reuse", 0)
        _laplace(c, capi)
        _assert_same(_product(c), {k_: grid["ref"][k_] for k_ in ("y", "info")})
        assert c.spmv_reuse_info() == {"last_reused": False, "n_reused": 2}
    finally:
        c.close()


def test_other_dirichlet_rows_fall_back(fedd_lib, grid):
    capi = fedd_lib
    c = _context(capi, grid["mesh"])
    try:
        _laplace(c, capi)
        _product(c)
        _laplace(c, capi, flags=(1,))       # fewer unit rows: those rows differ, the stream is built
        got = _product(c)
        assert c.spmv_reuse_info() == {"last_reused": False, "n_reused": 0}
        _assert_same(got, grid["ref1"])
        _laplace(c, capi, flags=(1,))       # ... and the build is what the next matrix is checked against
        got = _product(c)
        assert c.spmv_reuse_info() == {"last_reused": True, "n_reused": 1}
        _assert_same(got, grid["ref1"])
    finally:
        c.close()


OPTIONS = [("spmv_drop_tol", 0.0), ("spmv_compact", 1), ("spmv_classes", 0), ("spmv_classes_cover", 95), ("spmv_col16", 0),
           ("spmv_pattern", 2), ("spmv_pat_nu", 4), ("spmv_win_nu", 6)]     # every setter that invalidates the stream


@pytest.mark.parametrize("key,value", OPTIONS)
def test_an_option_set_between_two_steps_drops_the_keep(fedd_lib, key, value):
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, M)
    ref = _fresh(capi, mesh, lambda c: _laplace(c, capi), options=[(key, value)])
    c = _context(capi, mesh)
    try:
        _laplace(c, capi)
        _product(c)
        c.set_option(key, value)
        _laplace(c, capi)
        got = _product(c)
        assert c.spmv_reuse_info() == {"last_reused": False, "n_reused": 0}
        _assert_same(got, ref)
    finally:
        c.close()


@pytest.mark.parametrize("options", [[("spmv_pattern", 2), ("spmv_classes", 0)],
                                     [("spmv_pattern", 0), ("spmv_classes", 0), ("spmv_col16", 1)],
                                     [("spmv_pattern", 0), ("spmv_classes", 0), ("spmv_col16", 0)]],
                         ids=["dictionary", "col16", "col32"])
def test_new_values_on_the_same_graph_are_refreshed(fedd_lib, options):
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, ME)
    ref = _fresh(capi, mesh, lambda c: _elasticity(c, capi, 0.7), options=options)
    c = _context(capi, mesh, options)
    try:
        _elasticity(c, capi, 0.83)
        first = _product(c)
        _elasticity(c, capi, 0.7)
        got = _product(c)
        assert c.spmv_reuse_info() == {"last_reused": True, "n_reused": 1}
        _assert_same(got, ref)
        assert not np.array_equal(got["y"], first["y"])
    finally:
        c.close()

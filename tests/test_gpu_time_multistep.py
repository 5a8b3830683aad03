"""BDF history on the device (fedd_multistep_*, timestep.hip k_multistep) against the numpy restatement of the operation order
in include/fedd_hip.h, BIT FOR BIT: u_0, u_1 and the right-hand side after every advance.

The right-hand side is M t on the rows of M and 0.0 below.  M t is restated by walking the rows as k_block_apply does: G lanes
per row (8 while the longest row has at most 32 entries, else 16), lane g adds the separately rounded products of entries
g, g + G, ... in that order starting from 0.0, and the lane sums meet in the xor tree o = G/2, ..., 1 -- so the comparison
needs no tolerance.  (The padding products 0.0 * 0.0 the kernel adds leave every partial sum as it is.)

Shapes, (n, n_m) = (rows of the system, rows of the mass block), all four parities of the row-pair accesses:
    (108, 81)  structured_mesh(3, 1, 2), merged P1 / P1:  n even, n_m odd  -- the zero fill starts on the upper row of a pair
    ( 81, 81)  ... its velocity block alone:              n odd,  n_m odd  -- scalar tail row, nothing to zero
    ( 27, 18)  structured_mesh(2, 1, 2), merged P1 / P1:  n odd,  n_m even -- the tail row is a zeroed pressure row
    ( 18, 18)  ... its velocity block alone:              n even, n_m even
One workgroup covers each of them.  test_grid_stride_bit_for_bit adds the merged P1 / P1 system of structured_mesh(3, 1, 64),
(n, n_m) = (1098500, 823875): n / 2 row pairs are more than 2048 * 256 lanes, so the launch is capped at 2048 workgroups and every
lane of the low pairs walks the grid-stride loop a second time; n_m odd again, many workgroups in the zero fill."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOT_A, SLOT_B, SLOT_BT, SLOT_F, SLOT_M = 0, 1, 2, 4, 5
DT = 0.01
BDF1 = [1.0 / DT]
BDF2 = [2.0 / DT, -0.5 / DT]
SHAPES = {("3d", True): (108, 81), ("3d", False): (81, 81), ("2d", True): (27, 18), ("2d", False): (18, 18)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def block_apply_rowwalk(M, x):
    """y = M x in the summation order of k_block_apply (timestep.hip), alpha = 1.0"""
    M = M.tocsr()
    M.sort_indices()
    lens = np.diff(M.indptr)
    G = 8 if lens.max() <= 32 else 16
    trips = -(-int(lens.max()) // G)
    rows = np.repeat(np.arange(M.shape[0]), lens)
    pos = np.arange(M.nnz) - np.repeat(M.indptr[:-1], lens)     # entry k of its row: lane k % G, trip k // G
    prod = np.zeros((M.shape[0], trips * G))
    prod[rows, pos] = M.data * x[M.indices]
    prod = prod.reshape(M.shape[0], trips, G)
    acc = np.zeros((M.shape[0], G))
    for t in range(trips):
        acc = acc + prod[:, t, :]
    o = G // 2
    while o >= 1:
        acc = acc + acc[:, np.arange(G) ^ o]
        o //= 2
    return acc[:, 0].copy()


class History:
    """the header's definition, every product and every sum its own numpy operation"""

    def __init__(self, order, n):
        self.order, self.count = order, 0
        self.u = [np.zeros(n) for _ in range(order)]

    def advance(self, M, u, coeff):
        n_use = len(coeff)
        assert 1 <= n_use <= min(self.count + 1, self.order)
        old0 = self.u[0].copy() if self.count >= 1 else None
        if self.order == 2 and self.count >= 1:
            self.u[1] = old0
        self.u[0] = u.copy()
        t = coeff[0] * u if n_use == 1 else (coeff[0] * u) + (coeff[1] * old0)
        self.count = min(self.count + 1, self.order)
        rhs = np.zeros(u.shape[0])
        rhs[:M.shape[0]] = block_apply_rowwalk(M, t)
        return rhs


def setup(fedd_lib, c, which, merged):
    """slot 5 <- vector mass * density, slot 0 <- vector Laplacian; merged: the P1 / P1 system [A B^T; B 0], else the velocity block"""
    L = fedd_lib
    m = L.structured_mesh(3, 1, 2) if which == "3d" else L.structured_mesh(2, 1, 2)
    dim, nn = m["dim"], m["xyz"].shape[0]
    c.mesh_set_dict(m)
    c.pattern_build(dim, L.BLOCK_DIAG)
    c.assemble(L.FORM_MASS_VEC)
    c.matrix_scale(-1, 1.7)
    c.matrix_store(SLOT_M)
    c.assemble(L.FORM_LAPLACE_VEC)
    c.matrix_store(SLOT_A)
    if merged:
        c.assemble_div(nn, SLOT_B, SLOT_BT)
        c.block_merge(SLOT_A, SLOT_BT, SLOT_B, -1)
    else:
        c.matrix_combine(SLOT_M, 1.0, SLOT_A, 1.0)
    n, n_m = c.csr_sizes()[0], dim * nn
    assert (n, n_m) == SHAPES[(which, merged)]
    return m, n, n_m


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("which,merged", [("3d", True), ("3d", False), ("2d", True), ("2d", False)])
def test_four_advances_bit_for_bit(fedd_lib, ctx, which, merged, order):
    m, n, n_m = setup(fedd_lib, ctx, which, merged)
    M = ctx.matrix_get(SLOT_M)
    assert M.shape == (n_m, n_m)
    rng = np.random.default_rng(17)
    H = History(order, n)
    ctx.multistep_begin(order)
    assert ctx.multistep_info() == (order, 0)
    for step in range(4):
        u = rng.standard_normal(n)
        coeff = BDF2 if (order == 2 and step >= 1) else BDF1
        ctx.rhs_set(rng.standard_normal(n))             # whatever the right-hand side held is gone afterwards
        ctx.solution_set(u)
        ctx.multistep_advance(SLOT_M, coeff)
        expect = H.advance(M, u, coeff)
        assert ctx.multistep_info() == (order, H.count)
        got = ctx.rhs_get()
        diff = [int(np.count_nonzero(bits(ctx.multistep_get(k)) != bits(H.u[k]))) for k in range(order)]
        print(which, "merged" if merged else "velocity", "order", order, "step", step, "(n, n_m)", (n, n_m), "differing entries: history",
              diff, "rhs", int(np.count_nonzero(bits(got) != bits(expect))))
        assert not any(diff)
        assert np.array_equal(bits(got), bits(expect))
        assert not got[n_m:].any() and (n_m == n or got[:n_m].any())
        assert np.array_equal(bits(ctx.solution_get()), bits(u))        # the solution is read, not written
    # an order-2 history may still be advanced with one coefficient (the shift happens all the same)
    if order == 2:
        u = rng.standard_normal(n)
        ctx.solution_set(u)
        ctx.multistep_advance(SLOT_M, BDF1)
        expect = H.advance(M, u, BDF1)
        assert np.array_equal(bits(ctx.rhs_get()), bits(expect))
        assert all(np.array_equal(bits(ctx.multistep_get(k)), bits(H.u[k])) for k in range(2))


def test_grid_stride_bit_for_bit(fedd_lib, ctx):
    """more row pairs than 2048 workgroups of 256 lanes: the capped launch and the grid-stride loop, first step and full step"""
    L = fedd_lib
    m = L.structured_mesh(3, 1, 64)
    nn = m["xyz"].shape[0]
    ctx.mesh_set_dict(m)
    ctx.pattern_build(3, L.BLOCK_DIAG)
    ctx.assemble(L.FORM_MASS_VEC)
    ctx.matrix_store(SLOT_M)
    ctx.assemble(L.FORM_LAPLACE_VEC)
    ctx.matrix_store(SLOT_A)
    ctx.assemble_div(nn, SLOT_B, SLOT_BT)
    ctx.block_merge(SLOT_A, SLOT_BT, SLOT_B, -1)
    n, n_m = ctx.csr_sizes()[0], 3 * nn
    assert (n, n_m) == (1098500, 823875) and n // 2 > 2048 * 256
    M = ctx.matrix_get(SLOT_M)
    rng = np.random.default_rng(31)
    H = History(2, n)
    ctx.multistep_begin(2)
    for step, coeff in enumerate((BDF1, BDF2, BDF2)):
        u = rng.standard_normal(n)
        ctx.rhs_set(np.ones(n))
        ctx.solution_set(u)
        ctx.multistep_advance(SLOT_M, coeff)
        expect = H.advance(M, u, coeff)
        got = ctx.rhs_get()
        diff = [int(np.count_nonzero(bits(ctx.multistep_get(k)) != bits(H.u[k]))) for k in range(2)]
        print("step", step, "(n, n_m)", (n, n_m), "differing entries: history", diff, "rhs", int(np.count_nonzero(bits(got) != bits(expect))))
        assert not any(diff)
        assert np.array_equal(bits(got), bits(expect))


def run(fedd_lib, c, between=None):
    """three BDF2 advances on the merged 3D system; `between` runs after the first"""
    m, n, n_m = setup(fedd_lib, c, "3d", True)
    rng = np.random.default_rng(23)
    c.multistep_begin(2)
    out = []
    for step in range(3):
        c.solution_set(rng.standard_normal(n))
        c.multistep_advance(SLOT_M, BDF2 if step else BDF1)
        out.append((c.rhs_get(), c.multistep_get(0), c.multistep_get(1)))
        if step == 0 and between:
            between(m, n)
    return out


def test_history_survives_merge_advection_and_dirichlet_and_runs_repeat(fedd_lib, ctx):
    plain = run(fedd_lib, ctx)
    again = run(fedd_lib, ctx)

    def between(m, n):
        ctx.velocity_set(np.ones((m["xyz"].shape[0], 3)))
        ctx.assemble_advection(fedd_lib.ADV_NEWTON, 1.0, SLOT_A, SLOT_F)
        ctx.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)
        ctx.dirichlet_rows(np.arange(0, 9, dtype=np.int32), np.ones(9))
        ctx.matrix_combine(SLOT_M, 3.0, SLOT_A, 1.0)                    # a system of another length ...
        with pytest.raises(fedd_lib.FeddError, match="rows, the history was begun on"):
            ctx.solution_set(np.zeros(81))
            ctx.multistep_advance(SLOT_M, BDF1)
        ctx.block_merge(SLOT_F, SLOT_BT, SLOT_B, -1)                    # ... and back
        assert ctx.multistep_info() == (2, 1)

    disturbed = run(fedd_lib, ctx, between)
    for a, b, d in zip(plain, again, disturbed):
        for k in range(3):
            assert np.array_equal(bits(a[k]), bits(b[k]))               # two identical runs agree bit for bit
            assert np.array_equal(bits(a[k]), bits(d[k]))               # ... and so does the one with the calls in between


def test_mesh_set_drops_the_history(fedd_lib, ctx):
    m, n, n_m = setup(fedd_lib, ctx, "3d", True)
    with pytest.raises(fedd_lib.FeddError, match="fedd_multistep_begin"):      # advance before begin
        ctx.multistep_advance(SLOT_M, BDF1)
    ctx.multistep_begin(2)
    ctx.solution_set(np.ones(n))
    ctx.multistep_advance(SLOT_M, BDF1)
    ctx.mesh_set_dict(m)
    assert ctx.multistep_info() == (0, 0)
    with pytest.raises(fedd_lib.FeddError, match="fedd_multistep_begin"):
        ctx.multistep_advance(SLOT_M, BDF1)
    # slots of the earlier mesh are refused once there is a history again
    setup(fedd_lib, ctx, "3d", True)
    ctx.multistep_begin(1)
    ctx.mesh_set_dict(m)
    ctx.pattern_build(3, fedd_lib.BLOCK_DIAG)
    ctx.assemble(fedd_lib.FORM_MASS_VEC)
    ctx.multistep_begin(1)
    with pytest.raises(fedd_lib.FeddError, match="earlier mesh"):
        ctx.multistep_advance(SLOT_M, BDF1)


def test_set_get_and_argument_errors(fedd_lib, ctx):
    m, n, n_m = setup(fedd_lib, ctx, "2d", True)
    M = ctx.matrix_get(SLOT_M)
    rng = np.random.default_rng(29)
    ctx.multistep_begin(2)
    assert not ctx.multistep_get(0).any() and not ctx.multistep_get(1).any()   # begin zeroes, it does not read the solution
    with pytest.raises(fedd_lib.FeddError, match=r"n_use 2 exceeds min\(count \+ 1, order\) = 1"):
        ctx.multistep_advance(SLOT_M, BDF2)                                     # nothing recorded yet
    with pytest.raises(fedd_lib.FeddError, match="n_use 3 exceeds"):
        ctx.multistep_advance(SLOT_M, [1.0, 2.0, 3.0])
    with pytest.raises(fedd_lib.FeddError, match="slot 3 is empty"):
        ctx.multistep_advance(3, BDF1)
    with pytest.raises(fedd_lib.FeddError, match="k must be 0 .. order - 1"):
        ctx.multistep_set(2, np.zeros(n))
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    ctx.multistep_set(0, a)
    assert ctx.multistep_info() == (2, 1)
    ctx.multistep_set(1, b)
    assert ctx.multistep_info() == (2, 2)
    assert np.array_equal(bits(ctx.multistep_get(0)), bits(a)) and np.array_equal(bits(ctx.multistep_get(1)), bits(b))
    # a state that was set is a state after some step: the full step is allowed at once
    u = rng.standard_normal(n)
    ctx.solution_set(u)
    ctx.multistep_advance(SLOT_M, BDF2)
    t = (BDF2[0] * u) + (BDF2[1] * a)
    assert np.array_equal(bits(ctx.rhs_get()[:n_m]), bits(block_apply_rowwalk(M, t)))
    assert np.array_equal(bits(ctx.multistep_get(0)), bits(u)) and np.array_equal(bits(ctx.multistep_get(1)), bits(a))
    # a slot with more rows than the system: the merged system stored whole, against the velocity block as the system
    ctx.matrix_store(3)
    ctx.matrix_combine(SLOT_M, 1.0, SLOT_A, 1.0)
    ctx.multistep_begin(1)
    with pytest.raises(fedd_lib.FeddError, match="more rows or columns than the system"):
        ctx.multistep_advance(3, BDF1)
    ctx.multistep_begin(2)                                                      # begin again starts over
    assert ctx.multistep_info() == (2, 0)

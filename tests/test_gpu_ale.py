"""ALE convection on the GPU (fedd_mesh_velocity_set / _diff / _get, fedd_assemble_advection_ale) at the ABI through capi,
against the numpy restatement of tests/ale_ref.py evaluated on x_ref + d.  The meshes are the smallest on which the kernel can
still go wrong: element counts that are no multiple of the four waves of a workgroup, a distorted geometry (B^-1 is no multiple
of the identity), and one mesh with more elements than one grid trip covers (10 368 > 4 * 2048)."""
import numpy as np
import pytest

from ale_ref import AleRestatement, on_pattern
from test_gpu_distorted import check_mesh, distorted
from test_gpu_parity import assert_matrix_close
from test_navier_stokes_abi import EDGES, degrees, smooth_velocity

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
MESHES = ["square_p1", "cube_p1", "square_p2", "cube_p2"]
_meshes = {}


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def _mesh(lib, which):
    if which not in _meshes:
        if which == "square_p1":
            m = lib.structured_mesh(2, 1, 3)            # 18 elements
        elif which == "cube_p1":
            m = lib.structured_mesh(3, 1, 3)            # 162 elements
        elif which == "cube_p1_trips":
            m = lib.structured_mesh(3, 1, 12)           # 10 368 elements: the element kernel takes a second trip
        else:
            dim = 2 if which == "square_p2" else 3
            m = distorted(lib.structured_mesh(dim, 1, 3), 0.15, "all", seed=4 + dim)
            check_mesh(m)
            m = lib.p2_of_p1(m, volume_id=0)
        _meshes[which] = m
    return _meshes[which]


def displacement(m, amp=0.04, phase=0.0):
    """smooth, no polynomial, every component depends on every coordinate; small against the cell width 1/3 (1/12)"""
    x, dim = m["xyz"], m["dim"]
    s = x.sum(axis=1)
    return amp * np.stack([np.sin(2.3 * x[:, k] + 0.9 * s + 0.4 * k + phase) * np.cos(1.1 * x[:, (k + 1) % dim] - 0.3)
                           for k in range(dim)], axis=1)


def mesh_velocity(x):
    """smooth, of the size of the velocity, with a divergence that varies over the mesh"""
    s = x.sum(axis=1)
    cols = [0.8 * np.cos(1.7 * x[:, 0] - 0.5 * s) + 0.3 * x[:, 0] ** 2, np.sin(1.2 * x[:, 1] + 0.6 * s) * np.exp(-0.4 * x[:, 1]) - 0.2]
    if x.shape[1] == 3:
        cols.append(0.7 * np.sin(0.9 * x[:, 2] + 1.3 * x[:, 0]) + 0.4 * x[:, 2])
    return np.stack(cols, axis=1)


def moved(m, d):
    out = dict(m)
    out["xyz"] = m["xyz"] + d       # the single addition of Mesh::moveMesh
    return out


def affine_positions(m):
    """where the element maps put the nodes: the map is affine from the first dim + 1 nodes (FE::buildTransformation), so a
    P2 mid-side node sits at the midpoint of its edge, wherever a smooth displacement has carried its coordinates"""
    x, dim, conn = m["xyz"].copy(), m["dim"], m["conn"]
    if conn.shape[1] > dim + 1:
        for k, (a, b) in enumerate(EDGES[dim]):
            x[conn[:, dim + 1 + k]] = 0.5 * (m["xyz"][conn[:, a]] + m["xyz"][conn[:, b]])
    return x


def _kinds(lib):
    return ((lib.ALE_P, "P"), (lib.ALE_FIXEDPOINT, "FixedPoint"), (lib.ALE_NEWTON, "Newton"))


def _setup(lib, ctx, which, amp=0.04):
    m = _mesh(lib, which)
    d = displacement(m, amp)
    ctx.mesh_set_dict(m)
    ctx.mesh_move(d)
    assert ctx.mesh_move_info()["min_det_ratio"] > 0.5
    mm = moved(m, d)
    u, w = smooth_velocity(mm["xyz"]), mesh_velocity(mm["xyz"])
    ctx.velocity_set(u)
    ctx.mesh_velocity_set(w)
    return m, mm, d, u, w


@pytest.mark.parametrize("which", MESHES)
def test_ale_matrices_match_the_restatement_on_the_moved_mesh(fedd_lib, ctx, which):
    """P, N(u - w) - P and N(u - w) + W(u) - P after a mesh_move: same FULL pattern, structural zeros included, and the value
    criterion of the advection matrices; scale and slot_add with a DIAG and with a FULL matrix"""
    lib = fedd_lib
    m, mm, d, u, w = _setup(lib, ctx, which)
    dim = m["dim"]
    R = AleRestatement(lib, mm)
    ref = {}
    for kind, name in _kinds(lib):
        ref[kind] = R.ale(name, u, w)
        ctx.assemble_advection_ale(kind, 1.0, -1, 4)
        err = assert_matrix_close(ctx.matrix_get(4), ref[kind])
        print("%s %s: max error / row scale %.2e" % (which, name, err))
    # the terms are all of a size: the comparison would see a missing one
    assert abs(R.P(w.ravel())).max() > 0.05 * abs(ref[lib.ALE_FIXEDPOINT]).max()
    # scale and slot_add: A = nu * vector Laplacian of the MOVED mesh on the DIAG pattern, then a FULL matrix
    nu, rho = 0.37, 1.9
    ctx.pattern_build(dim, lib.BLOCK_DIAG)
    ctx.assemble(lib.FORM_LAPLACE_VEC)
    ctx.matrix_scale(-1, nu)
    ctx.matrix_store(0)
    Ad = ctx.matrix_get(0)
    for kind, name in _kinds(lib):
        E = ref[kind].copy()
        E.data = rho * E.data
        want = on_pattern([E, Ad], E.shape)
        ctx.assemble_advection_ale(kind, rho, 0, 4)
        F = ctx.matrix_get(4)
        assert_matrix_close(F, want)
        ctx.assemble_advection_ale(kind, -0.5, 4, 2)
        want2 = want.copy()
        want2.data = want.data - 0.5 * ref[kind].data
        assert_matrix_close(ctx.matrix_get(2), want2)


def test_more_elements_than_one_grid_trip(fedd_lib, ctx):
    """10 368 elements against 4 * 2048 waves: the second trip of the element loop, FEDD_ALE_NEWTON only"""
    lib = fedd_lib
    m, mm, d, u, w = _setup(lib, ctx, "cube_p1_trips", amp=0.01)
    assert m["conn"].shape[0] == 10368 > 4 * 2048
    ctx.assemble_advection_ale(lib.ALE_NEWTON, 1.0, -1, 4)
    assert_matrix_close(ctx.matrix_get(4), AleRestatement(lib, mm).ale("Newton", u, w))


@pytest.mark.parametrize("which", MESHES)
def test_zero_mesh_velocity_is_the_fixed_mesh_bit_for_bit(fedd_lib, ctx, which):
    lib = fedd_lib
    m, mm, d, u, w = _setup(lib, ctx, which)
    ctx.mesh_velocity_set(np.zeros_like(w))
    for ale, adv in ((lib.ALE_FIXEDPOINT, lib.ADV_N), (lib.ALE_NEWTON, lib.ADV_NEWTON)):
        ctx.assemble_advection(adv, 1.3, -1, 3)
        ctx.assemble_advection_ale(ale, 1.3, -1, 4)
        a, b = ctx.matrix_get(3), ctx.matrix_get(4)
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        assert np.array_equal(a.data, b.data)
        assert abs(a).max() > 0.0
    ctx.assemble_advection_ale(lib.ALE_P, 1.3, -1, 4)
    assert np.all(ctx.matrix_get(4).data == 0.0)


@pytest.mark.parametrize("which", MESHES)
def test_affine_mesh_velocity(fedd_lib, ctx, which):
    """div (G x + c) = tr(G), x the position under the element map: P is tr(G) times the assembled vector mass matrix (a DIAG matrix, so compared on the diagonal
    component pairs, the rest of P being structural zeros), and with u = w the fixed-point matrix is -P(w)"""
    lib = fedd_lib
    m, mm, d, u, _ = _setup(lib, ctx, which)
    dim = m["dim"]
    rng = np.random.default_rng(23)
    G, c0 = rng.standard_normal((dim, dim)), rng.standard_normal(dim)
    w = affine_positions(mm) @ G.T + c0[None, :]       # affine in every element's own map
    ctx.mesh_velocity_set(w)
    ctx.assemble_advection_ale(lib.ALE_P, 1.0, -1, 4)
    P = ctx.matrix_get(4)
    ctx.pattern_build(dim, lib.BLOCK_DIAG)
    ctx.assemble(lib.FORM_MASS_VEC)
    ctx.matrix_store(0)
    M = ctx.matrix_get(0)
    M.data = np.trace(G) * M.data
    rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    off = (rows % dim) != (P.indices % dim)
    assert np.all(P.data[off] == 0.0)
    Z = P.copy()
    Z.data = np.zeros_like(P.data)
    assert_matrix_close(P, on_pattern([Z, M], P.shape))
    ctx.velocity_set(w)
    ctx.assemble_advection_ale(lib.ALE_FIXEDPOINT, 1.0, -1, 3)
    neg = P.copy()
    neg.data = -P.data
    assert_matrix_close(ctx.matrix_get(3), neg)


@pytest.mark.parametrize("which", ["square_p2", "cube_p2", "cube_p1"])
def test_ale_newton_matrix_is_the_jacobian(fedd_lib, ctx, which):
    """F(u) = (N(u - w) - P(w)) u has the derivative N(u - w) + W(u) - P(w): the direction v enters N(u - w) u through N(v) u =
    W(u) v, with u, not u - w, behind W.  Quotient, step and criterion are those of test_newton_matrix_is_the_jacobian
    (tests/test_gpu_navier_stokes.py), a one-sided quotient, which loses nothing against a central one here because its
    truncation term is known exactly: [F(u + eps v) - F(u)] / eps against the FEDD_ALE_NEWTON matrix times v, all matrices
    from the device; F is quadratic in u, so the quotient differs from the derivative by exactly eps N(v) v, the rest is
    rounding, bounded entry by entry by ops * 2^-53 * (|A| |x|)_i with |A| the restatement with every product replaced by its
    magnitude.  Here |A| gains |P| and the magnitudes behind N are |u| + |w|; ops counts two quadrature sums per entry (N and
    P, or W and P) and three nodal fields.  eps makes the truncation term a tenth of the quotient's rounding term.

    A variant that feeds u - w to W differs from the true Jacobian by W(w) v, which is of the size of the matrix itself: the
    test asserts on the host that this difference exceeds the bound by orders of magnitude for the w used here, and it was
    confirmed once with a planted swap in the kernel (the staged u - w handed to the gradient loop): the planted build failed
    this test on every mesh and passed again after the swap was taken out."""
    lib = fedd_lib
    m = _mesh(lib, which)
    dim, nen = m["dim"], m["conn"].shape[1]
    d = displacement(m)
    mm = moved(m, d)
    R = AleRestatement(lib, mm)
    rng = np.random.default_rng(11)
    n = dim * m["xyz"].shape[0]
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    w = mesh_velocity(mm["xyz"]).ravel() + 0.5 * rng.standard_normal(n)
    ctx.mesh_set_dict(m)
    ctx.mesh_move(d)
    ctx.mesh_velocity_set(w)

    def dev(kind, z):
        ctx.velocity_set(z)
        ctx.assemble_advection_ale(kind, 1.0, -1, 4)
        return ctx.matrix_get(4)

    def Aabs(z):
        return R.N(np.abs(z) + np.abs(w), absolute=True) + R.P(np.abs(w), absolute=True)

    Aabs_u = Aabs(u)
    JabsV = (Aabs_u + R.W(np.abs(u), absolute=True)) @ np.abs(v)
    nq = max(lib.fe_quadrature(dim, dg)[1].shape[0] for dg in degrees(dim, nen))
    deg = np.bincount(m["conn"].ravel()).max()
    rowlen = np.diff(Aabs_u.indptr).max()
    ops = 2 * nq * (dim + 3) + 3 * nen * dim + deg + rowlen
    trunc_unit = np.abs(R.N(v) @ v)
    round_unit = ops * U * 2.0 * (Aabs_u @ np.abs(u))
    eps = float(np.sqrt(0.1 * round_unit.max() / trunc_unit.max()))
    z = u + eps * v
    q = (dev(lib.ALE_FIXEDPOINT, z) @ z - dev(lib.ALE_FIXEDPOINT, u) @ u) / eps
    Jv = dev(lib.ALE_NEWTON, u) @ v
    bound = eps * trunc_unit + ops * U * (Aabs(z) @ np.abs(z) + Aabs_u @ np.abs(u)) / eps + ops * U * JabsV
    err = np.abs(q - Jv)
    swapped = np.abs(R.W(w) @ v)                      # what W(u - w) in the place of W(u) would add to the error
    print("%s: eps %.2e, max error %.2e, max bound %.2e, largest error / bound %.2e, swap / bound %.2e"
          % (which, eps, err.max(), bound.max(), (err / np.maximum(bound, 1e-300)).max(), (swapped / bound).max()))
    assert eps * trunc_unit.max() < (round_unit / eps).max()
    assert np.all(err <= bound)
    assert (swapped / bound).max() > 1e3


def test_mesh_velocity_buffer(fedd_lib, ctx):
    """diff = (d_new - d_old) * (1.0 / dt) bit for bit with a dt whose reciprocal is inexact; set / get; None clears; a move
    keeps it; mesh_set releases it"""
    lib = fedd_lib
    m = _mesh(lib, "cube_p2")
    ctx.mesh_set_dict(m)
    with pytest.raises(lib.FeddError, match="no mesh velocity"):
        ctx.mesh_velocity()
    d_old, d_new = displacement(m, 0.03, 0.2), displacement(m, 0.04, 0.9)
    dt = 0.003
    ctx.mesh_velocity_diff(d_new, d_old, dt)
    want = (d_new - d_old) * (1.0 / dt)
    got = ctx.mesh_velocity()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert not np.array_equal(want, (d_new - d_old) / dt)          # the division would give other bits: the order matters
    w = mesh_velocity(m["xyz"])
    ctx.mesh_velocity_set(w)
    assert np.array_equal(ctx.mesh_velocity(), w)
    ctx.mesh_move(d_new)
    assert np.array_equal(ctx.mesh_velocity(), w)                   # a move keeps it
    ctx.assemble_advection_ale(lib.ALE_P, 1.0, -1, 4)
    ctx.mesh_velocity_set(None)
    with pytest.raises(lib.FeddError, match="no mesh velocity"):
        ctx.assemble_advection_ale(lib.ALE_P, 1.0, -1, 4)
    with pytest.raises(lib.FeddError, match="no mesh velocity"):
        ctx.mesh_velocity()
    ctx.mesh_velocity_set(w)
    ctx.mesh_set_dict(m)                                            # ... and a new mesh releases it
    with pytest.raises(lib.FeddError, match="no mesh velocity"):
        ctx.assemble_advection_ale(lib.ALE_P, 1.0, -1, 4)
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(lib.FeddError, match="time step"):
            ctx.mesh_velocity_diff(d_new, d_old, bad)


@pytest.mark.parametrize("which", ["square_p2", "cube_p1"])
def test_moved_equals_fresh_reproducible_and_no_symbolic_work(fedd_lib, ctx, which):
    """a context moved by d and a fresh context given x_ref + d: the same bits for the three kinds; two calls give the same
    bits; across move + ALE call after the first, the symbolic timer counts no launch"""
    lib = fedd_lib
    m = _mesh(lib, which)
    d0, d = displacement(m, 0.03, 1.1), displacement(m)
    mm = moved(m, d)
    u, w = smooth_velocity(m["xyz"]), mesh_velocity(m["xyz"])
    fresh = lib.Context(device=0)
    try:
        fresh.mesh_set_dict(mm)
        fresh.velocity_set(u)
        fresh.mesh_velocity_set(w)
        want = {}
        for kind, _ in _kinds(lib):
            fresh.assemble_advection_ale(kind, 1.7, -1, 4)
            want[kind] = fresh.matrix_get(4)
    finally:
        fresh.close()
    ctx.timing_enable(True)
    ctx.mesh_set_dict(m)
    ctx.velocity_set(u)
    ctx.mesh_velocity_set(w)
    ctx.mesh_move(d0)
    ctx.assemble_advection_ale(lib.ALE_NEWTON, 1.7, -1, 4)          # the first call on the mesh builds the structures
    ctx.assemble_advection_ale(lib.ALE_P, 1.7, -1, 4)
    before = ctx.timing_get()["symbolic"][1]
    assert before >= 1
    ctx.mesh_move(d)
    for kind, _ in _kinds(lib):
        ctx.assemble_advection_ale(kind, 1.7, -1, 4)
        A = ctx.matrix_get(4)
        assert np.array_equal(A.indptr, want[kind].indptr) and np.array_equal(A.indices, want[kind].indices)
        assert np.array_equal(A.data, want[kind].data)
        ctx.assemble_advection_ale(kind, 1.7, -1, 4)
        assert np.array_equal(ctx.matrix_get(4).data, A.data)      # bit for bit
    assert ctx.timing_get()["symbolic"][1] == before, "the symbolic stage ran again after a move"
    ctx.timing_enable(False)


def test_write_is_recorded_for_the_combine(fedd_lib, ctx):
    lib = fedd_lib
    m, mm, d, u, w = _setup(lib, ctx, "square_p2")
    dim = m["dim"]
    ctx.pattern_build(dim, lib.BLOCK_DIAG)
    ctx.assemble(lib.FORM_MASS_VEC)
    ctx.matrix_store(5)
    ctx.assemble_advection_ale(lib.ALE_FIXEDPOINT, 1.0, -1, 4)
    ctx.matrix_combine(5, 2.0, 4, 1.0)
    assert ctx.matrix_combine_current(5, 2.0, 4, 1.0) == 1
    ctx.assemble_advection_ale(lib.ALE_FIXEDPOINT, 1.0, -1, 4)
    assert ctx.matrix_combine_current(5, 2.0, 4, 1.0) == 0


def test_errors(fedd_lib, ctx):
    lib = fedd_lib
    m = _mesh(lib, "square_p1")
    w = mesh_velocity(m["xyz"])
    with pytest.raises(lib.FeddError, match="fedd_mesh_set first"):
        ctx.assemble_advection_ale(lib.ALE_P, 1.0, -1, 4)
    with pytest.raises(lib.FeddError, match="fedd_mesh_set first"):
        ctx.mesh_velocity_set(w)
    ctx.mesh_set_dict(m)
    with pytest.raises(lib.FeddError, match="no mesh velocity"):
        ctx.assemble_advection_ale(lib.ALE_P, 1.0, -1, 4)
    ctx.mesh_velocity_set(w)
    ctx.assemble_advection_ale(lib.ALE_P, 1.0, -1, 4)               # P needs no velocity
    for kind in (lib.ALE_FIXEDPOINT, lib.ALE_NEWTON):
        with pytest.raises(lib.FeddError, match="no velocity"):
            ctx.assemble_advection_ale(kind, 1.0, -1, 4)
    ctx.velocity_set(smooth_velocity(m["xyz"]))
    ctx.mesh_velocity_set(None)
    with pytest.raises(lib.FeddError, match="no mesh velocity"):
        ctx.assemble_advection_ale(lib.ALE_FIXEDPOINT, 1.0, -1, 4)
    ctx.mesh_velocity_set(w)
    for kind in (-1, 3, 7):
        with pytest.raises(lib.FeddError, match="unknown kind"):
            ctx.assemble_advection_ale(kind, 1.0, -1, 4)
    with pytest.raises(lib.FeddError, match="must differ"):
        ctx.assemble_advection_ale(lib.ALE_NEWTON, 1.0, 4, 4)
    for so in (-1, 7):
        with pytest.raises(lib.FeddError, match="out of range"):
            ctx.assemble_advection_ale(lib.ALE_NEWTON, 1.0, -1, so)
    with pytest.raises(lib.FeddError, match="out of range"):
        ctx.assemble_advection_ale(lib.ALE_NEWTON, 1.0, 7, 4)
    with pytest.raises(lib.FeddError, match="slot 3 is empty"):
        ctx.assemble_advection_ale(lib.ALE_NEWTON, 1.0, 3, 4)
    ctx.pattern_build(1, lib.BLOCK_SCALAR)                          # a scalar matrix is no velocity matrix
    ctx.assemble(lib.FORM_LAPLACE)
    ctx.matrix_store(3)
    with pytest.raises(lib.FeddError, match="does not hold a DIAG or FULL velocity matrix"):
        ctx.assemble_advection_ale(lib.ALE_NEWTON, 1.0, 3, 4)
    two = lib.Context(device=0, rank=0, nranks=2)                   # (no communicator: the rank count alone decides)
    try:
        two.mesh_set_dict(m)
        for call in (lambda: two.mesh_velocity_set(w), lambda: two.mesh_velocity_diff(w, w, 0.1),
                     lambda: two.assemble_advection_ale(lib.ALE_P, 1.0, -1, 4)):
            with pytest.raises(lib.FeddError, match="one rank"):
                call()
    finally:
        two.close()

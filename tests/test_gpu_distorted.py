"""Structured meshes with moved interior nodes: a general mesh to every kernel (the device sees only conn and xyz), on which
the memoisations of the fast paths -- tile shapes of the assembly, row classes of the SpMV, shared Schwarz inverses and the
batch table -- hold only in part or not at all.  Every case checks that the mesh is what it claims (positive element
determinants, the number of distinct local matrices / classes it expects) and compares against the oracle, a
high-precision product or an exact answer, with the defaults choosing the kernels at sizes just above their gates."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import fedd_oracle as fo
from test_gpu_parity import RTOL, assert_matrix_close, csr_global, oracle_mesh

pytestmark = pytest.mark.gpu

M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


def _unit(key):
    """splitmix64 finaliser of uint64 keys -> uniform numbers in [-1, 1)"""
    with np.errstate(over="ignore"):
        z = key + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


def distorted(m, amp, region="all", seed=0, box=(0.0, 1.0), cells=None, planes=1):
    """Copy of a structured_mesh dict whose interior nodes are moved by up to amp * h per coordinate.  The shift is a
    function of (global id, coordinate, seed) alone, so every rank moves a node it shares the same way.  Nodes on the
    boundary of `box` stay put (flags, bounding box and the Schwarz bin lattice are those of the lattice).  region: "all";
    "octant" (nodes below the centre in every coordinate); "slab" (`planes` node planes from x = centre on).  cells: global
    cells per direction (default: the dict's own)."""
    x = m["xyz"]
    dim = x.shape[1]
    lo, hi = box
    h = (hi - lo) / np.asarray(cells if cells is not None else m["cells"], dtype=np.float64)
    tol = 1e-9 * (hi - lo)
    interior = np.all((x > lo + tol) & (x < hi - tol), axis=1)
    c = 0.5 * (lo + hi)
    if region == "all":
        sel = interior
    elif region == "octant":
        sel = interior & np.all(x < c - tol, axis=1)
    elif region == "slab":
        k = (x[:, 0] - c) / h[0] + 0.5
        sel = interior & (k >= 0.0) & (k < planes)
    else:
        raise ValueError(region)
    key = (m["gid_rep"].astype(np.uint64)[:, None] * np.uint64(dim) + np.arange(dim, dtype=np.uint64)[None, :]) \
        ^ (np.uint64(seed) << np.uint64(40))
    out = dict(m)
    out["xyz"] = x + np.where(sel[:, None], amp * h[None, :] * _unit(key), 0.0)
    out["moved"] = sel
    out["det_lattice"] = element_dets(m)
    return out


def element_dets(m):
    x = m["xyz"]
    conn = m["conn"][:, :m["dim"] + 1]
    B = x[conn[:, 1:]] - x[conn[:, :1]]
    return np.linalg.det(B)


def check_mesh(m, min_moved=0.0):
    """every element keeps a positive volume; the elements that touch a moved node (at least the fraction min_moved of
    them) are all different from one another"""
    # (the generator's elements come in both orientations: each keeps the sign of its lattice determinant)
    det = element_dets(m) * np.sign(m["det_lattice"])
    assert det.min() > 0.25 * np.abs(m["det_lattice"]).min(), det.min()
    moved = m["moved"][m["conn"][:, :m["dim"] + 1]].any(axis=1)
    assert moved.any() and moved.mean() >= min_moved, moved.mean()
    x = m["xyz"]
    conn = m["conn"][:, :m["dim"] + 1]
    B = (x[conn[moved, 1:]] - x[conn[moved, :1]]).reshape(int(moved.sum()), -1)
    assert np.unique(B, axis=0).shape[0] == moved.sum()      # no two of them share a geometry
    return moved


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def _interior_rows(m):
    x = m["xyz"]
    return np.flatnonzero(np.all((x > 1e-9) & (x < 1.0 - 1e-9), axis=1))


# ---- 1. assembly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", [1, 0])
@pytest.mark.parametrize("amp", [0.15, 1e-12])
@pytest.mark.parametrize("dim,M", [(3, 15), (2, 63)])     # (64-node tiles: whole node lines, interior tiles share a shape)
def test_assembly_on_a_distorted_mesh(fedd_lib, ctx, dim, M, amp, tiles):
    """P1 Laplace, vector Laplace and elasticity against the oracle, tile kernel and pair kernels; and the identities that
    hold on any mesh: K times a linear function vanishes at interior rows, a constant strain gives no interior forces, the
    mass matrix sums to the volume."""
    m = distorted(fedd_lib.structured_mesh(dim, 1, M), amp, "all", seed=1)
    check_mesh(m, 0.8)
    om = oracle_mesh(m)
    n = om.n_global
    x = m["xyz"]
    inner = _interior_rows(m)
    ctx.mesh_set_dict(m)
    ctx.set_option("asm_tiles", tiles)
    rng = np.random.default_rng(dim)
    ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    ctx.assemble(fedd_lib.FORM_LAPLACE)
    A = csr_global(ctx, n)[0]
    assert_matrix_close(A, fo.assembly_laplace(om))
    u = 0.3 + x @ rng.standard_normal(dim)
    Ku = A @ u
    assert np.abs(Ku[inner]).max() <= 1e-12 * abs(A).max() * np.abs(u).max()
    ctx.assemble(fedd_lib.FORM_MASS)
    Mm = csr_global(ctx, n)[0]
    assert_matrix_close(Mm, fo.assembly_mass(om, "Scalar"))
    assert abs(Mm.sum() - 1.0) <= 1e-13
    ctx.pattern_build(dim, fedd_lib.BLOCK_DIAG)
    ctx.assemble(fedd_lib.FORM_LAPLACE_VEC)
    A = csr_global(ctx, dim * n)[0]
    assert_matrix_close(A, fo.assembly_laplace_vecfield(om))
    U = 0.1 + x @ rng.standard_normal((dim, dim))            # every component linear
    KU = (A @ U.ravel()).reshape(n, dim)
    assert np.abs(KU[inner]).max() <= 1e-12 * abs(A).max() * np.abs(U).max()
    mu, nu = 2.0e6, 0.4
    lam = 2.0 * mu * nu / (1.0 - 2.0 * nu)
    ctx.pattern_build(dim, fedd_lib.BLOCK_FULL)
    ctx.assemble(fedd_lib.FORM_LINELAS, [lam, mu])
    A = csr_global(ctx, dim * n)[0]
    assert_matrix_close(A, fo.assembly_linelas(om, lam, mu))
    G = rng.standard_normal((dim, dim))                      # constant strain (G + G^T) / 2 plus a rotation
    U = rng.standard_normal(dim) + x @ G.T
    KU = (A @ U.ravel()).reshape(n, dim)
    assert np.abs(KU[inner]).max() <= 1e-12 * abs(A).max() * np.abs(U).max()
    ctx.set_option("asm_tiles", 1)


def test_p2_assembly_on_a_distorted_mesh(fedd_lib, ctx):
    """P2 mesh from a distorted P1 mesh (straight edges, moved vertices): Laplace and mass against the oracle"""
    m1 = distorted(fedd_lib.structured_mesh(3, 1, 5), 0.15, "all", seed=2)
    check_mesh(m1, 0.8)
    mv = fedd_lib.p2_of_p1(m1, volume_id=0)
    om = oracle_mesh(mv)
    ctx.mesh_set_dict(mv)
    ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    ctx.assemble(fedd_lib.FORM_LAPLACE)
    assert_matrix_close(csr_global(ctx, om.n_global)[0], fo.assembly_laplace(om))
    ctx.assemble(fedd_lib.FORM_MASS)
    Mm = csr_global(ctx, om.n_global)[0]
    assert_matrix_close(Mm, fo.assembly_mass(om, "Scalar"))
    assert abs(Mm.sum() - 1.0) <= 1e-13


# ---- 2. SpMV at default options -------------------------------------------------------------------------------------------
def _spmv_exact_check(rowptr, col, val, x, y):
    """|y_i - sum_j a_ij x_j| <= gamma_k sum_j |a_ij x_j| for a row of k entries (sum in extended precision), plus what the
    solver's stream leaves out: the entries it drops are at most 2^-52 of their row's largest magnitude (spmv_drop_tol)"""
    n = rowptr.shape[0] - 1
    k = np.diff(rowptr)
    prod = val.astype(np.longdouble) * x[col].astype(np.longdouble)
    ref = np.add.reduceat(prod, rowptr[:-1]) if prod.size else np.zeros(n, np.longdouble)
    ref[k == 0] = 0
    absum = np.add.reduceat(np.abs(prod), rowptr[:-1]).astype(np.float64)
    u = 2.0 ** -53
    gamma = k * u / (1.0 - k * u)
    err = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
    rmax = np.maximum.reduceat(np.abs(val), rowptr[:-1])
    xsum = np.add.reduceat(np.abs(x[col]), rowptr[:-1])
    # (+ the extended-precision reference's own rounding, + the dropped entries)
    bound = gamma * absum + 2.0 ** -60 * absum + 2.0 ** -52 * rmax * xsum
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (bad[:5], err[bad[:5]], bound[bad[:5]])
    # one row in 2000 re-summed exactly
    for i in range(0, n, 2000):
        s = math.fsum(float(a) * float(b) for a, b in zip(val[rowptr[i]:rowptr[i + 1]], x[col[rowptr[i]:rowptr[i + 1]]]))
        assert abs(y[i] - s) <= gamma[i] * absum[i] + 2.0 ** -52 * rmax[i] * xsum[i] + 1e-300


def _laplace_system(fedd_lib, ctx, m):
    ctx.mesh_set_dict(m)
    ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    ctx.assemble(fedd_lib.FORM_LAPLACE)
    ctx.assemble_rhs([1.0])
    ctx.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])


@pytest.mark.parametrize("M,region,planes", [(48, "all", 1), (48, "slab", 1)])
def test_spmv_classes_on_a_distorted_mesh(fedd_lib, ctx, M, region, planes):
    """48^3 cells, 117 649 rows: the class builder runs on its own gate (65 536 rows).  Fully distorted, no row repeats
    another's values and the classes are dropped (more distinct rows than the table's 16 384 classes).  One node plane
    distorted: the rows of three node planes are classes of one row each, next to the lattice's classes.  (The builder
    keys its slots by the values, so classed rows side by side with stream rows arise only once the table overflows, and
    which classes it keeps then is the builder's choice, not a fixed scenario.)  Every row within the rounding bound of its exact sum, the same bits as the
    per-entry kernel (spmv_pattern 0), and again after a reassembly with spmv_keep_dictionary 1, which must drop or
    rebuild the classes the lattice left behind.  (spmv_exact_public 0: fedd_spmv runs the solver's compacted stream.)"""
    lat = fedd_lib.structured_mesh(3, 1, M)
    m = distorted(lat, 0.15, region, seed=3, planes=planes)
    check_mesh(m)
    n = lat["xyz"].shape[0]
    assert n >= 65536
    x = np.random.default_rng(4).standard_normal(n)
    ctx.set_option("spmv_exact_public", 0)
    _laplace_system(fedd_lib, ctx, lat)
    val_lat = ctx.csr_get()[2].copy()
    _laplace_system(fedd_lib, ctx, m)
    rowptr, col, val, _ = ctx.csr_get()
    # rows whose values differ from the lattice's (the Dirichlet rows are unit rows whatever the mesh)
    touched = np.zeros(n, bool)
    touched[np.repeat(np.arange(n), np.diff(rowptr))[val != val_lat]] = True
    y = ctx.spmv(x)
    info = ctx.spmv_info()
    if region == "all":
        assert touched.mean() > 0.8
        assert info["row_classes"] == 0, info
    else:
        assert 0.03 < touched.mean() < 0.1, touched.mean()
        assert info["rows_in_classes"] >= 0.9 * n, info
        # every distorted row a class of its own
        assert info["row_classes"] > touched.sum() and info["rows_in_classes"] == n, info
    _spmv_exact_check(rowptr, col, val, x, y)
    ctx.set_option("spmv_pattern", 0)
    y0 = ctx.spmv(x)
    ctx.set_option("spmv_pattern", 1)
    assert np.array_equal(y, y0)
    # the lattice's classes kept in the dictionary, then the distorted matrix on the same pattern
    ctx.set_option("spmv_keep_dictionary", 1)
    try:
        _laplace_system(fedd_lib, ctx, lat)
        ctx.spmv(x)
        assert ctx.spmv_info()["row_classes"] > 0
        _laplace_system(fedd_lib, ctx, m)
        y1 = ctx.spmv(x)
        info1 = ctx.spmv_info()
    finally:
        ctx.set_option("spmv_keep_dictionary", 0)
    assert info1["row_classes"] == info["row_classes"] and info1["rows_in_classes"] == info["rows_in_classes"], (info1, info)
    assert np.array_equal(y1, y)
    print("spmv M %d %s %d: touched rows %d, %s" % (M, region, planes, touched.sum(), info))


# ---- 3. Schwarz apply at default options ----------------------------------------------------------------------------------
def _elasticity_system(fedd_lib, ctx, m, mu, nu):
    lam = 2.0 * mu * nu / (1.0 - 2.0 * nu)
    ctx.mesh_set_dict(m)
    ctx.pattern_build(3, fedd_lib.BLOCK_FULL)
    ctx.assemble(fedd_lib.FORM_LINELAS, [lam, mu])
    ctx.dirichlet([2], np.zeros(3))
    return fo.linelas_problem(oracle_mesh(m), mu, nu, bc_flags=(2,))[0]


def _schwarz_against_oracle(fedd_lib, ctx, m, A_bc, dofs, target, seed):
    """default apply against fo.RAS (1e-10) and against the unshared inverses (1e-11); returns schwarz_info"""
    node_bin, nb, _ = fo.schwarz_bins(m["xyz"], target)
    r = np.random.default_rng(seed).standard_normal(A_bc.shape[0])
    ctx.schwarz_set_target(target, 1.0)
    ctx.set_option("schwarz_dedupe", 0)
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    z0 = ctx.schwarz_apply(r)
    ctx.set_option("schwarz_dedupe", 1)
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    info = ctx.schwarz_info()
    assert info["n_subdomains"] == nb
    z = ctx.schwarz_apply(r)
    ras = fo.RAS(A_bc, node_bin, nb, dofs=dofs)
    assert ras.max_size == info["max_size"]
    zo = ras.apply(r)
    scale = np.abs(zo).max()
    np.testing.assert_allclose(z, zo, rtol=0, atol=1e-10 * scale)
    np.testing.assert_allclose(z0, zo, rtol=0, atol=1e-10 * scale)
    np.testing.assert_allclose(z, z0, rtol=0, atol=1e-11 * scale)
    info["z"] = z
    info["r"] = r
    return info


@pytest.mark.parametrize("region", ["all", "octant"])
def test_schwarz_laplace_on_a_distorted_mesh(fedd_lib, ctx, region):
    """48^3 cells, 27-node boxes: 4913 subdomains, above the 4096 of the matrix-core gate.  Fully distorted: every local
    matrix is its own (n_unique = n_subdomains), the streaming kernel.  One octant distorted: the rest still share, within
    the 4x gate, so the default takes the matrix-core kernel over a mix of shared and unshared inverses (measured: 792
    distinct of 4913; every box conforms to its representative -- a distorted box is its own --, so that kernel is the
    batch-table one, k_apply_bt)."""
    lat = fedd_lib.structured_mesh(3, 1, 48)
    m = distorted(lat, 0.15, region, seed=5)
    check_mesh(m)
    _laplace_system(fedd_lib, ctx, m)
    A_bc = fo.laplace_problem(oracle_mesh(m))[0]
    info = _schwarz_against_oracle(fedd_lib, ctx, m, A_bc, 1, 27, 6)
    nsub = info["n_subdomains"]
    assert nsub >= 4096
    if region == "all":
        assert info["n_unique"] == nsub, info
    else:
        assert nsub // 8 < info["n_unique"] and info["n_unique"] * 4 <= nsub, info
        # the batch-table and the chunk-record kernels: the same products in the same order
        ctx.set_option("apply_kind", 6)
        try:
            assert np.array_equal(ctx.schwarz_apply(info["r"]), info["z"])
        finally:
            ctx.set_option("apply_kind", 0)
    print("schwarz laplace %s: n_subdomains %d n_unique %d n_conforming %s" % (region, nsub, info["n_unique"], info.get("n_conforming")))


@pytest.mark.parametrize("nu", [0.4, 0.49])
def test_schwarz_elasticity_on_a_distorted_octant(fedd_lib, ctx, nu):
    """Elasticity (mu = 2e6, the headline's nu = 0.4, and nu = 0.49), 32^3 cells, 8-node boxes: 4913 subdomains of up to
    138 dofs; one octant distorted (measured: 1056 distinct local matrices at either nu, every box conforming: k_apply_bt)."""
    lat = fedd_lib.structured_mesh(3, 1, 32)
    m = distorted(lat, 0.15, "octant", seed=7)
    check_mesh(m)
    A_bc = _elasticity_system(fedd_lib, ctx, m, 2.0e6, nu)
    info = _schwarz_against_oracle(fedd_lib, ctx, m, A_bc, 3, 8, 8)
    nsub = info["n_subdomains"]
    assert nsub >= 4096 and nsub // 8 < info["n_unique"] and info["n_unique"] * 4 <= nsub, info
    print("schwarz elasticity nu %g: n_subdomains %d n_unique %d n_conforming %s" % (nu, nsub, info["n_unique"], info.get("n_conforming")))


# ---- 4. the fingerprint's tolerance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", [1e-15, 1e-14, 1e-13, 1e-12])
def test_fingerprint_quantum_on_nearly_equal_local_matrices(fedd_lib, ctx, amp):
    """Elasticity at nu = 0.49 (the worst-conditioned local matrices the project runs), 16^3 cells, 8-node boxes (729
    subdomains), every interior node moved by amp * h: entries that differ from the lattice's by about amp, around the
    fingerprint's quantum of 2^-44 of the row maximum.  Whatever the fingerprints share, the apply is the oracle's.
    Measured n_unique: 64 at 1e-15 (shifts below half an ulp of most coordinates: the lattice's 64 classes), 729 = every
    subdomain at 1e-14, 1e-13 and 1e-12 (the quantised row maxima and entries already tell them apart)."""
    lat = fedd_lib.structured_mesh(3, 1, 16)
    m = distorted(lat, amp, "all", seed=9)
    assert np.array_equal(np.sign(element_dets(m)), np.sign(m["det_lattice"]))
    A_bc = _elasticity_system(fedd_lib, ctx, m, 2.0e6, 0.49)
    info = _schwarz_against_oracle(fedd_lib, ctx, m, A_bc, 3, 8, 10)
    ctx.set_option("apply_kind", 4)       # the matrix-core kernel over the same shared inverses
    try:
        ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        z4 = ctx.schwarz_apply(info["r"])
    finally:
        ctx.set_option("apply_kind", 0)
    np.testing.assert_allclose(z4, info["z"], rtol=0, atol=1e-11 * np.abs(info["z"]).max())
    print("fingerprint amp %g: n_subdomains %d n_unique %d" % (amp, info["n_subdomains"], info["n_unique"]))


def test_transposed_cells_do_not_share_an_inverse(fedd_lib, ctx):
    """Local matrices with the same pattern and the same row maxima but other values must not share an inverse.  A 2D
    grid mapped by x -> g(x), y -> g'(y) with g(t) = t (t <= 1/2), 2 t - 1/2 and g'(t) = 2 t (t <= 1/2), t + 1/2: cells of
    h x 2h in the quadrant x, y < 1/2 and of 2h x h in the quadrant x, y > 1/2 (powers of two: exact arithmetic).  P1
    Laplace rows there have the same diagonal 2 (hx / hy + hy / hx) and the x and y couplings exchanged.  One-node boxes
    (target 1, scale 1/2) + one layer of overlap = the 7-node stencil, the same dof layout in both quadrants."""
    M = 32
    m = dict(fedd_lib.structured_mesh(2, 1, M))
    t = m["xyz"]
    m["xyz"] = np.stack([np.where(t[:, 0] <= 0.5, t[:, 0], 2.0 * t[:, 0] - 0.5),
                         np.where(t[:, 1] <= 0.5, 2.0 * t[:, 1], t[:, 1] + 0.5)], axis=1)
    _laplace_system(fedd_lib, ctx, m)
    A_bc = fo.laplace_problem(oracle_mesh(m))[0]
    rowptr, col, val, _ = ctx.csr_get()
    A = sp.csr_matrix((val, col, rowptr), shape=A_bc.shape)
    i1 = (M + 1) * (M // 4) + M // 4              # lattice node (M/4, M/4): inside the h x 2h quadrant
    i2 = (M + 1) * (3 * M // 4) + 3 * M // 4      # (3M/4, 3M/4): inside the 2h x h quadrant
    # the scenario: equal diagonals, the +x and +y couplings exchanged
    assert A[i1, i1] == A[i2, i2] and A[i1, i1 + 1] == A[i2, i2 + M + 1] and A[i1, i1 + M + 1] == A[i2, i2 + 1]
    assert abs(A[i1, i1 + 1] - A[i1, i1 + M + 1]) > 0.5 * abs(A[i1, i1 + 1])
    node_bin, nb, _ = fo.schwarz_bins(m["xyz"], 1, 0.5)
    assert nb == m["xyz"].shape[0]
    r = np.random.default_rng(17).standard_normal(A_bc.shape[0])
    zo = fo.RAS(A_bc, node_bin, nb).apply(r)
    for kind in (0, 4):
        ctx.set_option("apply_kind", kind)
        ctx.schwarz_set_target(1, 0.5)
        ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        info = ctx.schwarz_info()
        assert info["n_subdomains"] == nb and info["n_unique"] * 4 <= nb, info
        np.testing.assert_allclose(ctx.schwarz_apply(r), zo, rtol=0, atol=1e-10 * np.abs(zo).max())
    ctx.set_option("apply_kind", 0)


# ---- 5. solves --------------------------------------------------------------------------------------------------------------
def test_patch_test_solve_at_default_options(fedd_lib, ctx):
    """Dirichlet values u = a + b.x on every boundary row, no source: the P1 solution is u at the nodes on any mesh"""
    lat = fedd_lib.structured_mesh(3, 1, 48)
    m = distorted(lat, 0.15, "all", seed=11)
    check_mesh(m)
    ctx.mesh_set_dict(m)
    ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    ctx.assemble(fedd_lib.FORM_LAPLACE)
    ctx.assemble_rhs([0.0])
    x = m["xyz"]
    u = 1.0 + x @ np.array([0.5, -0.25, 2.0])
    bnd = np.flatnonzero(~np.all((x > 1e-9) & (x < 1.0 - 1e-9), axis=1))
    ctx.dirichlet_rows(bnd, u[bnd])
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    xs, its, rel = ctx.gmres(None, rtol=1e-13, max_it=500, restart=100, use_prec=True)
    assert rel <= 1e-13
    np.testing.assert_allclose(xs, u, rtol=0, atol=RTOL * np.abs(u).max())
    rowptr, col, val, _ = ctx.csr_get()
    A = sp.csr_matrix((val, col, rowptr), shape=(x.shape[0], x.shape[0]))
    b = ctx.rhs_get()
    assert np.array_equal(b[bnd], u[bnd])
    true_rel = np.linalg.norm(b - A @ xs) / np.linalg.norm(b)
    assert abs(true_rel - rel) <= 0.05 * rel, (true_rel, rel)


@pytest.mark.parametrize("dim,M", [(3, 20), (2, 64)])
def test_solve_matches_the_direct_solve(fedd_lib, ctx, dim, M):
    m = distorted(fedd_lib.structured_mesh(dim, 1, M), 0.15, "all", seed=12)
    check_mesh(m)
    _laplace_system(fedd_lib, ctx, m)
    A_bc, rhs_bc = fo.laplace_problem(oracle_mesh(m))[:2]
    xd = fo.direct_solve(A_bc, rhs_bc)
    target = 27 if dim == 3 else 16
    node_bin, nb, _ = fo.schwarz_bins(m["xyz"], target)
    ras = fo.RAS(A_bc, node_bin, nb)
    _, its_o, _ = fo.gmres_right(A_bc, rhs_bc, ras.apply, rtol=1e-13, max_it=600, restart=200)
    ctx.schwarz_set_target(target, 1.0)
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    try:
        for s in (16, 8):
            for fuse in (1, -1):
                ctx.set_option("gmres_s", s)
                ctx.set_option("gmres_fuse", fuse)
                x, its, rel = ctx.gmres(None, rtol=1e-13, max_it=600, restart=200, use_prec=True)
                assert rel <= 1e-13
                np.testing.assert_allclose(x, xd, rtol=0, atol=RTOL * np.abs(xd).max())
                assert its_o - 2 <= its <= 1.25 * its_o + 2, (s, fuse, its, its_o)
    finally:
        ctx.set_option("gmres_s", 0)
        ctx.set_option("gmres_fuse", -1)


# ---- 6. two levels ----------------------------------------------------------------------------------------------------------
def test_two_level_q1_on_a_distorted_mesh(fedd_lib, ctx):
    m = distorted(fedd_lib.structured_mesh(3, 1, 16), 0.15, "all", seed=13)
    check_mesh(m)
    _laplace_system(fedd_lib, ctx, m)
    A_bc, rhs_bc, _, _, flags = fo.laplace_problem(oracle_mesh(m))
    is_dir = np.isin(flags, (1, 2, 3))
    ctx.schwarz_set_target(27, 1.0)
    ctx.schwarz_set_coarse(200)
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED, two_level=1, coarse_kind=fedd_lib.COARSE_Q1)
    g, Kinv = ctx.schwarz_coarse()
    co = fo.CoarseQ1(A_bc, m["xyz"], is_dir, 1, cells_target=200)
    np.testing.assert_array_equal(g[:3], co.g)
    np.testing.assert_allclose(Kinv, co.K0inv, rtol=0, atol=1e-10 * np.abs(co.K0inv).max())
    node_bin, nb, _ = fo.schwarz_bins(m["xyz"], 27)
    ras = fo.RAS(A_bc, node_bin, nb)
    r = np.random.default_rng(14).standard_normal(A_bc.shape[0])
    zo = ras.apply(r) + co.apply(r)
    np.testing.assert_allclose(ctx.schwarz_apply(r), zo, rtol=0, atol=1e-10 * np.abs(zo).max())
    x, its, rel = ctx.gmres(None, rtol=1e-8, max_it=300, restart=100, use_prec=True)
    _, its_o, _ = fo.gmres_right(A_bc, rhs_bc, lambda v: ras.apply(v) + co.apply(v), rtol=1e-8, max_it=300, restart=100)
    assert abs(its - its_o) <= 1, (its, its_o)


def test_two_level_rgdsw_on_a_distorted_mesh(fedd_lib, ctx):
    m = distorted(fedd_lib.structured_mesh(3, 1, 12), 0.15, "all", seed=15)
    check_mesh(m)
    _laplace_system(fedd_lib, ctx, m)
    A_bc, rhs_bc, _, _, flags = fo.laplace_problem(oracle_mesh(m))
    is_dir = np.isin(flags, (1, 2, 3))
    ctx.schwarz_set_target(27, 1.0)
    ctx.schwarz_set_coarse(27)
    ctx.set_option("gdsw_tol", 1e-13)
    try:
        ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED, two_level=1, coarse_kind=fedd_lib.COARSE_RGDSW)
        g, Kinv = ctx.schwarz_coarse()
    finally:
        ctx.set_option("gdsw_tol", 0)
    co = fo.CoarseGDSW(A_bc, m["conn"], m["xyz"], is_dir, 1, cells_target=27, reduced=True)
    np.testing.assert_array_equal(g[:3], co.g)
    np.testing.assert_allclose(Kinv, co.K0inv, rtol=0, atol=1e-10 * np.abs(co.K0inv).max())
    node_bin, nb, _ = fo.schwarz_bins(m["xyz"], 27)
    ras = fo.RAS(A_bc, node_bin, nb)
    r = np.random.default_rng(16).standard_normal(A_bc.shape[0])
    zo = ras.apply(r) + co.apply(r)
    np.testing.assert_allclose(ctx.schwarz_apply(r), zo, rtol=0, atol=1e-10 * np.abs(zo).max())


# ---- 7. ranks ---------------------------------------------------------------------------------------------------------------
def test_whole_boxes_on_a_distorted_mesh_make_the_preconditioner_independent_of_the_ranks(fedd_lib):
    """test_gpu_multirank's whole-box case on a distorted mesh: 2 x 2 x 2 thread ranks, each moving its nodes by their
    global id, give the one-rank apply and iteration count"""
    import threading
    capi = fedd_lib
    G, dec, target, layers = 12, (2, 2, 2), 27, 4

    def setup(c):
        c.pattern_build(1, capi.BLOCK_SCALAR)
        c.assemble(capi.FORM_LAPLACE)
        c.assemble_rhs([1.0])
        c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
        c.schwarz_set_target(target, 1.0)
        c.schwarz_setup(1, capi.COMBINE_RESTRICTED)

    ref = distorted(capi.structured_mesh(3, 1, G), 0.15, "all", seed=17)
    check_mesh(ref)
    c0 = capi.Context(device=0)
    c0.mesh_set_dict(ref)
    setup(c0)
    r = np.random.default_rng(3).standard_normal(ref["n_global"])
    z_ref = c0.schwarz_apply(r)
    x_ref, its_ref, _ = c0.gmres(None, rtol=1e-10, max_it=500, restart=100, use_prec=True)
    c0.close()
    # ... which is the oracle's operator
    A_bc = fo.laplace_problem(oracle_mesh(ref))[0]
    node_bin, nb, _ = fo.schwarz_bins(ref["xyz"], target)
    zo = fo.RAS(A_bc, node_bin, nb).apply(r)
    np.testing.assert_allclose(z_ref, zo, rtol=0, atol=1e-10 * np.abs(zo).max())
    world = int(np.prod(dec))
    cells = [G // d for d in dec]
    group = capi.ThreadGroup(world)
    out, errs = [None] * world, []

    def rank_main(rank):
        try:
            m = distorted(capi.structured_mesh(3, dec, cells, rank, ghosts=layers), 0.15, "all", seed=17, cells=[G] * 3)
            # (the same moved nodes; the rank's lattice points may differ from the one-rank ones in the last bit)
            assert np.array_equal(m["moved"], ref["moved"][m["gid_rep"]])
            assert np.abs(m["xyz"] - ref["xyz"][m["gid_rep"]]).max() <= 1e-15
            c = capi.Context(device=0, rank=rank, nranks=world, nccl_id=None)
            c.mesh_set_dict(m)
            c.halo_set_owners(m["gid_rep"], capi.structured_owner(3, dec, cells, m["gid_rep"]))
            c.comm_set_thread_group(group)
            setup(c)
            z = c.schwarz_apply(r[m["gid_uni"]])
            x, its, _ = c.gmres(None, rtol=1e-10, max_it=500, restart=100, use_prec=True)
            out[rank] = (m["gid_uni"], z, x, its)
            c.close()
        except Exception as e:      # pragma: no cover
            errs.append(repr(e))
            group._barrier.abort()

    th = [threading.Thread(target=rank_main, args=(k,)) for k in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    z, x = np.zeros_like(z_ref), np.zeros_like(x_ref)
    for gu, zz, xx, its in out:
        z[gu] = zz
        x[gu] = xx
        assert its == its_ref
    np.testing.assert_allclose(z, z_ref, rtol=0, atol=1e-13 * np.abs(z_ref).max())
    np.testing.assert_allclose(x, x_ref, rtol=0, atol=1e-9 * np.abs(x_ref).max())


# ---- options ----------------------------------------------------------------------------------------------------------------
def test_no_option_value_leaves_schwarz_apply_without_a_kernel(fedd_lib, ctx):
    """No value of an option may make schwarz_apply return with z not written.  The development option apply_dbg (ablation
    and phase-clock kernels; an unlisted value launched nothing and returned the previous z) is gone: every value is an
    unknown key.  apply_kind takes the kernel families schwarz_apply has and nothing else, and each of them writes z: on the
    smallest shared-inverse case of the suite (test_gpu_dedupe.CASES[0]) the apply of 2 r is twice the apply of r to the
    bit (scaling by two is exact), which a kernel that did not run cannot give."""
    for v in (2, 5, 1000, -2, 0.5) + (-1, 1, 3, 4, 7, 23, 32, 39, 55) + (0,):
        with pytest.raises(fedd_lib.FeddError, match="apply_dbg"):
            ctx.set_option("apply_dbg", v)
    for v in (3, 5, 7, 8, -1, 0.5):
        with pytest.raises(fedd_lib.FeddError, match="apply_kind"):
            ctx.set_option("apply_kind", v)
    kinds = (0, 1, 2, 4, 6)
    for v in kinds:
        ctx.set_option("apply_kind", v)
    ctx.set_option("apply_kind", 0)
    m = fedd_lib.structured_mesh(3, 1, 14)
    _laplace_system(fedd_lib, ctx, m)
    ctx.schwarz_set_target(27, 1.0)
    ctx.set_option("schwarz_dedupe", 1)
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    info = ctx.schwarz_info()
    assert info["n_unique"] * 4 <= info["n_subdomains"], info
    r = np.random.default_rng(19).standard_normal(m["n_global"])
    try:
        for kind in kinds:
            ctx.set_option("apply_kind", kind)
            z = ctx.schwarz_apply(r)
            assert np.all(z[_interior_rows(m)] != 0.0), kind
            assert np.array_equal(ctx.schwarz_apply(2.0 * r), 2.0 * z), kind
    finally:
        ctx.set_option("apply_kind", 0)

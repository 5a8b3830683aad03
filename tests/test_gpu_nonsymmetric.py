"""Schwarz, the coarse levels and GMRES on matrices whose free-free block is NOT symmetric -- what every Newton, fixed-point and
BDF step of Navier-Stokes hands to them, and what the operator-level tests (Laplace, elasticity, Stokes) never do: there a
transposed local inverse, a transposed K0^-1 or a row/column slip in a Galerkin product passes unseen, and inside a solve it
only costs iterations.

System 1 (not merged): the velocity block of a BDF step, cm M + nu L + rho (N + W)(u) on the FULL pattern, built with the
existing entry points (pattern_build DIAG, assemble, matrix_scale, matrix_store, velocity_set, assemble_advection,
matrix_combine, dirichlet), nu = 0.05, rho = 1, cm = 2; "smooth" velocity: every local matrix differs, "constant": W = 0 and a
structured mesh repeats its local matrices.  System 2: the merged P2 / P1 Newton matrix of steady Navier-Stokes on the 1k
cylinder.  The references (fo.RAS, fo.CoarseQ1, fo.CoarseGDSW, fo.gmres_right, fo.direct_solve: float64 numpy / scipy, plain
inverses and products, no symmetry assumed anywhere -- CoarseGDSW's only Cholesky sweep runs on the Gram matrix Phi^T Phi of
the rotation columns, which are off here) operate on the matrix READ BACK from the device, so assembly is not tested again.
tests/test_nonsymmetric_inputs.py shows on the host that these inputs tell A from its symmetric part and from its transpose
and that elimination without row exchanges is safe on them.

Tolerances are the project's: 1e-10 max |reference| for operator applications and K0^-1, 1e-11 between two device paths, RTOL
for solves.  3 dofs per node: a box of `target` nodes with its overlap can exceed the 256 dofs of the dense local solver, the
library then shrinks the box edge by 0.85 (lattice_bins restates that rule; box count and largest size are asserted equal)."""
import numpy as np
import pytest
import scipy.sparse as sp

import fedd_oracle as fo
from test_gpu_dedupe import CASES as DEDUPE_CASES
from test_gpu_navier_stokes import NavierStokesABI, _cylinder
from test_gpu_parity import RTOL, assert_matrix_close
from test_navier_stokes_abi import smooth_velocity
from test_nonsymmetric_inputs import (CM, COMBINES, NU, Q1_CASES, RAS_CASES, RHO, host_system, lattice_bins,
                                      subdomain_sizes, velocity)

pytestmark = pytest.mark.gpu


def combine_id(L, combine):
    return {"restricted": L.COMBINE_RESTRICTED, "averaging": L.COMBINE_AVERAGING, "full": L.COMBINE_FULL}[combine]


def device_system(L, c, dim, M, which="smooth"):
    """system 1 on context c; returns (mesh, the matrix read back, mask of the Dirichlet rows)"""
    m = L.structured_mesh(dim, 1, M)
    c.mesh_set_dict(m)
    c.pattern_build(dim, L.BLOCK_DIAG)
    c.assemble(L.FORM_LAPLACE_VEC)
    c.matrix_scale(-1, NU)
    c.matrix_store(0)
    c.assemble(L.FORM_MASS_VEC)
    c.matrix_store(5)
    c.velocity_set(velocity(which, m["xyz"]))
    c.assemble_advection(L.ADV_NEWTON, RHO, 0, 4)
    c.matrix_combine(5, CM, 4, 1.0)
    c.dirichlet([1, 2, 3])
    return m, read_back(c), fo.dirichlet_rows(m["flag_uni"], (1, 2, 3), dofs=dim)


def read_back(c):
    rowptr, col, val, gid = c.csr_get()
    n = rowptr.shape[0] - 1
    assert np.array_equal(gid[:n], np.arange(n))               # one rank: owned order = global order
    A = sp.csr_matrix((val, col, rowptr), shape=(n, n))
    A.sort_indices()
    return A


def rel_err(z, zo):
    return float(np.abs(z - zo).max() / np.abs(zo).max())


def true_relres(A, b, x):
    return float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))


def bisection_bins(A, xyz_dof, target):
    """the boxes of the large-subdomain path: fo.rcb_bins of the dofs' carrying nodes, the target lowered (x 0.7) until every
    box with one graph layer fits 1024 dofs"""
    while True:
        bins, nb = fo.rcb_bins(xyz_dof, target)
        if subdomain_sizes(A, bins, nb, 1, 1).max() <= 1024:
            return bins, nb
        target = max(1, int(target * 0.7))


# ---- a: the one-level operator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,M,target,overlap", RAS_CASES)
def test_one_level_operator_matches_the_oracle(fedd_lib, dim, M, target, overlap):
    """restricted, averaging and full; the three apply families of the unshared slabs; both local-inverse kernels (inv_kind 1
    works on the transpose by design).  Largest subdomains and the register-tile class (32, 64, 96, 112, 128, 144, 160 dofs) of
    the inversion they land in: 46 -> 64, 81 -> 96, 138 -> 144 (boxes of 40 and of 64 nodes are refined to the same lattice), 124
    -> 128, 238 -> the variant past 160; with two layers of overlap 86 -> 96 and 195 -> past 160.
    Measured: at most 1.4e-15 of max |z| over all combinations."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m, A, _ = device_system(L, c, dim, M)
        node_bin, nb, largest = lattice_bins(A, m["xyz"], target, dim, overlap)
        ras = fo.RAS(A, node_bin, nb, dofs=dim, overlap=overlap)
        assert ras.max_size == largest
        r = np.random.default_rng(3).standard_normal(A.shape[0])
        c.schwarz_set_target(target, 1.0)
        worst = 0.0
        for inv_kind in (0, 1):
            c.set_option("inv_kind", inv_kind)
            for combine in COMBINES:
                c.schwarz_setup(overlap, combine_id(L, combine))
                info = c.schwarz_info()
                assert info["n_subdomains"] == nb and info["max_size"] == ras.max_size
                ras.combine = combine
                zo = ras.apply(r)
                for apply_kind in ((0, 1, 2) if combine == "restricted" else (0,)):      # (the option picks the restricted apply only)
                    c.set_option("apply_kind", apply_kind)
                    z = c.schwarz_apply(r)
                    err = rel_err(z, zo)
                    worst = max(worst, err)
                    print("dim %d M %d target %d overlap %d inv_kind %d %s apply_kind %d: error %.2e"
                          % (dim, M, target, overlap, inv_kind, combine, apply_kind, err))
                    np.testing.assert_allclose(z, zo, rtol=0, atol=1e-10 * np.abs(zo).max())      # measured <= 1.4e-15
        print("worst %.2e" % worst)
    finally:
        c.set_option("apply_kind", 0)
        c.set_option("inv_kind", 0)
        c.close()


# ---- b: shared inverses ------------------------------------------------------------------------------------------------------
def box_lists(A, node_bin, nb, dofs, overlap):
    """(owned dofs, overlap dofs) of every box, as fo.RAS lists them (each sorted), from two sparse products"""
    n = A.shape[0]
    G = A.copy()
    G.data = np.ones_like(G.data)
    P0 = sp.csr_matrix((np.ones(n), (np.arange(n), np.repeat(node_bin, dofs))), shape=(n, nb))
    Pk = P0
    for _ in range(overlap):
        Pk = G @ Pk + Pk
        Pk.data[:] = 1.0
    P0, Pk = P0.tocsc(), Pk.tocsc()
    out = []
    for b in range(nb):
        own = np.sort(P0.indices[P0.indptr[b]:P0.indptr[b + 1]])
        allr = np.sort(Pk.indices[Pk.indptr[b]:Pk.indptr[b + 1]])
        out.append((own, np.setdiff1d(allr, own, assume_unique=True)))
    return out


def one_box_per_local_matrix(A, lists):
    """Boxes grouped by their local matrix, one representative each.  Two boxes fall into one group when their dof lists agree up to
    a shift and their rows carry the same fingerprint (the row's values weighted by a function of the column offset, to nine
    digits of the matrix scale): a grouping that only decides WHICH boxes meet the oracle, nothing is compared through it."""
    row = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    fp = np.zeros(A.shape[0])
    np.add.at(fp, row, A.data * np.cos(1.0 + 0.37 * (A.indices - row)))
    fp = np.round(fp / np.abs(A.data).max(), 9)
    reps = {}
    for b, (own, ext) in enumerate(lists):
        idx = np.concatenate([own, ext])
        reps.setdefault((own.shape[0], (idx - idx[0]).tobytes(), fp[idx].tobytes()), b)
    return sorted(reps.values())


def restricted_rows_of_boxes(A, lists, boxes, r):
    """fo.RAS's restricted operator on the owned rows of the given boxes only (they depend on their own box alone): the same
    lists, the same principal submatrix, the same np.linalg.inv -- for meshes whose thousands of boxes the full oracle would take
    minutes to invert"""
    rows, vals = [], []
    for b in boxes:
        own, ext = lists[b]
        idx = np.concatenate([own, ext])
        Ainv = np.linalg.inv(A[idx][:, idx].toarray())
        rows.append(own)
        vals.append(Ainv[:own.shape[0]] @ r[idx])
    return np.concatenate(rows), np.concatenate(vals)


# the 3D Laplace entries of test_gpu_dedupe.CASES, and two 2D meshes that 5 x 5- and 6 x 6-node boxes tile evenly (the constant
# velocity has no mirror symmetry: boxes of unequal size would leave too few equal local matrices): with 3 dofs per node the 3D lattices are refined
# to boxes of 1, 8 and 27 nodes, which reach the rows (2, 10), (2, 16) and (6, 16) of the launch table; the 2D ones add (4, 10)
SHARED_CASES = [(3,) + (t[2], t[3], t[4]) for t in DEDUPE_CASES if t[0] == "laplace" and t[1] == 3] + [(2, 64, 25, 1), (2, 65, 36, 1)]


@pytest.mark.parametrize("dim,M,target,overlap", SHARED_CASES)
def test_shared_inverses_on_a_translation_invariant_operator(fedd_lib, dim, M, target, overlap):
    """constant velocity: schwarz_dedupe 1 with the batch-table kernel (apply_kind 4) and the chunk records (6) against the
    unshared path and the oracle.  Largest box (owned dofs + overlap = size) and the row (row tiles, column steps) of the launch
    table it takes: 3D M = 14, both targets, the same lattice: 24 + 114 = 138, (2, 10); M = 26, one-node boxes with two layers:
    3 + 192 = 195, (2, 16); M = 27, 3 x 3 x 3 nodes: 81 + 111 = 192, (6, 16); 2D 5 x 5 nodes: 50 + 44 = 94, (4, 10); 2D 6 x 6 nodes: 72 + 52 = 124,
    (6, 16).  The oracle inverts every box up to 1000 boxes and one box per distinct local matrix beyond (one_box_per_local_matrix).
    Measured: 1.9e-15 of max |z| against the oracle, 1.7e-15 against the unshared path."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m, A, _ = device_system(L, c, dim, M, "constant")
        node_bin, nb, largest = lattice_bins(A, m["xyz"], target, dim, overlap)
        r = np.random.default_rng(M + target).standard_normal(A.shape[0])
        c.schwarz_set_target(target, 1.0)
        c.set_option("schwarz_dedupe", 0)
        c.set_option("apply_kind", 0)
        c.schwarz_setup(overlap, L.COMBINE_RESTRICTED)
        info0 = c.schwarz_info()
        assert info0["n_unique"] == info0["n_subdomains"] == nb and info0["max_size"] == largest
        z0 = c.schwarz_apply(r)
        c.set_option("schwarz_dedupe", 1)
        c.set_option("apply_kind", 4)
        c.schwarz_setup(overlap, L.COMBINE_RESTRICTED)
        info = c.schwarz_info()
        assert info["n_subdomains"] == nb and info["max_size"] == largest
        assert info["n_unique"] * 4 <= info["n_subdomains"], info
        z4 = c.schwarz_apply(r)
        scale = np.abs(z0).max()
        print("dim %d M %d target %d overlap %d: %d boxes, %d distinct, largest %d dofs (%d owned); shared against unshared %.2e"
              % (dim, M, target, overlap, nb, info["n_unique"], largest, dim * np.bincount(node_bin).max(),
                 np.abs(z4 - z0).max() / scale))
        np.testing.assert_allclose(z4, z0, rtol=0, atol=1e-11 * scale)                      # measured 1.7e-15
        assert np.array_equal(c.schwarz_apply(r), z4)
        c.set_option("apply_kind", 6)
        assert np.array_equal(c.schwarz_apply(r), z4)
        if nb <= 1000:
            zo = fo.RAS(A, node_bin, nb, dofs=dim, overlap=overlap).apply(r)
            rows = np.arange(A.shape[0])
        else:
            lists = box_lists(A, node_bin, nb, dim, overlap)
            boxes = one_box_per_local_matrix(A, lists)
            assert len(boxes) >= info["n_unique"]           # every inverse the device keeps meets the reference
            rows, zo = restricted_rows_of_boxes(A, lists, boxes, r)
            print("    %d of %d boxes, one per distinct local matrix" % (len(boxes), nb))
        for z in (z4, z0):
            print("    against the oracle (%d rows): %.2e" % (rows.shape[0], np.abs(z[rows] - zo).max() / scale))
            np.testing.assert_allclose(z[rows], zo, rtol=0, atol=1e-10 * scale)               # measured 1.9e-15
        c.set_option("apply_kind", 0)       # the flat kernel on the shared slabs
        np.testing.assert_allclose(c.schwarz_apply(r), z0, rtol=0, atol=1e-11 * scale)
    finally:
        c.set_option("schwarz_dedupe", 1)
        c.set_option("apply_kind", 0)
        c.close()


# ---- c: the large-subdomain path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combine", ["restricted", "averaging"])
def test_large_subdomain_path_matches_the_oracle(fedd_lib, combine):
    """schwarz_big 1, 150 owned dofs per box of the bisection (boxes per DOF: a node's three dofs may part), 3D M = 8.
    16 boxes, the largest 432 dofs.  Measured: 1.4e-15."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m, A, _ = device_system(L, c, 3, 8)
        c.set_option("schwarz_big", 1)
        c.set_option("schwarz_big_target", 150)
        c.schwarz_setup(1, combine_id(L, combine))
        info = c.schwarz_info()
        bins, nb = bisection_bins(A, np.repeat(m["xyz"], 3, axis=0), 150)
        ras = fo.RAS(A, bins, nb, overlap=1, combine=combine)
        assert info["n_subdomains"] == nb and info["max_size"] == ras.max_size
        assert 256 < ras.max_size <= 1024
        r = np.random.default_rng(5).standard_normal(A.shape[0])
        z, zo = c.schwarz_apply(r), ras.apply(r)
        print("large-subdomain path, %s: %d boxes, largest %d dofs, error %.2e" % (combine, nb, ras.max_size, rel_err(z, zo)))
        np.testing.assert_allclose(z, zo, rtol=0, atol=1e-10 * np.abs(zo).max())             # measured 1.4e-15
    finally:
        c.set_option("schwarz_big", -1)
        c.set_option("schwarz_big_target", 0)
        c.close()


# ---- d: park and gather ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combine", ["full", "averaging"])
def test_gather_apply_matches_the_oracle(fedd_lib, combine):
    """apply_gather 1: sum_i R_i^T A_i^-1 R_i (over the multiplicity for averaging) is defined for any A; k_full_park alone
    (apply_full_kind 1) and with the matrix-core kernel asked for (2: no inverse is shared here, every box stays on k_full_park).
    Measured: 2.3e-16."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m, A, _ = device_system(L, c, 3, 6)
        node_bin, nb, _ = lattice_bins(A, m["xyz"], 8, 3, 1)
        ras = fo.RAS(A, node_bin, nb, dofs=3, overlap=1, combine=combine)
        c.schwarz_set_target(8, 1.0)
        c.schwarz_setup(1, combine_id(L, combine))
        assert c.schwarz_info()["n_subdomains"] == nb and c.schwarz_info()["max_size"] == ras.max_size
        r = np.random.default_rng(3).standard_normal(A.shape[0])
        zo = ras.apply(r)
        z_atomic = c.schwarz_apply(r)
        c.set_option("apply_gather", 1)
        for kind in (1, 2):
            c.set_option("apply_full_kind", kind)
            z = c.schwarz_apply(r)
            fi = c.schwarz_full_info()
            print("gather %s, apply_full_kind %d: %r, error %.2e" % (combine, kind, fi, rel_err(z, zo)))
            assert fi["n_mfma"] + fi["n_plain"] == nb
            np.testing.assert_allclose(z, zo, rtol=0, atol=1e-10 * np.abs(zo).max())         # measured 2.3e-16
            np.testing.assert_allclose(z, z_atomic, rtol=0, atol=1e-11 * np.abs(zo).max())
            assert np.array_equal(c.schwarz_apply(r), z)
    finally:
        c.set_option("apply_gather", 0)
        c.set_option("apply_full_kind", 0)
        c.close()


# ---- e: the Q1 coarse level --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,M,target,cells", Q1_CASES)
def test_q1_coarse_level_matches_the_oracle(fedd_lib, dim, M, target, cells):
    """K0 = Phi^T A Phi is not symmetric here (the host companion: K0^-1 is 0.17 ... 0.25 of its size away from its transpose),
    so the Galerkin product, the gather, the dense inverse, its row- or column-major read in the dense product, restriction
    and prolongation are all pinned.  Multiplicative combination: z = y - Pc A y, y = M1^-1 r, with A the read-back matrix.
    Measured: K0^-1 2.0e-15, coarse apply 1.4e-15, additive 7.7e-16, multiplicative 1.5e-15."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m, A, is_dir = device_system(L, c, dim, M)
        c.schwarz_set_target(target, 1.0)
        c.schwarz_set_coarse(cells)
        c.schwarz_setup(1, L.COMBINE_RESTRICTED, two_level=1, coarse_kind=L.COARSE_Q1)
        g, Kinv = c.schwarz_coarse()
        co = fo.CoarseQ1(A, m["xyz"], is_dir, dim, cells_target=cells)
        np.testing.assert_array_equal(g[:dim], co.g)
        assert Kinv.shape == (co.n0, co.n0)
        asym = np.abs(co.K0inv - co.K0inv.T).max() / np.abs(co.K0inv).max()
        print("dim %d M %d cells %d: n0 %d, K0^-1 error %.2e (its distance from its transpose: %.2e)"
              % (dim, M, cells, co.n0, rel_err(Kinv, co.K0inv), asym))
        assert asym > 1e-3
        np.testing.assert_allclose(Kinv, co.K0inv, rtol=0, atol=1e-10 * np.abs(co.K0inv).max())      # measured 2.0e-15
        node_bin, nb, _ = lattice_bins(A, m["xyz"], target, dim, 1)
        ras = fo.RAS(A, node_bin, nb, dofs=dim)
        assert c.schwarz_info()["n_subdomains"] == nb and c.schwarz_info()["max_size"] == ras.max_size
        r = np.random.default_rng(5).standard_normal(A.shape[0])
        zc, zco = c.schwarz_coarse_apply(r), co.apply(r)
        np.testing.assert_allclose(zc, zco, rtol=0, atol=1e-10 * np.abs(zco).max())                  # measured 1.4e-15
        y = ras.apply(r)
        z_add, zo_add = c.schwarz_apply(r), y + zco
        np.testing.assert_allclose(z_add, zo_add, rtol=0, atol=1e-10 * np.abs(zo_add).max())         # measured 7.7e-16
        c.schwarz_set_level_combination(L.LEVELS_MULTIPLICATIVE)
        z_mult, zo_mult = c.schwarz_apply(r), y - co.apply(A @ y)
        assert np.abs(co.apply(A @ y)).max() > 1e-6 * np.abs(zo_mult).max()      # the coarse correction is not negligible
        np.testing.assert_allclose(z_mult, zo_mult, rtol=0, atol=1e-10 * np.abs(zo_mult).max())      # measured 1.5e-15
        print("    coarse apply %.2e, additive %.2e, multiplicative %.2e"
              % (rel_err(zc, zco), rel_err(z_add, zo_add), rel_err(z_mult, zo_mult)))
    finally:
        c.schwarz_set_level_combination(L.LEVELS_ADDITIVE)
        c.close()


# ---- f: GDSW and RGDSW -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gdsw", "rgdsw"])
def test_gdsw_coarse_levels_match_the_oracle(fedd_lib, kind):
    """the interior extensions -A_II^-1 A_IGamma Phi_Gamma (device GMRES to 1e-13 against the oracle's sparse LU) and the
    Galerkin product, translations only.  Measured: K0^-1 4.4e-15, coarse apply 2.0e-13 (the extension solves stop at 1e-13)."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m, A, is_dir = device_system(L, c, 3, 8)
        reduced = kind == "rgdsw"
        c.schwarz_set_target(8, 1.0)
        c.schwarz_set_coarse(8)
        c.set_option("gdsw_tol", 1e-13)
        c.set_option("gdsw_rotations", 0)
        c.schwarz_setup(1, L.COMBINE_RESTRICTED, two_level=1, coarse_kind=L.COARSE_RGDSW if reduced else L.COARSE_GDSW)
        g, Kinv = c.schwarz_coarse()
        co = fo.CoarseGDSW(A, m["conn"], m["xyz"], is_dir, 3, cells_target=8, reduced=reduced)
        np.testing.assert_array_equal(g[:3], co.g)
        assert Kinv.shape == (co.n0, co.n0) and co.nns == 3
        asym = np.abs(co.K0inv - co.K0inv.T).max() / np.abs(co.K0inv).max()
        assert asym > 1e-3
        r = np.random.default_rng(5).standard_normal(A.shape[0])
        zc, zco = c.schwarz_coarse_apply(r), co.apply(r)
        print("%s: n0 %d, K0^-1 error %.2e (distance from its transpose %.2e), coarse apply %.2e"
              % (kind, co.n0, rel_err(Kinv, co.K0inv), asym, rel_err(zc, zco)))
        np.testing.assert_allclose(Kinv, co.K0inv, rtol=0, atol=1e-10 * np.abs(co.K0inv).max())      # measured 4.4e-15
        np.testing.assert_allclose(zc, zco, rtol=0, atol=1e-10 * np.abs(zco).max())                  # measured 2.0e-13
    finally:
        c.set_option("gdsw_tol", 0.0)
        c.close()


# ---- g: the merged Navier-Stokes matrix --------------------------------------------------------------------------------------
@pytest.mark.parametrize("combine", ["restricted", "averaging"])
def test_monolithic_schwarz_on_the_newton_matrix_of_the_1k_cylinder(fedd_lib, combine):
    """P2 / P1, F = A + rho (N + W)(u) merged with B, B^T at a state that carries the inflow and a smooth interior velocity;
    viscosity 0.01 as in the flow test.  Boxes of the bisection as in the Stokes test: 512 boxes, the
    largest 811 dofs.  Measured: 2.0e-15."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m1, mv, rows, vals = _cylinder(L)
        ns = NavierStokesABI(L, c, m1, mv, 0.01, 1.0, rows, vals)
        x = np.zeros(ns.n)
        x[:3 * ns.nv] = 0.3 * smooth_velocity(mv["xyz"]).ravel()
        x[rows] = vals
        ns.system(L.ADV_NEWTON, x)
        c.dirichlet_rows(rows, vals)
        A = read_back(c)
        free = np.ones(ns.n, dtype=bool)
        free[rows] = False
        Fv = A[:3 * ns.nv][:, :3 * ns.nv][free[:3 * ns.nv]][:, free[:3 * ns.nv]]
        assert abs(Fv - Fv.T).max() > 0.05 * abs(Fv).max()
        c.schwarz_setup(overlap=1, combine=combine_id(L, combine))
        info = c.schwarz_info()
        xyz_dof = np.concatenate([np.repeat(mv["xyz"], 3, axis=0), m1["xyz"]], axis=0)
        bins, nb = bisection_bins(A, xyz_dof, 120)
        ras = fo.RAS(A, bins, nb, overlap=1, combine=combine)
        assert info["n_subdomains"] == nb and info["max_size"] == ras.max_size and 256 < ras.max_size <= 1024
        r = np.random.default_rng(9).standard_normal(ns.n)
        z, zo = c.schwarz_apply(r), ras.apply(r)
        print("merged Navier-Stokes, %s: %d boxes, largest %d dofs, error %.2e" % (combine, nb, ras.max_size, rel_err(z, zo)))
        np.testing.assert_allclose(z, zo, rtol=0, atol=1e-10 * np.abs(zo).max())             # measured 2.0e-15
    finally:
        c.close()


# ---- h: GMRES ----------------------------------------------------------------------------------------------------------------
def test_gmres_forms_take_the_oracles_iterations(fedd_lib):
    """3D M = 10, 27-node boxes (refined to fit), restricted one-level Schwarz: DCGS2, CGS2, s-step with blocks of 8 and of 16
    (four sweeps and fused) take the iterations of fo.gmres_right with the oracle's preconditioner (+-1) at 1e-8, report the
    true residual, and reach the direct solution within RTOL when driven to 1e-13.  Measured: oracle 14 iterations, device 14
    in every form (21 at 1e-13); reported and true residual agree to four digits; solution error 1.1e-13; with the coarse
    level 17 / 17."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m, A, is_dir = device_system(L, c, 3, 10)
        b = np.random.default_rng(7).standard_normal(A.shape[0])
        b[is_dir] = 0.0
        c.rhs_set(b)
        node_bin, nb, _ = lattice_bins(A, m["xyz"], 27, 3, 1)
        ras = fo.RAS(A, node_bin, nb, dofs=3)
        c.schwarz_set_target(27, 1.0)
        c.schwarz_setup(1, L.COMBINE_RESTRICTED)
        assert c.schwarz_info()["n_subdomains"] == nb and c.schwarz_info()["max_size"] == ras.max_size
        _, its_o, _ = fo.gmres_right(A, b, ras.apply, rtol=1e-8, max_it=300, restart=100)
        xd = fo.direct_solve(A, b)
        for gk, s, fuse in ((0, 0, -1), (1, 0, -1), (2, 8, -1), (2, 16, 0), (2, 16, 1)):
            c.set_option("gmres_kind", gk)
            c.set_option("gmres_s", s)
            c.set_option("gmres_fuse", fuse)
            x, its, rel = c.gmres(None, rtol=1e-8, max_it=300, restart=100, use_prec=True)
            tr = true_relres(A, b, x)
            x13, its13, rel13 = c.gmres(None, rtol=1e-13, max_it=300, restart=100, use_prec=True)
            err = rel_err(x13, xd)
            print("gmres_kind %d s %d fuse %d: %d iterations (oracle %d), reported %.3e true %.3e; at 1e-13: %d iterations, "
                  "solution error %.2e" % (gk, s, fuse, its, its_o, rel, tr, its13, err))
            assert abs(its - its_o) <= 1, (its, its_o)
            assert tr <= 1e-8 and abs(rel - tr) <= 1e-3 * tr
            assert rel13 <= 1e-13
            np.testing.assert_allclose(x13, xd, rtol=0, atol=RTOL * np.abs(xd).max())         # measured 1.1e-13
        # ... and with the Q1 coarse level of 27 cells added (default solver): the oracle's count with the oracle's two levels
        c.set_option("gmres_kind", 2)
        c.set_option("gmres_s", 0)
        c.set_option("gmres_fuse", -1)
        c.schwarz_set_coarse(27)
        c.schwarz_setup(1, L.COMBINE_RESTRICTED, two_level=1, coarse_kind=L.COARSE_Q1)
        co = fo.CoarseQ1(A, m["xyz"], is_dir, 3, cells_target=27)
        _, its_o2, _ = fo.gmres_right(A, b, lambda v: ras.apply(v) + co.apply(v), rtol=1e-8, max_it=300, restart=100)
        x, its, rel = c.gmres(None, rtol=1e-8, max_it=300, restart=100, use_prec=True)
        tr = true_relres(A, b, x)
        print("two levels: %d iterations (oracle %d), reported %.3e true %.3e" % (its, its_o2, rel, tr))
        assert abs(its - its_o2) <= 1, (its, its_o2)
        assert tr <= 1e-8 and abs(rel - tr) <= 1e-3 * tr
    finally:
        c.set_option("gmres_kind", 2)
        c.set_option("gmres_s", 0)
        c.set_option("gmres_fuse", -1)
        c.close()


def test_newton_basis_with_complex_ritz_pairs(fedd_lib):
    """unpreconditioned, 3D M = 12, blocks of 16: the Hessenberg matrix of the first block has complex conjugate eigenvalues
    (asserted on the oracle's side: the Arnoldi matrix of the same operator and start), so the shifts come from their real
    parts and the Leja order sees pairs.  Same iterations as the monomial basis (+-1), fewer blocks, true residual below the
    tolerance.  Measured: 43 / 43 iterations, 6 / 4 blocks."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m, A, is_dir = device_system(L, c, 3, 12)
        b = np.random.default_rng(7).standard_normal(A.shape[0])
        b[is_dir] = 0.0
        c.rhs_set(b)
        # Arnoldi on the host: 16 steps from b
        V = np.zeros((17, b.shape[0]))
        H = np.zeros((17, 16))
        V[0] = b / np.linalg.norm(b)
        for j in range(16):
            w = A @ V[j]
            for _ in range(2):
                h = V[:j + 1] @ w
                w = w - h @ V[:j + 1]
                H[:j + 1, j] += h
            H[j + 1, j] = np.linalg.norm(w)
            V[j + 1] = w / H[j + 1, j]
        ritz = np.linalg.eigvals(H[:16])
        assert np.abs(ritz.imag).max() > 1e-3 * np.abs(ritz).max(), ritz
        c.set_option("gmres_kind", 2)
        c.set_option("gmres_s", 16)
        out = {}
        for newton in (0, 1):
            c.set_option("gmres_newton", newton)
            x, its, rel = c.gmres(None, rtol=1e-8, max_it=400, restart=100, use_prec=False)
            out[newton] = (x, its, c.gmres_info()["blocks"])
            tr = true_relres(A, b, x)
            print("gmres_newton %d: %d iterations, %d blocks, reported %.3e true %.3e" % (newton, its, out[newton][2], rel, tr))
            assert rel <= 1e-8 and tr <= 1e-8
        assert abs(out[0][1] - out[1][1]) <= 1 and out[1][2] < out[0][2], [(o[1], o[2]) for o in out.values()]
        np.testing.assert_allclose(out[1][0], out[0][0], rtol=0, atol=1e-7 * np.abs(out[0][0]).max())
    finally:
        c.set_option("gmres_newton", 1)
        c.set_option("gmres_s", 0)
        c.close()


# ---- i: products, and CG on a system it is not made for ----------------------------------------------------------------------
def test_products_and_cg_on_the_nonsymmetric_system(fedd_lib):
    """The read-back matrix is the one the host companion analysed (RTOL of the row scale).  spmv and matrix_apply against scipy
    products of the read-back matrices.  fedd_cg refuses the system by its breakdown message (its first direction probes
    p.A(Ap) against (Ap).(Ap)); before the probe existed it saw no breakdown, since the symmetric part is positive definite, and
    ran its 300 iterations while the residual grew to 48 times its start (394 times preconditioned)."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m, A, is_dir = device_system(L, c, 3, 6)
        assert_matrix_close(A, host_system(L, m)[0])
        rng = np.random.default_rng(7)
        x = rng.standard_normal(A.shape[0])
        y, yo = c.spmv(x), A @ x
        np.testing.assert_allclose(y, yo, rtol=0, atol=RTOL * np.abs(yo).max())
        F = c.matrix_get(4)
        assert abs(F - F.T).max() > 0.1 * abs(F).max()
        y, yo = c.matrix_apply(4, x, -0.75), -0.75 * (F @ x)
        np.testing.assert_allclose(y, yo, rtol=0, atol=RTOL * np.abs(yo).max())
        b = rng.standard_normal(A.shape[0])
        b[is_dir] = 0.0
        c.rhs_set(b)
        c.schwarz_set_target(8, 1.0)
        c.schwarz_setup(1, L.COMBINE_FULL)
        for use_prec in (False, True):
            with pytest.raises(L.FeddError, match=r"breakdown \(operator not symmetric\).*fedd_gmres"):
                c.cg(None, rtol=1e-8, max_it=300, use_prec=use_prec)
            assert c.cg_info() == {"replacements": 0, "breakdown": 4}        # FEDD_CG_BREAKDOWN_NONSYMMETRIC
        # ... and the refusal is about the matrix, not about the context: the symmetric part cm M + nu L alone is solved
        c.matrix_combine(5, CM, 0, 1.0)
        c.dirichlet([1, 2, 3])
        S = read_back(c)
        c.rhs_set(b)
        c.schwarz_setup(1, L.COMBINE_FULL)
        xc, its, rel = c.cg(None, rtol=1e-10, max_it=300, use_prec=True)
        assert c.cg_info()["breakdown"] == 0 and rel <= 1e-10 and true_relres(S, b, xc) <= 1.05e-10
    finally:
        c.close()

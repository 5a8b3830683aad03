"""Preconditioned CG (fedd_cg, cg.hip) and the symmetric Schwarz apply without floating-point atomics (schwarz_sym.hip:
k_full_park, k_full_park_mfma, k_full_gather) against the CPU oracle: the apply against fo.RAS for both park kernels, the shapes
the matrix-core kernel meets, bitwise reproducibility, symmetry, solves against fo.direct_solve, iterates against a numpy PCG
that restates the normative algorithm of include/fedd_hip.h, initial guesses, the errors, and the default paths untouched.
Tolerances are DESIGN section 2: 1e-10 of the largest magnitude against oracle and direct solve, iteration counts +-2."""
import collections

import numpy as np
import pytest

import fedd_oracle as fo
from test_gpu_level_combination import elasticity_setup
from test_gpu_parity import oracle_mesh
from test_gpu_two_level import laplace_setup

pytestmark = pytest.mark.gpu

_CACHE = {}


def problem(fedd_lib, c, kind, dim, M, bc_value=0.0):
    """sets the problem up on the context; the oracle's matrix, rhs, Dirichlet rows and node coordinates (cached)"""
    if kind == "laplace":
        m, om, A, b, is_dir = laplace_setup(fedd_lib, c, dim, M)
        dofs = 1
        if bc_value != 0.0:
            c.assemble_rhs([1.0])
            c.dirichlet([1, 2, 3], [bc_value] * 3)
            key = (kind, dim, M, bc_value)
            if key not in _CACHE:
                _CACHE[key] = fo.laplace_problem(om, bc_value=bc_value)[:2]
            A, b = _CACHE[key]
    else:
        m, om, A, b, is_dir = elasticity_setup(fedd_lib, c, M)
        dofs = 3
    return m, A, b, np.asarray(is_dir, dtype=bool), dofs


def oracle_ras(m, A, dofs, target, combine, key):
    k = key + (target, combine)
    if k not in _CACHE:
        node_bin, nb, _ = fo.schwarz_bins(m["xyz"][:m["gid_uni"].shape[0]], target)
        _CACHE[k] = (fo.RAS(A, node_bin, nb, dofs=dofs, overlap=1, combine=combine), nb)
    return _CACHE[k]


APPLY_CASES = [("laplace", 3, 8, 27, "full"), ("laplace", 3, 8, 27, "averaging"), ("laplace", 3, 12, 27, "full"),
               ("laplace", 2, 30, 16, "full"), ("elasticity", 3, 8, 8, "full")]


@pytest.mark.parametrize("kind,dim,M,target,combine", APPLY_CASES)
def test_gather_apply_matches_oracle(fedd_lib, kind, dim, M, target, combine):
    """"apply_gather" = 1 through fedd_schwarz_apply: k_full_park only (kind 1) and the matrix-core kernel wherever an inverse
    is shared (kind 2), each within 1e-10 max|z| of the oracle and within 1e-13 max|z| of each other; two applies of the same
    r agree bit for bit"""
    c = fedd_lib.Context(device=0)
    try:
        m, A, b, is_dir, dofs = problem(fedd_lib, c, kind, dim, M)
        ras, nb = oracle_ras(m, A, dofs, target, combine, (kind, dim, M))
        c.schwarz_set_target(target, 1.0)
        c.schwarz_setup(1, fedd_lib.COMBINE_FULL if combine == "full" else fedd_lib.COMBINE_AVERAGING)
        assert c.schwarz_info()["n_subdomains"] == nb
        c.set_option("apply_gather", 1)
        r = np.random.default_rng(3).standard_normal(A.shape[0])
        zo = ras.apply(r)
        z = {}
        for k in (1, 2):
            c.set_option("apply_full_kind", k)
            z[k] = c.schwarz_apply(r)
            fi = c.schwarz_full_info()
            print(kind, dim, M, combine, "kind", k, fi, "err %.2e" % (np.abs(z[k] - zo).max() / np.abs(zo).max()))
            assert fi["n_mfma"] + fi["n_plain"] == nb
            if k == 1:
                assert fi["n_mfma"] == 0
            np.testing.assert_allclose(z[k], zo, rtol=0, atol=1e-10 * np.abs(zo).max())
            np.testing.assert_array_equal(c.schwarz_apply(r), z[k])
        print("kind 1 vs 2: %.2e" % (np.abs(z[1] - z[2]).max() / np.abs(zo).max()))
        np.testing.assert_allclose(z[1], z[2], rtol=0, atol=1e-13 * np.abs(zo).max())
    finally:
        c.close()


def test_matrix_core_kernel_shapes(fedd_lib):
    """Laplace (3, M = 12, target 27): 13 nodes per direction in 5 boxes of 2 or 3 nodes, 125 subdomains.  By the oracle's bins
    (grouping the boxes by size and local inverse): 64 distinct local matrices, 27 of them with a single member (the plain
    kernel: 27 of 125 subdomains, under the cap of a quarter), the others with 2, 4 or 8 members -- every matrix-core batch
    is a tail batch of fewer than 16 -- and sizes 46 ... 60, none a multiple of 16 (a 125-dof box does not occur on this
    lattice: its boxes hold at most 3 nodes per direction).  The device must agree, so the test cannot pass by never
    entering k_full_park_mfma."""
    c = fedd_lib.Context(device=0)
    try:
        m, A, b, is_dir, dofs = problem(fedd_lib, c, "laplace", 3, 12)
        ras, nb = oracle_ras(m, A, 1, 27, "full", ("laplace", 3, 12))
        cnt = collections.Counter()
        for idx, n_own, Ai in ras.subs:
            cnt[(idx.shape[0], np.round(Ai / np.abs(Ai).max(), 9).tobytes())] += 1
        members = sorted(cnt.values())
        shared_sizes = [k[0] for k, v in cnt.items() if v >= 2]
        assert members[0] == 1 and any(2 <= v < 16 for v in members)
        assert all(n % 16 != 0 for n in shared_sizes)
        singles = sum(1 for v in members if v == 1)
        c.schwarz_set_target(27, 1.0)
        c.schwarz_setup(1, fedd_lib.COMBINE_FULL)
        info = c.schwarz_info()
        assert info["n_subdomains"] == nb == 125
        assert info["n_unique"] == len(cnt)
        c.set_option("apply_full_kind", 2)
        fi = c.schwarz_full_info()
        print(info, fi, "oracle classes", len(cnt), "single", singles)
        assert fi["n_plain"] == singles and fi["n_mfma"] == nb - singles
        assert 1 <= fi["n_plain"] <= nb // 4
    finally:
        c.close()


@pytest.mark.parametrize("two_level", [0, 1])
@pytest.mark.parametrize("combine", ["full", "averaging"])
def test_apply_is_reproducible(fedd_lib, combine, two_level):
    c = fedd_lib.Context(device=0)
    try:
        m, A, b, is_dir, dofs = problem(fedd_lib, c, "laplace", 3, 12)
        c.schwarz_set_target(27, 1.0)
        c.schwarz_setup(1, fedd_lib.COMBINE_FULL if combine == "full" else fedd_lib.COMBINE_AVERAGING, two_level=two_level,
                        coarse_kind=fedd_lib.COARSE_Q1 if two_level else 0)
        c.set_option("apply_gather", 1)
        r = np.random.default_rng(11).standard_normal(A.shape[0])
        for k in (1, 2):
            c.set_option("apply_full_kind", k)
            z0 = c.schwarz_apply(r)
            for _ in range(3):
                np.testing.assert_array_equal(c.schwarz_apply(r), z0)
    finally:
        c.close()


@pytest.mark.parametrize("kind,M,target,level", [("laplace", 12, 27, "one"), ("laplace", 12, 27, "q1"), ("laplace", 12, 27, "gdsw"),
                                                 ("elasticity", 8, 8, "one"), ("elasticity", 8, 8, "q1"), ("elasticity", 8, 8, "gdsw")])
def test_preconditioner_is_symmetric(fedd_lib, kind, M, target, level):
    """|u^T M^-1 v - v^T M^-1 u| <= 1e-12 |u^T M^-1 v| for seeded random u, v that vanish on the Dirichlet rows"""
    c = fedd_lib.Context(device=0)
    try:
        m, A, b, is_dir, dofs = problem(fedd_lib, c, kind, 3, M)
        c.schwarz_set_target(target, 1.0)
        if level == "gdsw":
            c.set_option("gdsw_tol", 1e-13)
        ck = {"one": 0, "q1": fedd_lib.COARSE_Q1, "gdsw": fedd_lib.COARSE_GDSW}[level]
        c.schwarz_setup(1, fedd_lib.COMBINE_FULL, two_level=int(level != "one"), coarse_kind=ck)
        c.set_option("apply_gather", 1)
        rng = np.random.default_rng(5)
        u = rng.standard_normal(A.shape[0]) * ~is_dir
        v = rng.standard_normal(A.shape[0]) * ~is_dir
        a, bb = u @ c.schwarz_apply(v), v @ c.schwarz_apply(u)
        print(kind, level, "asymmetry %.2e" % (abs(a - bb) / abs(a)))
        assert abs(a - bb) <= 1e-12 * abs(a)
    finally:
        c.close()


SOLVE_CASES = [("laplace", 3, 12, 27, "none", 0.0), ("laplace", 3, 12, 27, "one", 0.0), ("laplace", 3, 12, 27, "q1", 0.0),
               ("laplace", 2, 32, 16, "one", 0.0), ("elasticity", 3, 8, 8, "q1", 0.0), ("laplace", 3, 12, 27, "one", 1.0)]


@pytest.mark.parametrize("kind,dim,M,target,level,bc_value", SOLVE_CASES)
def test_cg_solves_to_the_direct_solution(fedd_lib, kind, dim, M, target, level, bc_value):
    c = fedd_lib.Context(device=0)
    try:
        m, A, b, is_dir, dofs = problem(fedd_lib, c, kind, dim, M, bc_value)
        if level != "none":
            c.schwarz_set_target(target, 1.0)
            c.schwarz_setup(1, fedd_lib.COMBINE_FULL, two_level=int(level == "q1"), coarse_kind=fedd_lib.COARSE_Q1 if level == "q1" else 0)
        x, its, rel = c.cg(None, rtol=1e-13, max_it=2000, use_prec=level != "none")
        xd = fo.direct_solve(A, b)
        print(kind, dim, M, level, bc_value, "its", its, "relres %.2e" % rel, c.cg_info(), "err %.2e" % (np.abs(x - xd).max() / np.abs(xd).max()))
        assert rel <= 1e-13
        np.testing.assert_allclose(x, xd, rtol=0, atol=1e-10 * np.abs(xd).max())
        x2, its2, rel2 = c.cg(None, rtol=1e-13, max_it=2000, use_prec=level != "none")
        np.testing.assert_array_equal(x2, x)
        assert its2 == its and rel2 == rel
    finally:
        c.close()


def numpy_pcg(A, b, is_dir, prec, rtol, max_it, x0=None):
    """the normative algorithm of fedd_cg (include/fedd_hip.h), lift included"""
    x = np.zeros_like(b) if x0 is None else x0.copy()
    den = np.linalg.norm(b - A @ x)
    mask = (~is_dir).astype(float)
    x[is_dir] = b[is_dir]
    r = b - A @ x
    if np.linalg.norm(r) <= rtol * den:
        return x, 0
    z = prec(r)
    p = mask * z
    rho = r @ z
    for it in range(1, max_it + 1):
        q = A @ p
        alpha = rho / (p @ q)
        x += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) <= rtol * den:
            break
        z = prec(r)
        rho, rho_old = r @ z, rho
        p = mask * (z + (rho / rho_old) * p)
    return x, it


@pytest.mark.parametrize("bc_value", [0.0, 1.0])
def test_cg_iterates_match_the_numpy_restatement(fedd_lib, bc_value):
    c = fedd_lib.Context(device=0)
    try:
        m, A, b, is_dir, dofs = problem(fedd_lib, c, "laplace", 3, 12, bc_value)
        ras, nb = oracle_ras(m, A, 1, 27, "full", ("laplace", 3, 12))
        c.schwarz_set_target(27, 1.0)
        c.schwarz_setup(1, fedd_lib.COMBINE_FULL)
        x5, its5, _ = c.cg(None, rtol=1e-30, max_it=5, use_prec=True)
        y5, _ = numpy_pcg(A, b, is_dir, ras.apply, 1e-30, 5)
        assert its5 == 5
        np.testing.assert_allclose(x5, y5, rtol=0, atol=1e-10 * np.abs(y5).max())
        x, its, rel = c.cg(None, rtol=1e-8, max_it=500, use_prec=True)
        y, its_np = numpy_pcg(A, b, is_dir, ras.apply, 1e-8, 500)
        print("bc", bc_value, "device", its, "numpy", its_np)
        assert abs(its - its_np) <= 2 and rel <= 1e-8
    finally:
        c.close()


def test_one_subdomain_converges_in_one_iteration(fedd_lib):
    c = fedd_lib.Context(device=0)
    try:
        m, A, b, is_dir, dofs = problem(fedd_lib, c, "laplace", 3, 4)
        c.schwarz_set_target(10 ** 6, 1.0)
        c.schwarz_setup(1, fedd_lib.COMBINE_FULL)
        assert c.schwarz_info()["n_subdomains"] == 1
        x, its, rel = c.cg(None, rtol=1e-8, max_it=50, use_prec=True)
        assert its == 1 and rel <= 1e-8
    finally:
        c.close()


def test_cg_initial_guess(fedd_lib):
    c = fedd_lib.Context(device=0)
    try:
        m, A, b, is_dir, dofs = problem(fedd_lib, c, "laplace", 3, 12)
        c.schwarz_set_target(27, 1.0)
        c.schwarz_setup(1, fedd_lib.COMBINE_FULL)
        xd = fo.direct_solve(A, b)
        x, its, rel = c.cg_x0(xd, rtol=1e-10, max_it=500, use_prec=True)
        assert its == 0
        np.testing.assert_array_equal(x, xd)
        x0 = xd + 1e-3 * np.abs(xd).max() * np.random.default_rng(9).standard_normal(xd.shape[0])
        x, its, rel = c.cg_x0(x0, rtol=1e-10, max_it=500, use_prec=True)
        assert its > 0 and rel <= 1e-10
        np.testing.assert_allclose(x, xd, rtol=0, atol=1e-10 * np.abs(xd).max())
        # relres refers to the perturbed guess's residual
        true_rel = np.linalg.norm(b - A @ x) / np.linalg.norm(b - A @ x0)
        assert abs(rel - true_rel) <= 0.1 * rel
    finally:
        c.close()


def _merged_stokes(fedd_lib, c):
    """the merged Taylor-Hood system of test_gpu_stokes.test_small_stokes_solve (4 x 4 cells)"""
    m1 = fedd_lib.structured_mesh(2, 1, 4)
    mv = fedd_lib.p2_of_p1(m1, volume_id=0)
    n_p, nv = m1["xyz"].shape[0], mv["xyz"].shape[0]
    c.mesh_set_dict(mv)
    c.pattern_build(2, fedd_lib.BLOCK_DIAG)
    c.assemble(fedd_lib.FORM_LAPLACE_VEC)
    c.matrix_store(0)
    c.assemble_div(n_p, 1, 2)
    c.matrix_scale(1, -1.0)
    c.matrix_scale(2, -1.0)
    c.block_merge(0, 2, 1, -1)
    X = mv["xyz"]
    nodes = np.nonzero((X[:, 0] < 1e-12) | (X[:, 1] < 1e-12) | (X[:, 1] > 1 - 1e-12))[0]
    rows = np.concatenate([2 * nodes, 2 * nodes + 1])
    c.rhs_set(np.ones(2 * nv + n_p))
    c.dirichlet_rows(rows, np.zeros(rows.shape[0]))


def test_cg_errors_leave_gmres_untouched(fedd_lib):
    c, f = fedd_lib.Context(device=0), fedd_lib.Context(device=0)
    try:
        for cc in (c, f):
            problem(fedd_lib, cc, "laplace", 3, 12)
            cc.schwarz_set_target(27, 1.0)
        c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        with pytest.raises(fedd_lib.FeddError, match="not symmetric: use FEDD_COMBINE_FULL"):
            c.cg(None, use_prec=True)
        c.schwarz_setup(1, fedd_lib.COMBINE_AVERAGING)
        with pytest.raises(fedd_lib.FeddError, match="not symmetric: use FEDD_COMBINE_FULL"):
            c.cg(None, use_prec=True)
        c.schwarz_setup(1, fedd_lib.COMBINE_FULL, two_level=1, coarse_kind=fedd_lib.COARSE_Q1)
        c.schwarz_set_level_combination(fedd_lib.LEVELS_MULTIPLICATIVE)
        with pytest.raises(fedd_lib.FeddError, match="FEDD_LEVELS_MULTIPLICATIVE"):
            c.cg(None, use_prec=True)
        c.schwarz_set_level_combination(fedd_lib.LEVELS_ADDITIVE)
        c.set_option("schwarz_big", 1)
        c.schwarz_setup(1, fedd_lib.COMBINE_FULL)
        with pytest.raises(fedd_lib.FeddError, match="large-subdomain path"):
            c.cg(None, use_prec=True)
        c.set_option("schwarz_big", -1)
        c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        f.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        xa, ia, ra = c.gmres(None, rtol=1e-10, max_it=300, restart=100, use_prec=True)
        xb, ib, rb = f.gmres(None, rtol=1e-10, max_it=300, restart=100, use_prec=True)
        np.testing.assert_array_equal(xa, xb)
        assert ia == ib and ra == rb
    finally:
        c.close()
        f.close()
    s = fedd_lib.Context(device=0)
    try:
        _merged_stokes(fedd_lib, s)
        with pytest.raises(fedd_lib.FeddError, match="merged block system"):
            s.cg(None, use_prec=False)
    finally:
        s.close()


def test_default_paths_did_not_move(fedd_lib):
    """a context that used the new options and kernels, back on the defaults, against one that never touched them: the
    restricted apply and GMRES agree bit for bit"""
    c, f = fedd_lib.Context(device=0), fedd_lib.Context(device=0)
    try:
        for cc in (c, f):
            m, A, b, is_dir, dofs = problem(fedd_lib, cc, "laplace", 3, 12)
            cc.schwarz_set_target(27, 1.0)
        c.schwarz_setup(1, fedd_lib.COMBINE_FULL)
        c.set_option("apply_gather", 1)
        c.set_option("apply_full_kind", 2)
        r = np.random.default_rng(2).standard_normal(A.shape[0])
        c.schwarz_apply(r)
        c.cg(None, rtol=1e-8, max_it=100, use_prec=True)
        c.set_option("apply_gather", 0)
        c.set_option("apply_full_kind", 0)
        c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        f.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        np.testing.assert_array_equal(c.schwarz_apply(r), f.schwarz_apply(r))
        xa, ia, ra = c.gmres(None, rtol=1e-10, max_it=300, restart=100, use_prec=True)
        xb, ib, rb = f.gmres(None, rtol=1e-10, max_it=300, restart=100, use_prec=True)
        np.testing.assert_array_equal(xa, xb)
        assert ia == ib and ra == rb
    finally:
        c.close()
        f.close()
